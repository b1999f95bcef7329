"""What the keypoint gradients cost: capf_backward_points against capf_backward_maps and capf_backward on one engine, in one process
(EXPERIMENTS.md R23.1).

HRNet-32, fp32, 256 x 256, batches 64 and 512: one capf_forward_train, then the backwards alternate on its saved activations (a backward
only reads them), each call bracketed by device events; medians and (max - min) / median over the repeats:

    backward              capf_backward
    backward_maps         capf_backward_maps (the handle's map-gradient mode: atomic unless --ordered)
    backward_points       capf_backward_points with all three outputs (the four maps, dk2d, dref)
    backward_points_kp    capf_backward_points with dk2d and dref only (what _LifterStep runs on an image source: no map gradient)

    python tools/bench_points_grad.py [--batches 64 512] [--repeats 20] [--warmup 3] [--ordered]        (needs the MI355X)

--only backward --package <checkout>/contextaware-poseformer_amd times capf_backward alone through the package of ANOTHER checkout (the
parent commit, built in place): run it in the same session, before and after, to see that capf_backward did not move.
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--ordered", action="store_true", help="capf_set_map_grad_mode 1 for the map gradients")
    ap.add_argument("--only", choices=["backward"], default=None)
    ap.add_argument("--package", default=os.path.join(ROOT, "contextaware-poseformer_amd"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.package))
    import torch
    assert torch.cuda.is_available(), "bench_points_grad.py needs the MI355X"
    from capf import synth
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), "hrnet_32")
    cfg.model.backbone.fix_weights = True
    model = CA_PF(cfg)
    synth.load_synthetic(model, seed=1, bn_mode="random")
    model = model.cuda()
    model.train(); model.backbone.eval()
    for B in args.batches:
        img, k2d, kc, gt = synth.synth_inputs(B, 256, 256, seed=2, crop_range=(192, 256), with_gt=True)
        img, k2d, kc = img.cuda(), k2d.cuda(), kc.cuda()
        eng = model.engine_for(img)
        s = torch.cuda.current_stream().cuda_stream
        _, total = eng.grad_layout_cached()
        out, flat = torch.empty(B, 1, 17, 3, device="cuda"), torch.empty(total, device="cuda")
        dout = torch.randn(B, 1, 17, 3, generator=torch.Generator().manual_seed(3)).cuda() / (17 * B)
        eng.forward_train(img, k2d, kc, out, s, None)
        runs = {"backward": lambda: eng.backward(dout, flat, s, None)}
        if args.only is None:
            eng.set_map_grad_mode(1 if args.ordered else 0)
            dfeat = [torch.empty(B, h, w, c, device="cuda") for h, w, c in eng.feature_shapes()]
            dk2d, dref = torch.empty(B, 17, 2, device="cuda"), torch.empty(B, 17, 2, device="cuda")
            runs["backward_maps"] = lambda: eng.backward_maps(dout, flat, dfeat, s, None)
            runs["backward_points"] = lambda: eng.backward_points(dout, flat, s, None, dfeat, dk2d, dref)
            runs["backward_points_kp"] = lambda: eng.backward_points(dout, flat, s, None, None, dk2d, dref)
        times = {k: [] for k in runs}
        for it in range(args.warmup + args.repeats):
            for name, run in runs.items():                      # alternating: all see the same drift of the box
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
        med = {k: statistics.median(v) for k, v in times.items()}
        row = {"batch": B, "package": os.path.abspath(args.package), "map_grad_mode": int(args.ordered), "repeats": args.repeats}
        row.update({k + "_ms": round(v, 4) for k, v in med.items()})
        row["spread"] = {k: round((max(v) - min(v)) / med[k], 4) for k, v in times.items()}
        if args.only is None:
            row["points_minus_maps_ms"] = round(med["backward_points"] - med["backward_maps"], 4)
            row["points_kp_minus_backward_ms"] = round(med["backward_points_kp"] - med["backward"], 4)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
