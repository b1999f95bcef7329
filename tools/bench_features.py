"""capf_backward vs capf_backward_maps in both summation modes on one engine, in one process (EXPERIMENTS.md R12.1, R15.1).

HRNet-32, fp32, 256 x 256, batches 64 and 512: one capf_forward_train, then the three backwards -- capf_backward, capf_backward_maps
with atomic adds (capf_set_map_grad_mode 0) and with the ordered sum (mode 1) -- alternate on its saved activations (a
backward only reads them), each call bracketed by device events; medians and (max - min) / median over the repeats.  Also printed: the
bytes the map gradient adds with atomics (every in-range corner of every deformable sample and of every reference point, 4 bytes per
channel) and the rate that the time difference implies, next to the chip-wide rate of fp32 atomic adds (about 1.3 TB/s of added bytes).

    python tools/bench_features.py [--batches 64 512] [--repeats 20] [--warmup 3]        (needs the MI355X)
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "contextaware-poseformer_amd"))

import torch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_features.py needs the MI355X"
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
        dfeat = [torch.empty(B, h, w, c, device="cuda") for h, w, c in eng.feature_shapes()]
        dout = torch.randn(B, 1, 17, 3, generator=torch.Generator().manual_seed(3)).cuda() / (17 * B)
        eng.forward_train(img, k2d, kc, out, s, None)
        def maps(mode):
            eng.set_map_grad_mode(mode)                     # (a host-side state change, outside the events)
            return lambda: eng.backward_maps(dout, flat, dfeat, s, None)

        runs = {"backward": lambda: (lambda: eng.backward(dout, flat, s, None)),
                "backward_maps": lambda: maps(0),
                "backward_maps_ordered": lambda: maps(1)}
        times = {k: [] for k in runs}
        for it in range(args.warmup + args.repeats):
            for name, prepare in runs.items():                  # alternating: all see the same drift of the box
                run = prepare()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                if it >= args.warmup:
                    times[name].append(e0.elapsed_time(e1))
        med = {k: statistics.median(v) for k, v in times.items()}
        spread = {k: (max(v) - min(v)) / med[k] for k, v in times.items()}
        C = sum(c for _, _, c in eng.feature_shapes())
        # upper count: every corner in range (a clamped +1 corner and a reference corner outside the map add nothing)
        added = B * 17 * (4 * 16 * 4 + 4) * C * 4
        extra_ms = med["backward_maps"] - med["backward"]
        extra_ordered_ms = med["backward_maps_ordered"] - med["backward"]
        eng.set_map_grad_mode(0)
        zeroed = sum(t.numel() for t in dfeat) * 4
        print(json.dumps({"batch": B, "backward_ms": round(med["backward"], 4), "backward_maps_ms": round(med["backward_maps"], 4),
                          "backward_maps_ordered_ms": round(med["backward_maps_ordered"], 4),
                          "spread": {k: round(v, 4) for k, v in spread.items()}, "extra_ms": round(extra_ms, 4),
                          "extra_ordered_ms": round(extra_ordered_ms, 4),
                          "atomic_bytes": added, "zeroed_bytes": zeroed,
                          "atomic_TBps_if_all_extra_time": round(added / (extra_ms * 1e-3) / 1e12, 3) if extra_ms > 0 else None,
                          "ms_at_1.3TBps": round(added / 1.3e12 * 1e3, 4), "repeats": args.repeats}))


if __name__ == "__main__":
    main()
