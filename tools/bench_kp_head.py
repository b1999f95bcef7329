"""What the native 2-D keypoint head costs (EXPERIMENTS.md R24.1): capf_kp_head_forward in both decodes and capf_kp_head_backward on the
feat0 of an engine, next to capf_backbone_forward of the same handle and to the byte floor of one read of feat0; then forward_detect
against forward on given keypoints.  One process, device events around every call, the calls alternating so that all see the same drift of
the machine; medians with min / max over the repeats.

    python tools/bench_kp_head.py [--configs hrnet_32:fp32:64 hrnet_32:fp32:512 hrnet_48:fp16:256] [--repeats 20] [--warmup 3]   (needs the MI355X)

The floor is feat0's bytes over --hbm-gbs (default 4000 GB/s, roughly what a streaming read reaches on an MI355X); the backward reads the
map three times (statistics, dz, the dW products) and, with dmap, writes it once.
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def timed(runs, repeats, warmup):
    import torch
    times = {k: [] for k in runs}
    for it in range(warmup + repeats):
        for name, run in runs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            if it >= warmup:
                times[name].append(e0.elapsed_time(e1))
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", nargs="+", default=["hrnet_32:fp32:64", "hrnet_32:fp32:512", "hrnet_48:fp16:256"], help="backbone:dtype:batch")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--hbm-gbs", type=float, default=4000.0)
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(ROOT, "contextaware-poseformer_amd"))
    import numpy as np
    import torch
    assert torch.cuda.is_available(), "bench_kp_head.py needs the MI355X"
    from capf import lib as capf
    from capf import synth
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    for spec in args.configs:
        backbone, dtype, B = spec.split(":")
        B = int(B)
        cfg = backbone_preset(copy.deepcopy(config), backbone)
        cfg.model.backbone.fix_weights = True
        model = CA_PF(cfg, compute_dtype=dtype, keypoint_head="integral", keypoint_beta=2.0)
        synth.load_synthetic(model, seed=1, bn_mode="random")
        model = model.cuda().eval()
        img, k2d, kc = (t.cuda() for t in synth.synth_inputs(B, 256, 256, seed=2, crop_range=(192, 256)))
        A = torch.from_numpy(np.stack([capf.crop_to_image_matrix((500.0, 500.0), (1.5, 1.5), (256, 256), 1000, 1000)] * B).astype(np.float32)).cuda()
        eng = model.engine_for(img)
        s = torch.cuda.current_stream().cuda_stream
        eng.backbone_forward(img, s)
        feat0 = eng.tensor_view("feat0", B)
        fl = model.keypoint_head.final_layer
        w, b = fl.weight.detach().reshape(17, -1).contiguous(), fl.bias.detach()
        dec = (4.0, 0.0, 4.0, 0.0)
        runs = {
            "backbone_forward": lambda: eng.backbone_forward(img, s),
            "head_argmax": lambda: capf.kp_head_forward(feat0, w, b, capf.KP_ARGMAX, 1.0, dec, A),
            "head_integral": lambda: capf.kp_head_forward(feat0, w, b, capf.KP_INTEGRAL, 2.0, dec, A),
        }
        if dtype == "fp32":
            g1, g2 = torch.randn(B, 17, 2, device="cuda"), torch.randn(B, 17, 2, device="cuda")
            dmap = torch.zeros_like(feat0)
            runs["head_backward_dW"] = lambda: capf.kp_head_backward(feat0, w, b, g1, g2, 2.0, dec, A)
            runs["head_backward_dW_dmap"] = lambda: capf.kp_head_backward(feat0, w, b, g1, g2, 2.0, dec, A, dmap=dmap)
        with torch.no_grad():
            runs["forward_given_keypoints"] = lambda: model(img, k2d, kc.clone())
            runs["forward_detect"] = lambda: model.forward_detect(img, A)
            row = {"config": spec, "feat0": list(feat0.shape), "feat0_MB": round(feat0.numel() * feat0.element_size() / 1e6, 2),
                   "one_read_floor_ms": round(feat0.numel() * feat0.element_size() / (args.hbm_gbs * 1e9) * 1e3, 4), "repeats": args.repeats}
            row.update(timed(runs, args.repeats, args.warmup))
        print(json.dumps(row), flush=True)
        for e in model._engines.values():
            e.close()
        model._engines.clear()


if __name__ == "__main__":
    main()
