#!/usr/bin/env python
"""Two compute dtypes of the same build side by side on one GPU: speed, interleaved, and distance from the fp32 oracle.  (GPU box)

Both engines are built from the same synthetic checkpoint and run the same frames.  Speed: rounds of `--iters` forwards per dtype, the
dtypes alternating A B A B ... in one process, so that whatever else shares the host hits both alike; reported per dtype as the median
round and the spread of the rounds.  Then one profiled forward each (capf_forward_profile_launches), summed by kernel name: where a
difference sits.  Accuracy (--oracle-frames N): N frames spread over the batch through the fp32 CPU oracle, joints max-abs and mean
Euclidean distance per dtype (the vs_fp32_oracle figures of bench.py, for any dtype pair).

Usage: python tools/dtype_ab.py --backbone hrnet_48 --batch 256 [--dtypes bf16,fp16] [--rounds 7] [--iters 10] [--oracle-frames 8] [--json out.json]"""
import argparse
import contextlib
import copy
import io
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "contextaware-poseformer_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import torch
from capf import synth
from mvn.models.conpose import CA_PF
from mvn.utils.cfg import backbone_preset, config


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--backbone", default="hrnet_32")
    ap.add_argument("--dtypes", default="bf16,fp16")
    ap.add_argument("--height", type=int, default=256)
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--oracle-frames", type=int, default=0)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    dtypes = a.dtypes.split(",")
    cfg = backbone_preset(copy.deepcopy(config), a.backbone)
    cfg.model.backbone.fix_weights = True
    models, sd = {}, None
    for dt in dtypes:
        with contextlib.redirect_stdout(io.StringIO()):
            m = CA_PF(cfg, compute_dtype=dt).eval()
        sd = synth.load_synthetic(m, seed=1, bn_mode="random")
        models[dt] = m.cuda()
    img, k2d, kc = synth.synth_inputs(a.batch, a.height, a.width, seed=1000, crop_range=(a.width, a.height))
    img_d, k2d_d, kc_d = img.cuda(), k2d.cuda(), kc.cuda()
    outs = {}
    with torch.no_grad():
        for dt in dtypes:                                          # warm-up: code objects, workspace, weight packs
            for _ in range(3):
                outs[dt] = models[dt](img_d, k2d_d, kc_d.clone())
        torch.cuda.synchronize()
        rates = {dt: [] for dt in dtypes}
        kcs = [kc_d.clone() for _ in range(a.iters)]               # (the crop keypoints are normalised in place: fresh copies, made outside the window)
        for _ in range(a.rounds):
            for dt in dtypes:
                for k in kcs:
                    k.copy_(kc_d)
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for k in kcs:
                    models[dt](img_d, k2d_d, k)
                t1.record()
                torch.cuda.synchronize()
                rates[dt].append(a.batch * a.iters / (t0.elapsed_time(t1) * 1e-3))
    result = {"backbone": a.backbone, "batch": a.batch, "height": a.height, "width": a.width, "rounds": a.rounds, "iters": a.iters, "dtypes": {}}
    print(f"{a.backbone} batch {a.batch} {a.height}x{a.width}: {a.rounds} rounds of {a.iters} forwards per dtype, alternating")
    for dt in dtypes:
        r = sorted(rates[dt])
        result["dtypes"][dt] = {"frames_per_s_median": statistics.median(r), "frames_per_s_min": r[0], "frames_per_s_max": r[-1]}
        print(f"    {dt:5s} {statistics.median(r):10.1f} frames/s median   (rounds {r[0]:.1f} .. {r[-1]:.1f}, spread {100 * (r[-1] - r[0]) / statistics.median(r):.1f} %)")
    if len(dtypes) == 2:
        x, y = (result["dtypes"][dt]["frames_per_s_median"] for dt in dtypes)
        print(f"    {dtypes[1]} / {dtypes[0]} = {y / x:.4f}")
        result["ratio"] = y / x
    # where the time goes, by kernel: one profiled forward each (serialised launches: not the end-to-end time)
    stream = torch.cuda.current_stream().cuda_stream
    by_kernel = {}
    for dt in dtypes:
        eng = models[dt].engine_for(img_d)
        table = eng.op_table(a.batch)
        acc = None
        for _ in range(3):
            ms, leader = eng.forward_profile_launches(img_d, k2d_d, kc_d.clone(), outs[dt], stream)
            acc = ms if acc is None else [p + q for p, q in zip(acc, ms)]
        agg = {}
        for i, l in enumerate(leader):
            if l == i:
                name = table[i][1].replace("bf16", "16").replace("f16", "16")          # the same launch under either format
                agg[name] = agg.get(name, 0.0) + acc[i] / 3
        by_kernel[dt] = agg
    names = sorted(set().union(*[set(v) for v in by_kernel.values()]), key=lambda n: -max(v.get(n, 0.0) for v in by_kernel.values()))
    print("    per kernel family, ms per forward (launches profiled one by one):  " + "  ".join(f"{dt:>9s}" for dt in dtypes))
    for n in names[:14]:
        print(f"        {n:40s} " + "  ".join(f"{by_kernel[dt].get(n, 0.0):9.3f}" for dt in dtypes))
    print(f"        {'sum':40s} " + "  ".join(f"{sum(by_kernel[dt].values()):9.3f}" for dt in dtypes))
    result["kernel_ms"] = by_kernel
    if a.oracle_frames > 0:
        import capf_oracle as oracle
        pick = [round(i * (a.batch - 1) / max(1, a.oracle_frames - 1)) for i in range(a.oracle_frames)] if a.oracle_frames > 1 else [0]
        pick = sorted(set(pick))
        with torch.no_grad():
            want = oracle.ca_pf_forward(sd, img[pick], k2d[pick], kc[pick].clone(), backbone=a.backbone)
        print(f"    joints vs the fp32 CPU oracle on {len(pick)} frames of the batch (metres):")
        for dt in dtypes:
            d = outs[dt].cpu()[pick].reshape(-1, 17, 3) - want.reshape(-1, 17, 3)
            mx, mean = d.abs().max().item(), d.norm(dim=-1).mean().item()
            result["dtypes"][dt].update({"vs_fp32_oracle_max": mx, "vs_fp32_oracle_mean": mean})
            print(f"        {dt:5s} max-abs {mx:.3e}   mean distance {mean:.3e}")
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
