#!/usr/bin/env python
"""Micro-benchmark of the optimizer end of the training step at the real lifter size (HRNet-32, 256x192 plan: ~14.1 M fp32 elements).

Alternates, on one device in one process, the legacy update (capf_adamw_step: seven streams of 4 n bytes) with the guarded route
(capf_grad_sumsq + capf_adamw_step_guarded: one more read of the gradient and one more launch) in four settings: one group / the nine
segments of the sampling_offsets rule, without / with clipping engaged.  Each figure is the median over --pairs rounds of one HIP-event
interval around --calls back-to-back steps.  Prints one JSON line.

    python tools/bench_optim.py [--pairs 9] [--calls 20]
"""
import argparse
import copy
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "contextaware-poseformer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=9)
    ap.add_argument("--calls", type=int, default=20)
    a = ap.parse_args()
    assert a.pairs >= 7
    import torch
    from capf import Engine
    from capf.optim import FusedAdamW, param_groups
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), "hrnet_32")
    cfg.model.backbone.fix_weights = True
    eng = Engine(_native.make_capf_config(cfg, 256, 192), device=None)
    layout, n = eng.grad_layout()
    nine = param_groups(layout, [("sampling_offsets", 0.1)], total=n)
    eng.close()
    gen = torch.Generator(device="cuda").manual_seed(0)
    p0 = torch.randn(n, device="cuda", generator=gen) * 0.02
    g = torch.randn(n, device="cuda", generator=gen) * 1e-3
    norm = g.double().norm().item()
    variants = {
        "legacy": dict(),
        "guarded_1group": dict(skip_nonfinite=True),
        "guarded_9segments": dict(groups=nine),
        "guarded_1group_clipped": dict(max_grad_norm=0.5 * norm),
        "guarded_9segments_clipped": dict(groups=nine, max_grad_norm=0.5 * norm),
    }
    opts = {k: FusedAdamW(p0.clone(), lr=6.4e-4, weight_decay=0.1, **kw) for k, kw in variants.items()}
    for o in opts.values():                      # warm-up: module load, control blocks
        o.step(g)
    torch.cuda.synchronize()
    ms = {k: [] for k in opts}
    for _ in range(a.pairs):
        for k, o in opts.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                o.step(g)
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / a.calls)
    out = {"elements": n, "pairs": a.pairs, "calls": a.calls, "device": torch.cuda.get_device_name(0)}
    for k, v in ms.items():
        med = statistics.median(v)
        streams = 7 if k == "legacy" else 8
        out[k] = {"ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "GBps": round(streams * 4 * n / med / 1e6, 1)}
    for k in ms:
        if k != "legacy":
            out[k]["vs_legacy"] = round(out[k]["ms"] / out["legacy"]["ms"], 3)
    rep = opts["guarded_9segments_clipped"].report()
    out["clip_coef"] = rep["clip_coef"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
