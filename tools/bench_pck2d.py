"""What the 2-D PCKh metric costs (EXPERIMENTS.md R36.1): capf_pck2d_counts at an evaluation batch and at a whole test set, and
CA_PF.keypoint_loss with and without return_accuracy on the same engine (the second is the call as it was before the keyword existed, so
the difference is the overhead of the accuracy figure).  bench_kp_head.py's method: one process, device events around every host call,
the calls alternating, medians with min / max over the repeats.

    python tools/bench_pck2d.py [--sizes 512 100000] [--loss-config hrnet_32:fp32:64] [--repeats 20] [--warmup 3]      (needs the MI355X)
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "contextaware-poseformer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="+", type=int, default=[512, 100000])
    ap.add_argument("--loss-config", default="hrnet_32:fp32:64", help="backbone:dtype:batch of the keypoint_loss comparison")
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_pck2d.py needs the MI355X"
    from bench_kp_head import timed
    from capf import lib as capf
    from capf import synth
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config

    J, thresholds = 17, [25.6 * 0.1 * k for k in range(1, 11)]
    g = torch.Generator().manual_seed(1)
    runs = {}
    for n in args.sizes:
        gt = (torch.rand(n, J, 2, generator=g) * 256).cuda()
        pred = gt + torch.randn(n, J, 2, generator=g).cuda() * 12
        seg = torch.randint(0, 2, (n,), generator=g, dtype=torch.int32).cuda()
        runs[f"pck2d_counts_n{n}"] = lambda pred=pred, gt=gt: capf.pck2d_counts(pred, gt, thresholds)
        runs[f"pck2d_counts_n{n}_2_segments"] = lambda pred=pred, gt=gt, seg=seg: capf.pck2d_counts(pred, gt, thresholds, segment=seg, n_segments=2)
    row = {"joints": J, "thresholds": len(thresholds), "repeats": args.repeats}
    row.update(timed(runs, args.repeats, args.warmup))
    print(json.dumps(row), flush=True)

    backbone, dtype, B = args.loss_config.split(":")
    B = int(B)
    cfg = backbone_preset(copy.deepcopy(config), backbone)
    cfg.model.backbone.fix_weights = True
    model = CA_PF(cfg, compute_dtype=dtype, keypoint_head="argmax")
    synth.load_synthetic(model, seed=1, bn_mode="random")
    model = model.cuda().eval()
    img = synth.synth_inputs(B, 256, 256, seed=2, crop_range=(192, 256))[0].cuda()
    gt = (torch.rand(B, J, 2, generator=g) * 256).cuda()
    tw = torch.ones(B, J).cuda()
    fl = model.keypoint_head.final_layer

    def step(**kw):
        fl.weight.grad = fl.bias.grad = None
        out = model.keypoint_loss(img, gt, tw, **kw)
        (out[0] if isinstance(out, tuple) else out).backward()

    runs = {"keypoint_loss_step": step, "keypoint_loss_step_return_accuracy": lambda: step(return_accuracy=True)}
    row = {"config": args.loss_config, "repeats": args.repeats}
    row.update(timed(runs, args.repeats, args.warmup))
    row["overhead_ms"] = round(row["keypoint_loss_step_return_accuracy"]["median_ms"] - row["keypoint_loss_step"]["median_ms"], 4)
    print(json.dumps(row), flush=True)
    for e in model._engines.values():
        e.close()
    model._engines.clear()


if __name__ == "__main__":
    main()
