"""What the occlusion costs (EXPERIMENTS.md R37.1): capf_erase_patches on batches of 256 x 192 crops with 17 patches of size 70 (the
skeleton at the reference function's defaults), next to capf_preprocess on the same batch in the same process.  bench_kp_head.py's method:
device events around every host call, the calls alternating, medians with min / max over the repeats.  The erase calls include the
binding's scratch allocation (a cached block after the first call); `in_place` writes over its input, which the paint kernel also reads.

    python tools/bench_erase.py [--batches 64 512] [--patches 17] [--size 70] [--repeats 20] [--warmup 3]      (needs the MI355X)
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "contextaware-poseformer_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[64, 512])
    ap.add_argument("--patches", type=int, default=17)
    ap.add_argument("--size", type=int, default=70)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_erase.py needs the MI355X"
    from bench_kp_head import timed
    from capf import lib as capf

    H, W, P = 256, 192, args.patches
    g = torch.Generator().manual_seed(1)
    for B in args.batches:
        images = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8).cuda()
        centres = (torch.rand(B, P, 2, generator=g) * torch.tensor([float(W), float(H)])).cuda()
        half = (torch.rand(B, P, generator=g) < 0.5).to(torch.uint8).cuda()
        gt, k2d = torch.randn(B, 1, 17, 3, generator=g).cuda(), (torch.rand(B, 17, 2, generator=g) * 2 - 1).cuda()
        kc = (torch.rand(B, 17, 2, generator=g) * torch.tensor([float(W), float(H)])).cuda()
        out, work = torch.empty_like(images), images.clone()
        runs = {
            "erase_mean": lambda: capf.erase_patches(images, centres, None, args.size, True, out=out),
            "erase_zero": lambda: capf.erase_patches(images, centres, None, args.size, False, out=out),
            "erase_mean_half_masked": lambda: capf.erase_patches(images, centres, half, args.size, True, out=out),
            "erase_mean_in_place": lambda: capf.erase_patches(work, centres, None, args.size, True, out=work),
            "preprocess_mode0": lambda: capf.preprocess(images, gt, k2d, kc, "hrnet_32", 0),
        }
        row = {"batch": B, "height": H, "width": W, "patches": P, "size": args.size, "repeats": args.repeats,
               "image_mbytes": round(images.numel() / 1e6, 2)}
        row.update(timed(runs, args.repeats, args.warmup))
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
