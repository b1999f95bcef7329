"""What KeypointsL2Loss, LimbLengthError / limb_length_loss and UNCERTAINTY cost on the native path (EXPERIMENTS.md R39.1): each C entry
without gradients (dpred = NULL) and with every gradient written, at 64 x 17 and 512 x 17 rows, the limb kernels also at 5 x 10^5 poses
(an evaluation set) -- each next to the reference's expression run by torch on the same device in the same process, forward alone and
forward + backward.  The torch expression is the only other form there is: before these entries the library had none.
bench_kp_head.py's method: device events around every host call, the calls alternating, medians with min / max over the repeats.
LimbLengthError's reference form ends in sixteen `.cpu()` calls, so its time (and the native class's, which ends in one) is taken around
the whole host call with time.perf_counter.

    python tools/bench_losses.py [--batches 64 512] [--poses 500000] [--repeats 20] [--warmup 3]      (needs the MI355X)
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "contextaware-poseformer_amd"))


def wall(runs, repeats, warmup):
    import torch
    times = {k: [] for k in runs}
    for it in range(warmup + repeats):
        for name, run in runs.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            if it >= warmup:
                times[name].append((time.perf_counter() - t0) * 1e3)
    return {k: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)} for k, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="+", type=int, default=[64, 512])
    ap.add_argument("--poses", type=int, default=500000)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_losses.py needs the MI355X"
    from bench_kp_head import timed
    from capf import lib as capf
    from mvn.models.loss import CONNECTIVITY_DICT, LimbLengthError

    J, L = 17, len(CONNECTIVITY_DICT)
    g = torch.Generator().manual_seed(1)

    def torch_l2(p, t, v):                                         # loss.py:145-146
        loss = torch.sum(torch.sqrt(torch.sum((t - p) ** 2 * v, dim=2)))
        return loss / max(1, torch.sum(v).item())

    def torch_limb(p, t):                                          # loss.py:190-199 without the .cpu() per limb: the form a loss would take
        error = 0
        for a, b in CONNECTIVITY_DICT:
            error = error + torch.abs(torch.norm(p[:, a] - p[:, b], dim=1) - torch.norm(t[:, a] - t[:, b], dim=1)).mean()
        return error / L

    def torch_limb_reference(p, t):                                # loss.py:190-201 as it stands: sixteen .cpu() calls, a Python float
        error = 0
        for a, b in CONNECTIVITY_DICT:
            error += torch.abs(torch.norm(p[:, a] - p[:, b], dim=1) - torch.norm(t[:, a] - t[:, b], dim=1)).mean().cpu()
        return float(error) / L

    def torch_unc(sigmas, p, t):                                   # loss.py:8-13
        diff = p - t
        return sum(torch.mean(torch.norm(diff / (s + 1e-6), dim=2)) + 0.01 * torch.mean(torch.log(s + 1e-6)) for s in sigmas)

    def fwd_bwd(f, leaves):
        def run():
            for x in leaves:
                x.grad = None
            f().backward()
        return run

    for B in args.batches:
        gt = (0.3 * torch.randn(B, J, 3, generator=g)).cuda()
        pred = (gt + 0.05 * torch.randn(B, J, 3, generator=g).cuda())
        v = (torch.rand(B, J, 1, generator=g) > 0.2).float().cuda()
        ones = torch.ones(B, J, 1).cuda()
        sig = [(0.05 + 0.5 * torch.rand(B, J, w, generator=g)).cuda() for w in (3, 1)]
        lp = pred.clone().requires_grad_(True)
        ls = [s.clone().requires_grad_(True) for s in sig]
        runs = {
            "l2_native": lambda: capf.keypoints_l2_loss(pred, gt, v),
            "l2_native_grad": lambda: capf.keypoints_l2_loss(pred, gt, v, want_grad=True),
            "l2_torch": lambda: torch_l2(pred, gt, v),
            "l2_torch_grad": fwd_bwd(lambda: torch_l2(lp, gt, ones), [lp]),          # (all ones: with a masked row the gradient is NaN)
            "limb_native": lambda: capf.limb_length_sums(capf.limb_length_errors(pred, gt, CONNECTIVITY_DICT)[0]),
            "limb_native_grad": lambda: capf.limb_length_sums(capf.limb_length_errors(pred, gt, CONNECTIVITY_DICT, want_grad=True, grad_scale=1.0 / (B * L))[0]),
            "limb_torch": lambda: torch_limb(pred, gt),
            "limb_torch_grad": fwd_bwd(lambda: torch_limb(lp, gt), [lp]),
            "uncertainty_native": lambda: capf.uncertainty_loss(pred, gt, sig),
            "uncertainty_native_grad": lambda: capf.uncertainty_loss(pred, gt, sig, want_dpred=True, want_dsigma=[True, True]),
            "uncertainty_torch": lambda: torch_unc(sig, pred, gt),
            "uncertainty_torch_grad": fwd_bwd(lambda: torch_unc(ls, lp, gt), [lp] + ls),
        }
        row = {"rows": B * J, "repeats": args.repeats}
        row.update(timed(runs, args.repeats, args.warmup))
        print(json.dumps(row), flush=True)

    n = args.poses
    gt = (0.3 * torch.randn(n, J, 3, generator=g)).cuda()
    pred = gt + 0.05 * torch.randn(n, J, 3, generator=g).cuda()
    seg = torch.randint(0, 15, (n,), generator=g, dtype=torch.int32).cuda()
    err = capf.limb_length_errors(pred, gt, CONNECTIVITY_DICT)[0]
    runs = {
        "limb_errors": lambda: capf.limb_length_errors(pred, gt, CONNECTIVITY_DICT),
        "limb_errors_grad": lambda: capf.limb_length_errors(pred, gt, CONNECTIVITY_DICT, want_grad=True),
        "limb_sums": lambda: capf.limb_length_sums(err),
        "limb_sums_15_segments": lambda: capf.limb_length_sums(err, seg, n_segments=15),
        "limb_torch": lambda: torch_limb(pred, gt),
    }
    row = {"poses": n, "repeats": args.repeats}
    row.update(timed(runs, args.repeats, args.warmup))
    print(json.dumps(row), flush=True)
    native = LimbLengthError()
    row = {"poses": n, "repeats": args.repeats, "clock": "host, synchronised"}
    row.update(wall({"LimbLengthError_native": lambda: native(pred, gt), "LimbLengthError_torch_reference_form": lambda: torch_limb_reference(pred, gt)},
                    args.repeats, args.warmup))
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
