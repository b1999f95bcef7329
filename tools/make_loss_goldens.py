"""Writes tests/golden/losses_extra.npz: what the REFERENCE's KeypointsL2Loss, LimbLengthError and UNCERTAINTY (ContextPose/mvn/models/loss.py,
imported through oracle/_refshim.reference_losses(), torch on the CPU) return on tests/loss_extra_cases.golden_inputs(), and their own
autograd gradients where autograd is finite: L2 with validity all ones on poses that share no row, UNCERTAINTY on the same poses.  Numbers
only; the inputs are regenerated from seeds on both sides.

    python tools/make_loss_goldens.py            (needs the reference tree; writes the file)
    python tools/make_loss_goldens.py --check    (recomputes and compares with the file; exit status 1 on a difference)
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("contextaware-poseformer_amd", "oracle", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
PATH = os.path.join(ROOT, "tests", "golden", "losses_extra.npz")


def compute():
    import torch
    import _refshim
    import loss_extra_cases as lc
    ref = _refshim.reference_losses()
    pred, gt, validity, sigmas = lc.golden_inputs()
    t = torch.from_numpy
    out = {}
    with torch.no_grad():
        out["l2_loss"] = ref.KeypointsL2Loss()(t(pred), t(gt), t(validity)).numpy()
        out["limb_error"] = np.float64(ref.LimbLengthError()(t(pred), t(gt)))
        out["limb_error_numpy_arguments"] = np.float64(ref.LimbLengthError()(pred, gt))
        out["uncertainty_loss"] = ref.UNCERTAINTY([t(s) for s in sigmas], t(pred), t(gt)).numpy()
    # gradients: autograd is finite only where no square root sits at 0 -- no row shared between pred and gt, no masked row
    n = lc.GRAD_POSES
    assert not (pred[:n] == gt[:n]).all(-1).any(), "a row of pred equals its row of gt: the reference's gradient is NaN there"
    p = t(pred[:n]).clone().requires_grad_(True)
    loss = ref.KeypointsL2Loss()(p, t(gt[:n]), torch.ones(n, pred.shape[1], 1))
    loss.backward()
    out["l2_ones_loss"], out["l2_ones_dpred"] = loss.detach().numpy(), p.grad.numpy()
    p = t(pred[:n]).clone().requires_grad_(True)
    sg = [t(s[:n]).clone().requires_grad_(True) for s in sigmas]
    loss = ref.UNCERTAINTY(sg, p, t(gt[:n]))
    loss.backward()
    out["uncertainty_grad_loss"], out["uncertainty_dpred"] = loss.detach().numpy(), p.grad.numpy()
    for k, s in enumerate(sg):
        out[f"uncertainty_dsigma{k}"] = s.grad.numpy()
    assert all(np.isfinite(v).all() for v in out.values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    out = compute()
    if args.check:
        have = np.load(PATH, allow_pickle=False)
        bad = [k for k in out if k not in have.files or not np.array_equal(have[k], out[k])] + [k for k in have.files if k not in out]
        print("losses_extra.npz:", "differs in " + ", ".join(bad) if bad else f"{len(out)} arrays equal the reference's")
        sys.exit(1 if bad else 0)
    np.savez(PATH, **out)
    print(f"wrote {PATH}: {os.path.getsize(PATH)} bytes, {len(out)} arrays")


if __name__ == "__main__":
    main()
