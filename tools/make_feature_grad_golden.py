"""Generate tests/golden/feature_grads.npz: the gradient of the loss w.r.t. the four context maps, from the REAL reference lifter.

Run in the build container only (the reference is imported read-only through oracle/_refshim.py, as oracle/make_goldens.py does):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_feature_grad_golden.py

The reference's PoseTransformer (pose_dformer.py:144-241) gets a seeded synthetic state (capf.synth), is cast to float64 and run in eval
mode (DropPath is the identity) as volume_net(k2d, ref, feats) on seeded maps that require grad (tests/feature_cases.py), followed by
MPJPE (loss.py:16-22) and backward -- autograd through the two F.grid_sample sites (pose_dformer.py:128, 217), which is what a
trainable backbone receives (conpose.py:22-25 with fix_weights = False).  Stored: dfeat0..3 (NCHW, float64) and the loss; arrays only,
inputs and weights are regenerated from seeds.  float64 because tests/test_features_api.py holds the oracle to 1e-9 of these values."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in ("oracle", "contextaware-poseformer_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
sys.dont_write_bytecode = True

import numpy as np
import torch


def main():
    import _refshim
    from capf import synth
    from feature_cases import GOLDEN, golden_inputs

    torch.set_num_threads(8)
    model, _ = _refshim.build_reference(GOLDEN["backbone"])
    synth.load_synthetic(model, seed=GOLDEN["wseed"], bn_mode="random")
    vn = model.volume_net.double().eval()
    maps, k2d, ref, gt = golden_inputs()
    feats = [m.double().requires_grad_(True) for m in maps]
    pred = vn(k2d.double(), ref.double(), feats)
    loss = _refshim.reference_losses().MPJPE()(pred, gt.double())
    loss.backward()
    rec = {"loss": np.array(loss.item(), np.float64), "pred": pred.detach().numpy()}
    for l, f in enumerate(feats):
        assert f.grad is not None and f.grad.dtype == torch.float64 and f.grad.abs().max() > 0
        rec[f"dfeat{l}"] = f.grad.numpy()
    out = os.path.join(ROOT, "tests", "golden", "feature_grads.npz")
    np.savez_compressed(out, **rec)
    print(f"wrote {out}: {os.path.getsize(out)} bytes, loss {loss.item():.12f}, "
          + ", ".join(f"|dfeat{l}| {f.grad.norm().item():.3e}" for l, f in enumerate(feats)))


if __name__ == "__main__":
    main()
