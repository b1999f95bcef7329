"""GPU: CA_PF.keypoint_loss(return_accuracy=True) -- the loss and final_layer's gradients are the default call's bit for bit, and acc
EQUALS the restatement of capf_pck2d_counts (pck2d_oracle.py: norm = (W / 10, H / 10) of the crop as fp32, strict `<`, threshold 0.5,
weight = target_weight; the mean over the joints with a valid sample of counts / valid) applied to detect()'s keypoints on the same images.
HRNet-32 at a 64 x 64 crop (feat0 16 x 16), argmax and integral heads, fp32 and bf16, and one 32 x 64 crop, where exchanging the two norm
entries changes the figure.

Why `==` and no tolerance: the batch is 8 and the target weights leave every joint 0, 1, 2, 4 or 8 valid samples, so every rate is a
multiple of 1 / 8 no larger than 1, the sum of at most 17 of them is exact in float64 in ANY order, and the one division by the number
of joints is the same correctly rounded operation on the device and in numpy."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import pck2d_oracle as O
from capf import synth

pytestmark = pytest.mark.gpu
J, B = 17, 8


def _model(head, dtype="fp32", wseed=3):
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), "hrnet_32")
    cfg.model.backbone.fix_weights = True
    with contextlib.redirect_stdout(io.StringIO()):
        m = CA_PF(cfg, compute_dtype=dtype, keypoint_head=head).eval()
    synth.load_synthetic(m, seed=wseed, bn_mode="random")
    return m


def _release(*models):
    for m in models:
        for e in m._engines.values():
            e.close()
        m._engines.clear()


def _ground_truth(kcrop, seed=5):
    """detect()'s keypoints plus offsets (1, 0), (0, 5), (2, 2), (3, 0) pixels -- at a 64-pixel side (radius 3.2 pixels at threshold 0.5)
    a hit, a miss, a hit, a hit; at 32 rows x 64 columns (3.2 pixels in x, 1.6 in y) a hit, a miss, a miss, a hit, and (3, 0) a MISS
    were the two norm entries exchanged -- and a target_weight with zeros: joint j keeps 8, 4, 2, 1 samples (j % 4), joint 6 none"""
    rng = np.random.RandomState(seed)
    offs = np.array([(1, 0), (0, 5), (2, 2), (3, 0)], np.float32)
    gt = (kcrop + offs[(np.arange(B)[:, None] + np.arange(J)[None]) % 4]).astype(np.float32)
    tw = np.zeros((B, J), np.float32)
    for j in range(J):
        keep = 0 if j == 6 else (8, 4, 2, 1)[j % 4]
        tw[rng.permutation(B)[:keep], j] = rng.choice([1.0, 0.5], keep)
    return gt, tw


def _reference(kcrop, gt, tw, H, W, swapped=False):
    nx, ny = (H / 10.0, W / 10.0) if swapped else (W / 10.0, H / 10.0)
    norm = np.tile(np.array([nx, ny], np.float32), (B, 1))
    counts, valid = O.pck2d_counts(kcrop, gt, [0.5], norm=norm, weight=tw, strict=True)[:2]
    assert all(int(v) in (0, 1, 2, 4, 8) for v in valid[0])                    # what makes the mean exact in any order (module docstring)
    return O.accuracy(counts, valid), counts, valid


CASES = [("argmax", "fp32", 64, 64), ("integral", "fp32", 64, 64), ("argmax", "bf16", 64, 64), ("integral", "bf16", 64, 64), ("argmax", "fp32", 32, 64)]


@pytest.mark.parametrize("head,dtype,H,W", CASES, ids=[f"{h}-{d}-{a}x{b}" for h, d, a, b in CASES])
def test_accuracy_is_the_restatement_on_detect_s_keypoints_and_changes_no_bit_of_the_loss(head, dtype, H, W):
    m = _model(head, dtype).cuda()
    try:
        images = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(9)).cuda()
        with torch.no_grad():
            kcrop = m.detect(images)[0].cpu().numpy()
        gt, tw = _ground_truth(kcrop)
        want, counts, valid = _reference(kcrop, gt, tw, H, W)
        assert 0.0 < want < 1.0 and valid[0, 6] == 0 and (valid[0] > 0).sum() == J - 1          # the restatement alone: strictly inside (0, 1)
        if H != W:
            assert _reference(kcrop, gt, tw, H, W, swapped=True)[0] != want                     # (nx, ny) exchanged would show here
        gt_d, tw_d = torch.from_numpy(gt).cuda(), torch.from_numpy(tw).cuda()
        fl = m.keypoint_head.final_layer
        bits = lambda t: t.detach().contiguous().view(-1).view(torch.int32).clone()
        sigma = 1.0 if min(H, W) < 64 else 2.0

        plain = m.keypoint_loss(images, gt_d, tw_d, sigma=sigma)                              # the default: the loss alone, as before
        assert torch.is_tensor(plain) and plain.dim() == 0 and plain.requires_grad
        plain.backward()
        ref_bits = bits(plain), bits(fl.weight.grad), bits(fl.bias.grad)
        fl.weight.grad = fl.bias.grad = None

        out = m.keypoint_loss(images, gt_d, tw_d, sigma=sigma, return_accuracy=True)
        assert isinstance(out, tuple) and len(out) == 2
        loss, acc = out
        assert acc.dim() == 0 and acc.is_cuda and acc.dtype == torch.float64 and not acc.requires_grad and acc.grad_fn is None
        loss.backward()
        assert torch.equal(bits(loss), ref_bits[0]) and torch.equal(bits(fl.weight.grad), ref_bits[1]) and torch.equal(bits(fl.bias.grad), ref_bits[2])
        assert fl.weight.grad.abs().max() > 0
        print(f"{head} {dtype} {H}x{W}: acc {acc.item():.17g}, restatement {want:.17g}")
        assert acc.item() == want

        with torch.no_grad():                                                                  # without grad: the same two values
            loss2, acc2 = m.keypoint_loss(images, gt_d, tw_d, sigma=sigma, return_accuracy=True)
        assert torch.equal(bits(loss2), ref_bits[0]) and acc2.item() == want and not loss2.requires_grad
        # no target_weight: every joint counts, 8 samples each
        acc3 = m.keypoint_loss(images, gt_d, sigma=sigma, return_accuracy=True)[1].item()
        want3, _, v3 = _reference(kcrop, gt, None, H, W)
        assert (v3 == B).all() and 0.0 < want3 < 1.0 and acc3 == want3
    finally:
        _release(m)


def test_mpi_variant_forwards_the_keyword_and_no_valid_joint_gives_nan():
    from model.conpose import VolumetricTriangulationNet, mpi_preset
    from mvn.utils.cfg import config
    H = W = 64
    with contextlib.redirect_stdout(io.StringIO()):
        m = VolumetricTriangulationNet(mpi_preset(copy.deepcopy(config), "hrnet_32"), keypoint_head="argmax").eval()
    synth.load_synthetic(m, seed=3, bn_mode="random")
    m = m.cuda()
    try:
        images = torch.randn(B, H, W, 3, generator=torch.Generator().manual_seed(9)).cuda()
        with torch.no_grad():
            kcrop = m.detect(images)[0].cpu().numpy()
        gt, tw = _ground_truth(kcrop)
        want = _reference(kcrop, gt, tw, H, W)[0]
        assert 0.0 < want < 1.0
        loss = m.keypoint_loss(images, torch.from_numpy(gt).cuda(), torch.from_numpy(tw).cuda())
        assert torch.is_tensor(loss) and loss.dim() == 0
        loss_a, acc = m.keypoint_loss(images, torch.from_numpy(gt).cuda(), torch.from_numpy(tw).cuda(), return_accuracy=True)
        assert torch.equal(loss_a.detach().view(1).view(torch.int32), loss.detach().view(1).view(torch.int32))
        assert acc.item() == want and not acc.requires_grad
        nothing = m.keypoint_loss(images, torch.from_numpy(gt).cuda(), torch.zeros(B, J).cuda(), return_accuracy=True)[1]
        assert torch.isnan(nothing).item()
    finally:
        _release(m)
