"""CPU: heatmap supervision of the 2-D keypoint head (capf_kp_heatmap_loss) -- the float64 oracle the GPU tests use against torch's float64
autograd and against hand-computed targets, every refusal the header lists (none needs a device: each returns before anything is
launched), the scratch size, the Python-level errors, and that the GPU tests' bound cannot hide a dropped pixel."""
import contextlib
import copy
import io
import math

import numpy as np
import pytest
import torch

import kp_heatmap_oracle as O
from capf import lib as capf

INVALID, UNSUPPORTED = -1, -2


def _problem(seed, B=3, J=5, H=7, W=6, C=8, sigma=1.0):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((B, H, W, C))
    wt = rng.standard_normal((J, C)) * 0.3
    bias = rng.standard_normal(J) * 0.1
    gt = np.stack([rng.uniform(-3, W + 3, (B, J)), rng.uniform(-3, H + 3, (B, J))], -1).astype(np.float32)
    tw = rng.choice([0.0, 0.5, 1.0, 1.0], (B, J)).astype(np.float32)
    return x, wt, bias, gt, tw


# ---- the oracle against autograd --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction,topk,scale", [(O.MEAN, 8, 0.5), (O.OHKM, 1, 0.5), (O.OHKM, 3, 1.0), (O.OHKM, 5, 0.5), (O.OHKM, 8, 0.5)])
def test_oracle_gradients_equal_float64_autograd(reduction, topk, scale):
    x, wt, bias, gt, tw = _problem(3)
    B, H, W, C = x.shape
    J = wt.shape[0]
    decode, sigma = (1.5, 0.25, 2.0, -0.5), 1.0
    X, Wt, Bs = (torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (x, wt, bias))
    z = torch.einsum("byxc,jc->bjyx", X, Wt) + Bs[None, :, None, None]
    t = torch.tensor(O.targets(gt, decode, sigma, H, W))
    w = torch.tensor(O.effective_weight(gt, tw, decode, sigma, H, W))
    lj = scale * ((z * w[..., None, None] - t * w[..., None, None]) ** 2).mean((2, 3))        # HRNet: prediction and target times w
    if reduction == O.MEAN:
        loss = lj.mean()
    else:
        loss = torch.stack([torch.topk(lj[b], min(topk, J)).values.sum() / topk for b in range(B)]).mean()
    loss.backward()
    got = O.evaluate(z.detach().numpy(), x, wt, gt, tw, decode, sigma, reduction, topk, scale)
    rel = lambda a, b: np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)
    assert rel(got["joint_loss"], lj.detach().numpy()) < 1e-12
    assert abs(got["loss"] - loss.item()) <= 1e-12 * abs(loss.item())
    assert rel(got["dweight"], Wt.grad.numpy()) < 1e-12
    assert rel(got["dbias"], Bs.grad.numpy()) < 1e-12
    assert rel(got["dmap"], X.grad.numpy()) < 1e-12
    assert got["sel"].sum(1).tolist() == [J if reduction == O.MEAN else min(topk, J)] * B


def test_oracle_ohkm_ties_go_to_the_smaller_index_and_nan_ranks_first():
    lj = np.array([[1.0, 3.0, 3.0, 0.5], [2.0, np.nan, 5.0, 5.0]])
    assert O.select(lj, O.OHKM, 1).tolist() == [[0, 1, 0, 0], [0, 1, 0, 0]]
    assert O.select(lj, O.OHKM, 2).tolist() == [[0, 1, 1, 0], [0, 1, 1, 0]]
    assert O.select(lj, O.OHKM, 7).tolist() == [[1, 1, 1, 1], [1, 1, 1, 1]]
    assert O.select(lj, O.MEAN, 1).tolist() == [[1, 1, 1, 1], [1, 1, 1, 1]]


# ---- hand-computable targets: sigma = 1, R = 3, a 5 x 3 map (H = 5 rows, W = 3 columns) ----------------------------------------------------
def test_hand_computed_targets():
    H, W, sigma = 5, 3, 1.0
    assert O.radius(sigma) == 3 and O.radius(2.0) == 6 and O.radius(0.4) == 2
    gt = np.array([[[0.0, 0.0], [1.5, 2.0], [-0.7, 4.0], [2.0, 4.0]]], np.float32)       # corner; x.5; -0.7; the far corner
    c, mu, ok = O.centres(gt, (1, 0, 1, 0))
    assert ok.all() and mu[0].tolist() == [[0, 0], [2, 2], [0, 4], [2, 4]]               # int(1.5 + 0.5) = 2; int(-0.2) = 0, not -1
    t = O.targets(gt, (1, 0, 1, 0), sigma, H, W)
    e = lambda d2: math.exp(-d2 / 2.0)
    assert np.allclose(t[0, 0], [[e(0), e(1), e(4)], [e(1), e(2), e(5)], [e(4), e(5), e(8)], [e(9), e(10), e(13)], [0, 0, 0]], rtol=1e-15, atol=0)
    assert t[0, 0, 4].tolist() == [0, 0, 0]                                              # row 4 is outside the corner's window (|dy| = 4 > R)
    assert np.allclose(t[0, 1, 2], [e(4), e(1), e(0)], rtol=1e-15) and np.allclose(t[0, 1, 0], [e(8), e(5), e(4)], rtol=1e-15)
    assert np.allclose(t[0, 2, 4], [e(0), e(1), e(4)], rtol=1e-15) and t[0, 2, 0].tolist() == [0, 0, 0]
    assert np.allclose(t[0, 3, 4], [e(4), e(1), e(0)], rtol=1e-15)
    # the decode: heatmap cell = (k - o) / s
    _, mu, _ = O.centres(np.array([[[9.0, 10.0]]], np.float32), (4.0, 1.0, 2.0, 0.0))
    assert mu[0, 0].tolist() == [2, 5]


def test_weight_zeroing_rules():
    H, W, sigma = 5, 3, 1.0                                                              # R = 3
    gt = np.array([[[1.0, 2.0], [5.4, 2.0], [5.6, 2.0], [-3.4, 2.0], [-3.6, 2.0], [1.0, 7.6], [1.0, -3.6], [np.nan, 1.0], [1.0, np.inf],
                    [2.0 ** 21, 1.0], [1.0, 2.0]]], np.float32)
    tw = np.array([[1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0.5]], np.float32)
    w = O.effective_weight(gt, tw, (1, 0, 1, 0), sigma, H, W)
    # mu_x = 5: 5 - 3 = 2 < W stays; mu_x = 6: 6 - 3 >= W goes; mu_x = -3: -3 + 3 = 0 stays; mu_x = int(-3.1) = -3 ... -3.6 + .5 -> -3 stays
    assert w[0].tolist() == [1, 1, 0, 1, 1, 0, 1, 0, 0, 0, 0.5]
    gt2 = np.array([[[-4.6, 2.0], [1.0, -4.6]]], np.float32)                             # int(-4.1) = -4: -4 + 3 < 0
    assert O.effective_weight(gt2, None, (1, 0, 1, 0), sigma, H, W)[0].tolist() == [0, 0]
    assert O.effective_weight(gt[:, :1], None, (1, 0, 1, 0), sigma, H, W)[0].tolist() == [1]


# ---- the bound of the GPU tests cannot hide a dropped pixel ----------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (5, 3), (16, 16), (17, 16), (24, 22), (64, 64)])
def test_bound_is_below_the_effect_of_any_dropped_window_pixel(H, W):
    """On logits that differ from the target by 1/2 everywhere (so that every pixel's term is known: 1/4), deleting ANY single in-window pixel
    of an item moves joint_loss, the loss, dbias and the item's dweight row by more than (d + 8) 2^-24 sum|terms| -- the bound the GPU tests
    hold the kernel to is finer than one pixel."""
    B, J, C, sigma = 1, 2, 4, 1.0
    gt = np.array([[[W / 2.0, H / 2.0], [0.0, 0.0]]], np.float32)
    decode = (1, 0, 1, 0)
    t = O.targets(gt, decode, sigma, H, W)
    sign = np.where((np.arange(H)[:, None] + np.arange(W)[None, :]) % 2 == 0, 0.5, -0.5)
    z = t + sign
    x = np.ones((B, H, W, C))
    full = O.evaluate(z, x, None, gt, None, decode, sigma)
    win = O.window(gt, decode, sigma, H, W)
    assert win[0, 0].sum() >= 1
    for y, xx in zip(*np.nonzero(win[0, 0])):
        cut = O.evaluate(z, x, None, gt, None, decode, sigma, drop=(0, 0, y, xx))
        for name, at in (("joint_loss", (0, 0)), ("loss", ()), ("dbias", (0,)), ("dweight", (0,))):      # item (0, 0)'s entries
            a, b = np.asarray(full[name])[at], np.asarray(cut[name])[at]
            limit = np.asarray(O.bound(name, full["mass"][name], B, H, W, J))[at]
            assert np.all(np.abs(a - b) > limit), (name, y, xx, float(np.max(np.abs(a - b))), float(np.max(limit)))


# ---- every refusal of the header, through the library built in-tree --------------------------------------------------------------------
P = 0x10000        # a well-aligned non-NULL "pointer": every call below is refused before anything could read it


def _args(**kw):
    a = dict(stream=None, map=P, dtype=capf.F32, weight=P, bias=P, B=2, H=8, W=8, C=32, J=17, gt=P, tw=None,
             decode=(capf.c_float * 4)(1, 0, 1, 0), sigma=2.0, reduction=0, topk=8, scale=0.5, loss=P, joint_loss=None, dw=None, db=None,
             dmap=None, accumulate=0, scratch=P, nbytes=1 << 30)
    a.update(kw)
    return list(a.values())


_dec = lambda *v: (capf.c_float * 4)(*v)
REFUSALS = [
    ("NULL map", dict(map=None), INVALID), ("NULL weight", dict(weight=None), INVALID), ("NULL kcrop_gt", dict(gt=None), INVALID),
    ("NULL decode", dict(decode=None), INVALID), ("NULL loss", dict(loss=None), INVALID), ("NULL scratch", dict(scratch=None), INVALID),
    ("B = 0", dict(B=0), INVALID), ("H = 0", dict(H=0), INVALID), ("W = -1", dict(W=-1), INVALID),
    ("J = 0", dict(J=0), INVALID), ("J = 33", dict(J=33), INVALID),
    ("C = 30", dict(C=30), INVALID), ("C = 0", dict(C=0), INVALID), ("C = 516", dict(C=516), INVALID),
    ("sx = 0", dict(decode=_dec(0, 0, 1, 0)), INVALID), ("sy = 0", dict(decode=_dec(1, 0, 0, 0)), INVALID),
    ("sx = inf", dict(decode=_dec(float("inf"), 0, 1, 0)), INVALID), ("sy = NaN", dict(decode=_dec(1, 0, float("nan"), 0)), INVALID),
    ("sigma = 0", dict(sigma=0.0), INVALID), ("sigma < 0", dict(sigma=-1.0), INVALID), ("sigma = inf", dict(sigma=float("inf")), INVALID),
    ("sigma = NaN", dict(sigma=float("nan")), INVALID), ("R = 65", dict(sigma=21.5), INVALID),
    ("reduction 2", dict(reduction=2), INVALID), ("reduction -1", dict(reduction=-1), INVALID),
    ("dtype 3", dict(dtype=3), INVALID), ("dtype -1", dict(dtype=-1), INVALID),
    ("topk = 0", dict(topk=0), INVALID), ("topk < 0", dict(topk=-3), INVALID),
    ("scale = inf", dict(scale=float("inf")), INVALID), ("scale = NaN", dict(scale=float("nan")), INVALID),
    ("accumulate 2", dict(accumulate=2), INVALID), ("accumulate -1", dict(accumulate=-1), INVALID),
    ("misaligned map", dict(map=P + 4), INVALID), ("misaligned 16-bit map", dict(map=P + 4, dtype=capf.BF16), INVALID),
    ("misaligned dmap", dict(dmap=P + 4), INVALID),
    ("scratch too small", dict(nbytes=16), INVALID),
    ("dmap of a bf16 map", dict(dmap=P, dtype=capf.BF16), UNSUPPORTED), ("dmap of an fp16 map", dict(dmap=P, dtype=capf.F16), UNSUPPORTED),
]


@pytest.mark.parametrize("why,kw,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_need_no_device(why, kw, code):
    assert capf.load_library().capf_kp_heatmap_loss(*_args(**kw)) == code, why


def test_scratch_one_byte_short_and_the_first_radius_refused():
    lib = capf.load_library()
    for red in (0, 1):
        need = lib.capf_kp_heatmap_loss_scratch_bytes(2, 8, 8, 32, 17, red)
        assert lib.capf_kp_heatmap_loss(*_args(reduction=red, nbytes=need - 1)) == INVALID
    assert O.radius(21.3) == 64 and O.radius(21.4) == 65
    assert lib.capf_kp_heatmap_loss(*_args(sigma=21.4)) == INVALID               # R = ceil(64.2) = 65


def test_scratch_bytes():
    lib = capf.load_library()
    size = lib.capf_kp_heatmap_loss_scratch_bytes
    for bad in ((0, 8, 8, 32, 17), (2, 0, 8, 32, 17), (2, 8, 0, 32, 17), (2, 8, 8, 30, 17), (2, 8, 8, 516, 17), (2, 8, 8, 0, 17),
                (2, 8, 8, 32, 0), (2, 8, 8, 32, 33)):
        assert size(*bad, 0) == 0 and size(*bad, 1) == 0, bad                  # the shapes the head refuses
        assert lib.capf_kp_head_scratch_bytes(*bad, 0) == 0
    assert size(2, 8, 8, 32, 17, 2) == 0 and size(2, 8, 8, 32, 17, -1) == 0
    for red in (0, 1):
        sizes = [size(B, 64, 64, 32, 17, red) for B in (1, 2, 3, 7, 64, 65, 512)]
        assert all(a < b for a, b in zip(sizes, sizes[1:])) and sizes[0] > 0     # monotone in B
    assert size(4, 64, 64, 32, 17, 1) > size(4, 64, 64, 32, 17, 0)
    assert size(6, 24, 22, 48, 17, 0) == 3 * size(2, 24, 22, 48, 17, 0)          # the tiling is a function of H * W alone


def test_entries_are_declared_bound_and_documented():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lib = capf.load_library()
    for s in ("capf_kp_heatmap_loss_scratch_bytes", "capf_kp_heatmap_loss"):
        assert hasattr(lib, s) and s in capf.PROTOTYPES
        assert f"`{s}`" in open(os.path.join(root, "INTEGRATION.md")).read()
    assert (capf.KP_LOSS_MEAN, capf.KP_LOSS_OHKM) == (0, 1)
    header = open(os.path.join(root, "include", "capf.h")).read()
    for word in ("ties going to the smaller joint index", "a NaN ranking", "truncated toward zero", "wholly outside"):
        assert word in header, word


# ---- Python-level errors ------------------------------------------------------------------------------------------------------------------
def _model(backbone="hrnet_32", **kw):
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    with contextlib.redirect_stdout(io.StringIO()):
        return CA_PF(backbone_preset(copy.deepcopy(config), backbone), **kw)


def test_python_level_errors():
    from mvn.models.conpose import keypoint_heatmap_loss
    img, gt = torch.zeros(1, 64, 64, 3), torch.zeros(1, 17, 2)
    with pytest.raises(capf.CapfError, match="this model has no keypoint head"):
        _model().keypoint_loss(img, gt)
    with pytest.raises(NotImplementedError, match="frozen backbone"):
        _model("cpn", keypoint_head="cpn").keypoint_loss(img, gt)
    m = _model(keypoint_head="argmax")
    for bad in ("sum", "OHKM", None, 1):
        with pytest.raises(ValueError, match="reduction must be 'mean' or 'ohkm'"):
            m.keypoint_loss(img, gt, reduction=bad)
        with pytest.raises(ValueError, match="reduction must be 'mean' or 'ohkm'"):
            keypoint_heatmap_loss(torch.zeros(1, 4, 4, 8), torch.zeros(17, 8), None, gt, reduction=bad)
    with pytest.raises(ValueError, match="reduction must be 'mean' or 'ohkm'"):
        capf.kp_heatmap_loss(torch.zeros(1, 4, 4, 8), torch.zeros(17, 8), None, gt, reduction="sum")
    with pytest.raises(capf.CapfError):                                              # no CPU fallback
        m.keypoint_loss(img, gt)


def test_mpi_variant_forwards_the_method():
    from model.conpose import VolumetricTriangulationNet
    from mvn.models.conpose import CA_PF
    assert VolumetricTriangulationNet.keypoint_loss is not CA_PF.keypoint_loss and "keypoint_loss" in vars(VolumetricTriangulationNet)
