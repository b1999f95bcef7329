"""GPU: capf_kp_heatmap_loss against tests/kp_heatmap_oracle.py (float64) evaluated on the library's OWN logits (capf_kp_head_forward's `heat`,
which the entry reproduces bit for bit), so that only the rounding of z - t, the loss arithmetic and the documented summation orders remain:
every output within (d + 8) 2^-24 of its sum of absolute terms, d the depth of the summation order at that shape
(tests/test_kp_heatmap_loss.py shows on the CPU that this bound is finer than one dropped pixel).  Plus both reductions with exact ties,
determinism across scratch buffers, batch sizes and positions, 16-bit maps, accumulate, all-NULL gradients, NaN, and scratch hygiene."""
import numpy as np
import pytest
import torch

import kp_heatmap_oracle as O
from capf import lib as capf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
OUTPUTS = ("loss", "joint_loss", "dweight", "dbias", "dmap")
_CACHE = {}


def _points(rng, B, J, H, W, R, sx, sy, first=0):
    """ground truth in crop pixels (cell * s): a point inside, mu on each border, windows partly and wholly outside on each side, a .5 and a
    negative coordinate, one NaN -- spread over the (frame, joint) items, the rest random around the map; with fewer items than special points the
    items take consecutive ones from `first` on, so that the small cases between them see them all"""
    special = [(W / 2.0, H / 2.0), (0.0, H / 2.0), (W - 1.0, H / 2.0), (W / 2.0, 0.0), (W / 2.0, H - 1.0),          # inside, the four borders
               (-R + 1.0, 1.0), (W + R - 2.0, H - 1.0), (1.0, -R + 1.0), (1.0, H + R - 2.0),                          # partly outside
               (W + R + 0.0, 1.0), (-R - 2.0, 1.0), (1.0, H + R + 0.0), (1.0, -R - 2.0),                              # wholly outside, each side (int(-R - 1.5) = -R - 1)
               (W / 2 + 0.5, H / 2 + 0.5), (-0.7, 0.3), (float("nan"), 1.0)]
    gt = np.stack([rng.uniform(-R, W + R, (B, J)), rng.uniform(-R, H + R, (B, J))], -1)
    flat = gt.reshape(-1, 2)
    if len(flat) >= len(special):
        for i, p in enumerate(special):
            flat[(i * 7) % len(flat)] = p
    else:
        for i in range(len(flat)):
            flat[i] = special[(first + i) % len(special)]
    return (flat.reshape(B, J, 2) * np.array([sx, sy])).astype(np.float32)


def _case(B, J, C, H, W, sigma=1.0, seed=0, dtype=torch.float32, decode=(4.0, 0.0, 4.0, 0.0)):
    """a problem on the device and, once per problem, the library's own logits of it"""
    key = (B, J, C, H, W, sigma, seed, dtype, decode)
    if key not in _CACHE:
        rng = np.random.default_rng(1000 * seed + 7 * H + W + 31 * J + C + B)
        x = torch.tensor(rng.standard_normal((B, H, W, C)), dtype=torch.float32).to(dtype)
        wt = torch.tensor(rng.standard_normal((J, C)) * (0.6 / np.sqrt(C)), dtype=torch.float32)
        bias = torch.tensor(rng.standard_normal(J) * 0.2, dtype=torch.float32)
        gt = _points(rng, B, J, H, W, O.radius(sigma), decode[0], decode[2], first=3 * (C // 16) + 5 * (H % 5) + B)
        tw = rng.choice([1.0, 1.0, 1.0, 0.5, 0.0], (B, J)).astype(np.float32)
        tw.reshape(-1)[:2] = (0.5, 0.0) if B * J >= 2 else 1.0
        d = dict(x=x.to(DEV), wt=wt.to(DEV), bias=bias.to(DEV), gt=torch.tensor(gt).to(DEV), tw=torch.tensor(tw).to(DEV),
                 x64=x.to(torch.float64).numpy(), wt64=wt.to(torch.float64).numpy(), gt_np=gt, tw_np=tw, decode=decode, sigma=sigma)
        d["heat"] = capf.kp_head_forward(d["x"], d["wt"], d["bias"], want_heat=True)[3].cpu().numpy()
        _CACHE[key] = d
    return _CACHE[key]


def _run(d, reduction="mean", topk=8, scale=0.5, tw=True, want_dmap=True, **kw):
    out = capf.kp_heatmap_loss(d["x"], d["wt"], d["bias"], d["gt"], d["tw"] if tw else None, d["decode"], d["sigma"], reduction, topk, scale,
                               want_dmap=want_dmap and d["x"].dtype == torch.float32, **kw)
    torch.cuda.synchronize()
    return dict(zip(OUTPUTS, out))


def _check(d, got, reduction, topk, scale=0.5, tw=True, names=OUTPUTS):
    B, J, H, W = d["heat"].shape
    red = O.MEAN if reduction == "mean" else O.OHKM
    want = O.evaluate(d["heat"], d["x64"], d["wt64"], d["gt_np"], d["tw_np"] if tw else None, d["decode"], d["sigma"], red, topk, scale)
    for name in names:
        if got[name] is None:
            continue
        g = got[name].cpu().to(torch.float64).numpy().reshape(np.shape(want[name]))
        limit = O.bound(name, want["mass"][name], B, H, W, J)
        err = np.abs(g - want[name])
        worst = float(np.max(err / np.maximum(limit, 1e-300)))
        print(f"{name}: max |got - want| / bound = {worst:.3f}")
        assert np.all(err <= limit), (name, worst)
    return want


def _raw(d, reduction, fill, band=0):
    """the entry through the C ABI on an exact-size scratch of the caller's, pre-filled with `fill`, between `band` floats of NaN on either
    side: (outputs, scratch, the whole buffer)"""
    red = capf.KP_LOSS_REDUCTIONS[reduction]
    B, H, W, C = d["x"].shape
    J = d["wt"].shape[0]
    nbytes = capf.load_library().capf_kp_heatmap_loss_scratch_bytes(B, H, W, C, J, red)
    assert nbytes > 0 and nbytes % 4 == 0
    buf = torch.full((2 * band + nbytes // 4,), float("nan"), device=DEV)
    scratch = buf[band:band + nbytes // 4]
    scratch.fill_(fill)
    f32 = dict(dtype=torch.float32, device=DEV)
    out = (torch.empty(1, **f32), torch.empty(B, J, **f32), torch.empty(J, C, **f32), torch.empty(J, **f32), torch.empty(B, H, W, C, **f32))
    p = capf._p
    capf._call("capf_kp_heatmap_loss", capf._stream(d["x"]), p(d["x"]), capf.F32, p(d["wt"]), p(d["bias"]), B, H, W, C, J, p(d["gt"]), p(d["tw"]),
               capf._kp_decode(d["decode"]), d["sigma"], red, 8, 0.5, *(p(t) for t in out), 0, p(scratch), nbytes)
    torch.cuda.synchronize()
    return dict(zip(OUTPUTS, out)), scratch, buf


SHAPES = [(1, 1), (5, 3), (16, 16), (17, 16), (24, 22)]
COMBOS = [(b, j, c) for b in (1, 3) for j in (1, 17, 32) for c in (4, 32, 48)]


@pytest.mark.parametrize("H,W", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
@pytest.mark.parametrize("B,J,C", COMBOS, ids=[f"B{b}-J{j}-C{c}" for b, j, c in COMBOS])
def test_mean_against_the_oracle_on_the_library_s_logits(B, J, C, H, W):
    d = _case(B, J, C, H, W)
    want = _check(d, _run(d), "mean", 8)
    # the items whose window lies wholly outside the map, or whose ground truth is NaN, contribute exactly 0
    got = _run(d)
    assert torch.equal(got["joint_loss"].cpu()[torch.tensor(want["w"] == 0)], torch.zeros(int((want["w"] == 0).sum())))


def test_the_head_s_own_size():
    d = _case(2, 17, 32, 64, 64, sigma=2.0)
    _check(d, _run(d), "mean", 8)
    _check(d, _run(d, "ohkm", 8), "ohkm", 8)
    _check(d, _run(d, scale=1.0, tw=False), "mean", 8, scale=1.0, tw=False)


def test_zero_weight_items_contribute_exactly_nothing():
    """every item's window wholly outside (one side each), NaN, or target_weight 0: all outputs are exact zeros"""
    d = dict(_case(1, 17, 32, 17, 16))
    H, W, R = 17, 16, O.radius(1.0)
    outside = [(W + R + 0.0, 1.0), (-R - 2.0, 1.0), (1.0, H + R + 0.0), (1.0, -R - 2.0), (float("nan"), 1.0), (1.0, float("inf")), (2.0 ** 22, 1.0)]
    gt = np.array([[outside[j % len(outside)] for j in range(17)]], np.float32) * 4.0
    gt[0, 7:10] = (8.0, 8.0)                                                             # inside, but target_weight 0
    tw = np.ones((1, 17), np.float32)
    tw[0, 7:10] = 0.0
    d["gt"], d["tw"], d["gt_np"], d["tw_np"] = torch.tensor(gt).to(DEV), torch.tensor(tw).to(DEV), gt, tw
    assert (O.effective_weight(gt, tw, d["decode"], 1.0, H, W) == 0).all()
    for reduction in ("mean", "ohkm"):
        got = _run(d, reduction, 8)
        for name in OUTPUTS:
            assert not got[name].cpu().to(torch.float64).abs().max().item(), name


# ---- OHKM -------------------------------------------------------------------------------------------------------------------------------
OHKM_SEEDS = {1: 4, 8: 4, 17: 4, 20: 4}      # topk -> seed, chosen on the CPU so that the k-th and (k + 1)-th l_bj of every frame are 1e-3 apart


def _ohkm_gap(lj, topk):
    """the smallest relative gap between the k-th and (k + 1)-th largest l_bj over the frames (inf where topk takes every joint)"""
    gap = np.inf
    for row in lj:
        s = np.sort(row)[::-1]
        if topk < len(s):
            gap = min(gap, (s[topk - 1] - s[topk]) / max(s[topk - 1], 1e-300))
    return gap


@pytest.mark.parametrize("topk", [1, 8, 17, 20])
def test_ohkm_against_the_oracle(topk):
    d = dict(_case(3, 17, 32, 24, 22, seed=OHKM_SEEDS[topk]))
    # finite ground truth only: a NaN item has l = 0 exactly, and ties among such zeros are the exact-tie test's subject
    rng = np.random.default_rng(5 + OHKM_SEEDS[topk])
    gt = (np.stack([rng.uniform(0, 22, (3, 17)), rng.uniform(0, 24, (3, 17))], -1) * 4.0).astype(np.float32)
    tw = rng.uniform(0.5, 1.0, (3, 17)).astype(np.float32)
    d["gt"], d["tw"], d["gt_np"], d["tw_np"] = torch.tensor(gt).to(DEV), torch.tensor(tw).to(DEV), gt, tw
    want = O.evaluate(d["heat"], None, None, gt, tw, d["decode"], d["sigma"], O.OHKM, topk)
    gap = _ohkm_gap(want["joint_loss"], topk)
    print(f"topk {topk}: smallest relative gap at the cut = {gap:.3e}")
    assert gap > 1e-3                                                  # the precondition: rounding cannot move the selection (no frame skipped)
    got = _run(d, "ohkm", topk)
    want = _check(d, got, "ohkm", topk)
    assert want["sel"].sum(1).tolist() == [min(topk, 17)] * 3


def test_ohkm_exact_tie_goes_to_the_smaller_index():
    """joints 2 and 5 share weight row, bias and ground truth: their l_bj are bit-identical and the largest of the frame; topk = 1 cuts
    between them, and joint 2 carries all the gradient"""
    d = dict(_case(2, 8, 32, 17, 16, seed=3))
    wt, bias = d["wt"].clone(), d["bias"].clone()
    wt[2] *= 6.0                                                       # large logits: the largest loss
    wt[5], bias[5] = wt[2], bias[2]
    gt = d["gt_np"].copy()
    gt[:] = (20.0, 24.0)
    d.update(wt=wt, bias=bias, gt=torch.tensor(gt).to(DEV), tw=None, gt_np=gt, tw_np=None, wt64=wt.cpu().to(torch.float64).numpy())
    d["heat"] = capf.kp_head_forward(d["x"], wt, bias, want_heat=True)[3].cpu().numpy()
    got = _run(d, "ohkm", 1, tw=False)
    jl = got["joint_loss"].cpu()
    assert torch.equal(jl[:, 2], jl[:, 5]) and (jl[:, 2:3] >= jl).all() and (jl[:, 2] > jl[:, [0, 1, 3, 4, 6, 7]].max(1).values).all()
    dw, db = got["dweight"].cpu(), got["dbias"].cpu()
    assert dw[2].abs().max() > 0 and db[2] != 0
    rest = [0, 1, 3, 4, 5, 6, 7]
    assert not dw[rest].abs().max().item() and not db[rest].abs().max().item()
    _check(d, got, "ohkm", 1, tw=False)
    # topk = 2 takes both, with equal gradients
    got2 = _run(d, "ohkm", 2, tw=False)
    assert torch.equal(got2["dweight"][2], got2["dweight"][5]) and got2["dweight"][5].abs().max() > 0


# ---- determinism ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["mean", "ohkm"])
def test_bits_do_not_depend_on_the_scratch_buffer(reduction):
    """two calls on two scratch buffers of the test's own, both alive at once, one filled with NaN and one with 1e30: bit-equal everywhere"""
    d = _case(3, 17, 32, 24, 22)
    a, sa, _ = _raw(d, reduction, float("nan"))
    b, sb, _ = _raw(d, reduction, 1e30)
    assert sa.data_ptr() != sb.data_ptr()
    for name in OUTPUTS:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name
    ref = _run(d, reduction, 8)
    for name in OUTPUTS:
        assert torch.equal(a[name].view(torch.int32), ref[name].view(torch.int32)), name


def test_joint_loss_bits_depend_on_the_frame_alone():
    d = _case(3, 17, 32, 24, 22)
    batch = _run(d)["joint_loss"]
    for pos in (0, 2):
        one = capf.kp_heatmap_loss(d["x"][pos:pos + 1].contiguous(), d["wt"], d["bias"], d["gt"][pos:pos + 1].contiguous(),
                                   d["tw"][pos:pos + 1].contiguous(), d["decode"], d["sigma"], want_grads=False)[1]
        assert torch.equal(one[0].view(torch.int32), batch[pos].view(torch.int32)), pos
    # ... and at another position of another batch
    perm = [2, 0, 1]
    moved = capf.kp_heatmap_loss(d["x"][perm].contiguous(), d["wt"], d["bias"], d["gt"][perm].contiguous(), d["tw"][perm].contiguous(),
                                 d["decode"], d["sigma"], "ohkm", 3)[1]
    assert torch.equal(moved.view(torch.int32), batch[perm].view(torch.int32))


# ---- 16-bit maps ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
def test_16_bit_maps(dtype):
    d = _case(3, 17, 32, 24, 22, dtype=dtype)
    for reduction in ("mean", "ohkm"):
        got = _run(d, reduction, 8)
        assert got["dmap"] is None
        _check(d, got, reduction, 8, names=("loss", "joint_loss", "dweight", "dbias"))
    with pytest.raises(capf.CapfError, match=r"capf_kp_heatmap_loss failed \(-2\)"):       # CAPF_ERR_UNSUPPORTED
        capf.kp_heatmap_loss(d["x"], d["wt"], d["bias"], d["gt"], d["tw"], d["decode"], d["sigma"], want_dmap=True)


# ---- accumulate, all-NULL gradients -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["mean", "ohkm"])
def test_accumulate_adds_onto_a_prefilled_dmap(reduction):
    d = _case(3, 17, 32, 17, 16)
    plain = _run(d, reduction, 8)
    prefill = torch.randn(d["x"].shape, device=DEV, generator=torch.Generator(DEV).manual_seed(9))
    into = prefill.clone()
    acc = _run(d, reduction, 8, dmap_accumulate_into=into)
    assert acc["dmap"] is into
    assert torch.equal(into.view(torch.int32), (prefill + plain["dmap"]).view(torch.int32))
    for name in ("loss", "joint_loss", "dweight", "dbias"):
        assert torch.equal(acc[name].view(torch.int32), plain[name].view(torch.int32)), name


@pytest.mark.parametrize("reduction", ["mean", "ohkm"])
def test_loss_alone_is_bit_equal_to_the_full_call(reduction):
    d = _case(3, 17, 32, 24, 22)
    full = _run(d, reduction, 8)
    alone = _run(d, reduction, 8, want_grads=False, want_dmap=False)
    assert alone["dweight"] is None and alone["dbias"] is None and alone["dmap"] is None
    for name in ("loss", "joint_loss"):
        assert torch.equal(alone[name].view(torch.int32), full[name].view(torch.int32)), name


# ---- NaN --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["mean", "ohkm"])
def test_nan_in_one_map_pixel(reduction):
    """joint_loss is NaN for exactly the (frame, joint) items whose logits hold a NaN -- read off capf_kp_head_forward's `heat` on the same
    map -- and whose effective weight is not 0; the loss is NaN; the other frames keep their bits.
    One joint's weight at the NaN's channel is set to 0.  The logit is the forward's fma chain bit for bit, and fma(NaN, 0, z) is NaN in
    IEEE arithmetic, so that joint's logit is NaN in `heat` too and its joint_loss is NaN like the others': a zero weight does not spare a
    joint (the test asserts that this is what `heat` says, and holds the loss to `heat`)."""
    d = dict(_case(3, 17, 32, 24, 22))
    x, wt = d["x"].clone(), d["wt"].clone()
    wt[4, 6] = 0.0
    d.update(wt=wt)
    clean = _run(d, reduction, 8, tw=False)
    x[1, 13, 5, 6] = float("nan")
    d.update(x=x)
    heat = capf.kp_head_forward(x, wt, d["bias"], want_heat=True)[3].cpu()
    nan_logits = torch.isnan(heat).flatten(2).any(2)                    # [B, J]
    assert nan_logits[1].all() and not nan_logits[0].any() and not nan_logits[2].any()
    got = _run(d, reduction, 8, tw=False)
    jl = got["joint_loss"].cpu()
    w = torch.tensor(O.effective_weight(d["gt_np"], None, d["decode"], d["sigma"], 24, 22) != 0)
    assert (w[1].sum() > 0) and (~w[1]).sum() > 0                       # frame 1 has items of both kinds
    assert torch.isnan(got["loss"]).all()
    assert torch.equal(torch.isnan(jl), nan_logits & w)
    assert not jl[1][~w[1]].abs().max().item()                          # an item of effective weight 0 is an exact 0 even there
    for b in (0, 2):
        assert torch.equal(jl[b].view(torch.int32), clean["joint_loss"].cpu()[b].view(torch.int32))


# ---- scratch hygiene --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reduction", ["mean", "ohkm"])
def test_exact_size_scratch_between_nan_guard_bands(reduction):
    d = _case(3, 17, 32, 24, 22)
    band = 4096
    got, scratch, buf = _raw(d, reduction, float("nan"), band)
    assert torch.isnan(buf[:band]).all() and torch.isnan(buf[band + scratch.numel():]).all()
    ref = _run(d, reduction, 8)
    for name in OUTPUTS:
        assert torch.equal(got[name].view(torch.int32), ref[name].view(torch.int32)), name
