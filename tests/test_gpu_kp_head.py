"""GPU: the stand-alone 2-D keypoint head (capf_kp_head_forward / capf_kp_head_backward) against the float64 evaluation of kp_head_cases.

Bounds: 4 x d32 + 1e-6 x scale everywhere a value is continuous (d32: torch's own float32 evaluation against float64, kp_head_cases);
the argmax decode is compared EXACTLY -- with the numpy decode of the kernel's own `heat`, and, since every gap the decode decides on is at
least 50 x d32 wide (test_kp_head_api.py checks that on the CPU for every case), with the float64 decode as well.
Every test prints worst error / bound per case (pytest -s; EXPERIMENTS R24.1 has the table)."""
import numpy as np
import pytest
import torch

import kp_head_cases as K
from capf import lib as capf

pytestmark = pytest.mark.gpu

SHAPES = K.SHAPES + (K.ONE_INTERIOR,)
DECODE = (3.7, 0.5, 4.0, -1.25)          # sx, ox, sy, oy: one product that rounds, one that is exact
_CASES = {}


def _case(shape, seed, dtype=torch.float32):
    """heat_case, computed once per session and never modified"""
    key = (shape, seed, dtype)
    if key not in _CASES:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        _CASES[key] = K.heat_case(shape, seed, dtype)
    return _CASES[key]


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(a).to(dtype).cuda().contiguous()


def _fwd(c, mode, beta=1.0, decode=DECODE, to_image=None, dtype=torch.float32, want_score=True, want_heat=False, bias=True, X=None):
    out = capf.kp_head_forward(_dev(c["X"] if X is None else X, dtype), _dev(c["Wt"]), _dev(c["bias"]) if bias else None, mode, beta, decode,
                               _dev(to_image), want_score, want_heat)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def _ids(shape):
    return "x".join(str(s) for s in shape)


# ---- logits --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_logits_vs_fp64_and_argmax_decode(shape):
    for seed in K.SEEDS:
        c = _case(shape, seed)
        kcrop, score, k2d, heat = _fwd(c, capf.KP_ARGMAX, want_heat=True)
        err = np.abs(heat.astype(np.float64) - c["z64"]).max()
        print(f"  {_ids(shape)} seed {seed}: heat max|hip - fp64| {err:.2e} bound {c['bound']:.2e} ratio {err / c['bound']:.2f}")
        assert err <= c["bound"]
        assert k2d is None
        # heat does not depend on which other outputs are asked for, nor on the decode
        for mode, ws in ((capf.KP_ARGMAX, False), (capf.KP_INTEGRAL, True)):
            assert np.array_equal(_fwd(c, mode, want_score=ws, want_heat=True, to_image=K.sample_to_image(shape[0]))[3], heat)
        # the decode of the kernel's own logits, exactly; and (margin rule) of the float64 logits
        xy, sc, _ = K.decode_argmax(heat)
        assert np.array_equal(kcrop, K.kcrop_f32(xy, DECODE)) and np.array_equal(score, sc)
        xy64, sc64, _ = K.decode_argmax(c["z64"])
        assert np.array_equal(xy, xy64)
        assert np.abs(score - sc64).max() <= c["bound"]
        # the same keypoints without `heat` and without `score`
        k2, s2, _, h2 = _fwd(c, capf.KP_ARGMAX, want_score=False)
        assert np.array_equal(k2, kcrop) and s2 is None and h2 is None


def _onehot_case(heatmaps, spare=0):
    """maps whose channel j IS heatmap j (weight = identity rows, no bias; `spare` more channels of zeros, C rounded up to a multiple of 4):
    heatmaps [B, J, H, W] float32"""
    B, J, H, W = heatmaps.shape
    C = (J + spare + 3) // 4 * 4
    X = np.zeros((B, H, W, C), np.float32)
    X[..., :J] = heatmaps.transpose(0, 2, 3, 1)
    return {"X": X, "Wt": np.eye(J, C, dtype=np.float32), "bias": None}


def test_argmax_rules_on_hand_built_heatmaps():
    H, W = 6, 7
    names, maps, want = [], [], []

    def add(name, h, xy):
        names.append(name); maps.append(h.astype(np.float32)); want.append(xy)

    base = -np.ones((H, W))
    h = base.copy(); h[2, 3] = h[4, 1] = h[2, 5] = 2.0; h[2, 4] = 1.0; h[2, 2] = 0.5; h[3, 3] = 0.5; h[1, 3] = 1.0
    add("tie: first index wins, shifts read its neighbours", h, (3.25, 1.75))
    for name, (py, px) in {"top border": (0, 3), "bottom border": (H - 1, 3), "left border": (2, 0), "right border": (2, W - 1),
                           "corner NW": (0, 0), "corner NE": (0, W - 1), "corner SW": (H - 1, 0), "corner SE": (H - 1, W - 1),
                           "px == 1 is not interior": (2, 1), "py == 1 is not interior": (1, 3)}.items():
        h = base.copy(); h[py, px] = 3.0
        h[min(py + 1, H - 1), px] += 0.5; h[py, min(px + 1, W - 1)] += 0.5       # unequal neighbours: a shift would show
        add(name, h, (float(px), float(py)))
    for name, (py, px) in {"px == W - 2 is interior": (2, W - 2), "py == H - 2 is interior": (H - 2, 3)}.items():
        h = base.copy(); h[py, px] = 3.0
        h[py + 1, px] += 0.5; h[py, px + 1] += 0.5
        add(name, h, (px + 0.25, py + 0.25))
    h = base.copy(); h[3, 3] = 1.0
    add("equal neighbours: shift 0", h, (3.0, 3.0))
    h = base.copy(); h[3, 3] = 1.0; h[3, 2] = 0.5; h[4, 3] = 0.25
    add("negative x shift, positive y shift", h, (2.75, 3.25))
    h = base.copy() - 1.0; h[3, 4] = -0.5; h[3, 5] = -0.75
    add("all negative: coordinates (ox, oy), score kept", h, None)
    h = base.copy(); h[2, 2] = 0.0
    add("maximum exactly 0: score <= 0", h, None)
    J = len(maps)
    hm = np.stack(maps)[None].repeat(2, 0)                                         # two equal frames
    A = K.sample_to_image(2)
    c = _onehot_case(hm)
    kcrop, score, k2d, heat = _fwd(c, capf.KP_ARGMAX, bias=False, want_heat=True, to_image=A)
    assert np.array_equal(heat, hm)
    for j, (name, xy) in enumerate(zip(names, want)):
        x, y = xy if xy is not None else (0.0, 0.0)
        exp = K.kcrop_f32(np.array([x, y]), DECODE)
        print(f"  {name}: {kcrop[0, j]} score {score[0, j]}")
        assert np.array_equal(kcrop[0, j], exp) and np.array_equal(kcrop[1, j], exp), (name, kcrop[:, j], exp)
        assert score[0, j] == hm[0, j].max() == score[1, j], name
    assert np.array_equal(kcrop[0, -2], np.float32([DECODE[1], DECODE[3]])) and score[0, -2] == -0.5 and score[0, -1] == 0.0
    # NaN.  A 1x1 conv hands a NaN map value to every joint of its frame (NaN x 0), and finite inputs cannot make one (an fma's product is
    # never an infinity of its own), so a NaN logit is confined to a frame by a NaN pixel and to a joint by a NaN bias: one run each
    clean = {m: _fwd(c, m, 2.0, DECODE, A, bias=False) for m in (capf.KP_ARGMAX, capf.KP_INTEGRAL)}
    poisoned = {"X": c["X"].copy(), "Wt": c["Wt"], "bias": None}
    poisoned["X"][1, 4, 4, 2] = np.nan
    nan_joint = 3
    biased = {"X": c["X"], "Wt": c["Wt"], "bias": np.zeros(J, np.float32)}
    biased["bias"][nan_joint] = np.nan
    for m in (capf.KP_ARGMAX, capf.KP_INTEGRAL):
        kc, sc, k2, _ = _fwd(poisoned, m, 2.0, DECODE, A, bias=False)
        assert np.isnan(kc[1]).all() and np.isnan(sc[1]).all() and np.isnan(k2[1]).all()
        assert all(np.array_equal(g[0], w[0]) for g, w in zip((kc, sc, k2), clean[m]))                  # the other frame: untouched
        kc, sc, k2, _ = _fwd(biased, m, 2.0, DECODE, A)
        assert np.isnan(kc[:, nan_joint]).all() and np.isnan(sc[:, nan_joint]).all() and np.isnan(k2[:, nan_joint]).all()
        rest = [j for j in range(J) if j != nan_joint]
        assert all(np.array_equal(g[:, rest], w[:, rest]) for g, w in zip((kc, sc, k2), clean[m]))      # the other joints: untouched


# ---- integral ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_integral_decode_and_coordinates_vs_fp64(shape):
    A = K.sample_to_image(shape[0])
    for seed in K.SEEDS:
        c = _case(shape, seed)
        for beta in (1.0, 25.0):
            for decode in ((1.0, 0.0, 1.0, 0.0), DECODE):
                k64, a64, s64, bk, ba = K.integral_case(c, beta, decode, A)
                kcrop, score, k2d, _ = _fwd(c, capf.KP_INTEGRAL, beta, decode, A)
                ek, ea = np.abs(kcrop - k64).max(), np.abs(k2d - a64).max()
                print(f"  {_ids(shape)} seed {seed} beta {beta:g} sx {decode[0]:g}: kcrop {ek:.2e} / {bk:.2e} ({ek / bk:.2f})   "
                      f"k2d {ea:.2e} / {ba:.2e} ({ea / ba:.2f})")
                assert ek <= bk and ea <= ba
                assert np.abs(score - s64).max() <= c["bound"]
        # argmax through decode and to_image, against float64
        xy64, _, _ = K.decode_argmax(c["z64"])
        k64, a64 = K.to_outputs(xy64, DECODE, A.astype(np.float64))
        kcrop, _, k2d, _ = _fwd(c, capf.KP_ARGMAX, 1.0, DECODE, A)
        assert np.abs(kcrop - k64).max() <= 1e-6 * max(np.abs(k64).max(), 1.0)
        assert np.abs(k2d - a64).max() <= 4e-7 * max(np.abs(a64).max(), 1.0) + 1e-6 * np.abs(A[:, :, :2]).max() * np.abs(k64).max()


def test_integral_limits_one_hot_and_constant_maps():
    H, W, J = 9, 11, 5
    hm = np.zeros((1, J, H, W), np.float32)
    spots = [(0, 0), (H - 1, W - 1), (4, 7), (8, 0), (3, 10)]
    for j, (y, x) in enumerate(spots):
        hm[0, j, y, x] = 1.0
    kcrop, score, _, _ = _fwd(_onehot_case(hm), capf.KP_INTEGRAL, 1e4, (1.0, 0.0, 1.0, 0.0), bias=False)
    assert np.array_equal(kcrop[0], np.float32([(x, y) for y, x in spots])) and (score == 1.0).all()
    const = np.full((2, 3, H, W), 0.75, np.float32)
    kcrop, score, _, _ = _fwd(_onehot_case(const), capf.KP_INTEGRAL, 3.0, (1.0, 0.0, 1.0, 0.0), bias=False)
    assert np.abs(kcrop - np.float32([(W - 1) / 2, (H - 1) / 2])).max() <= 1e-6 * max(H, W) and (score == 0.75).all()


def test_to_image_null_leaves_k2d_untouched():
    lib = capf.load_library()
    c = _case((2, 8, 8, 32, 17), 0)
    x, w, b = _dev(c["X"]), _dev(c["Wt"]), _dev(c["bias"])
    B, H, W, C = x.shape
    J = w.shape[0]
    kcrop = torch.empty(B, J, 2, device="cuda")
    k2d = torch.full((B, J, 2), 12345.0, device="cuda")
    nbytes = lib.capf_kp_head_scratch_bytes(B, H, W, C, J, 0)
    scratch = torch.empty(nbytes // 4, device="cuda")
    dec = (capf.c_float * 4)(1, 0, 1, 0)
    for mode in (0, 1):
        capf._call("capf_kp_head_forward", capf._stream(x), capf._p(x), 0, capf._p(w), capf._p(b), B, H, W, C, J, mode, 1.0, dec, None,
                   capf._p(kcrop), capf._p(k2d), None, None, capf._p(scratch), nbytes)
        torch.cuda.synchronize()
        assert (k2d == 12345.0).all()


# ---- dtypes --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", [(3, 16, 12, 48, 17), (2, 64, 48, 32, 17), (1, 24, 18, 256, 17), K.ONE_INTERIOR], ids=_ids)
def test_16_bit_maps_vs_fp64_of_the_rounded_map(shape, dtype):
    A = K.sample_to_image(shape[0])
    for seed in K.SEEDS[:2]:
        c = _case(shape, seed, dtype)
        kcrop, score, _, heat = _fwd(c, capf.KP_ARGMAX, dtype=dtype, want_heat=True)
        err = np.abs(heat.astype(np.float64) - c["z64"]).max()
        assert err <= c["bound"]
        xy, sc, _ = K.decode_argmax(heat)
        assert np.array_equal(kcrop, K.kcrop_f32(xy, DECODE)) and np.array_equal(score, sc)
        if K.margins(c["z64"], c["d32"]) >= K.MARGIN:
            assert np.array_equal(xy, K.decode_argmax(c["z64"])[0])
        worst = 0.0
        for beta in (1.0, 25.0):
            k64, a64, _, bk, ba = K.integral_case(c, beta, DECODE, A)
            ki, _, k2i, _ = _fwd(c, capf.KP_INTEGRAL, beta, DECODE, A, dtype=dtype)
            assert np.abs(ki - k64).max() <= bk and np.abs(k2i - a64).max() <= ba
            worst = max(worst, np.abs(ki - k64).max() / bk)
        print(f"  {_ids(shape)} seed {seed} {dtype}: heat {err:.2e} / {c['bound']:.2e}, integral worst ratio {worst:.2f}")


# ---- batch independence, determinism -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 16, 12, 48, 17), (3, 64, 48, 32, 17)], ids=_ids)
def test_a_frame_does_not_depend_on_its_batch(shape):
    c = _case(shape, 1)
    A = K.sample_to_image(shape[0])
    for mode, beta in ((capf.KP_ARGMAX, 1.0), (capf.KP_INTEGRAL, 7.0)):
        whole = _fwd(c, mode, beta, DECODE, A, want_heat=True)
        for b in range(shape[0]):
            alone = _fwd(c, mode, beta, DECODE, A[b:b + 1], want_heat=True, X=c["X"][b:b + 1])
            for w, a in zip(whole, alone):
                assert np.array_equal(w[b:b + 1], a)


def _bwd(c, beta, decode, A, gc, gk, want_dmap=True, dmap=None):
    out = capf.kp_head_backward(_dev(c["X"]), _dev(c["Wt"]), _dev(c["bias"]), _dev(gc), _dev(gk), beta, decode, _dev(A), want_dmap, dmap)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def _cotangents(shape, seed=11):
    rng = np.random.default_rng(seed)
    B, J = shape[0], shape[4]
    return rng.standard_normal((B, J, 2)).astype(np.float32), (100.0 * rng.standard_normal((B, J, 2))).astype(np.float32)


def test_two_runs_give_the_same_bits():
    shape = (2, 64, 48, 32, 17)
    c = _case(shape, 2)
    A = K.sample_to_image(shape[0])
    gc, gk = _cotangents(shape)
    for mode, beta in ((capf.KP_ARGMAX, 1.0), (capf.KP_INTEGRAL, 7.0)):
        first = _fwd(c, mode, beta, DECODE, A, want_heat=True)
        junk = torch.full((1 << 20,), float("nan"), device="cuda")           # the second run's scratch lands on other, poisoned memory
        second = _fwd(c, mode, beta, DECODE, A, want_heat=True)
        del junk
        assert all(np.array_equal(a, b) for a, b in zip(first, second))
    first = _bwd(c, 7.0, DECODE, A, gc, gk)
    junk = torch.full((1 << 20,), float("nan"), device="cuda")
    second = _bwd(c, 7.0, DECODE, A, gc, gk)
    del junk
    assert all(np.array_equal(a, b) for a, b in zip(first, second))


# ---- backward ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_backward_vs_fp64_autograd(shape):
    A = K.sample_to_image(shape[0])
    gc, gk = _cotangents(shape)
    for seed, beta, which in ((0, 1.0, "both"), (1, 25.0, "both"), (2, 3.0, "dkcrop"), (2, 3.0, "dk2d")):
        c = _case(shape, seed)
        a, b = (gc if which != "dk2d" else None), (gk if which != "dkcrop" else None)
        want = K.backward_case(c, beta, DECODE, A, a, b)
        dW, db, dmap = _bwd(c, beta, DECODE, A, a, b)
        assert (db == 0).all() and not np.signbit(db).any()
        line = []
        for name, got in (("dW", dW), ("dmap", dmap)):
            g64, bound = want[name]
            err = np.abs(got - g64.reshape(got.shape)).max()
            line.append(f"{name} {err:.2e} / {bound:.2e} ({err / bound if bound else 0.0:.2f})")
            assert err <= bound, (name, err, bound)
        print(f"  {_ids(shape)} seed {seed} beta {beta:g} {which}: " + "   ".join(line) +
              f"   |dbias64| {np.abs(want['dbias'][0]).max():.1e}")
        # without dmap: the same dW; accumulate = 1: the overwriting result added to what was there, one rounding per element
        assert np.array_equal(_bwd(c, beta, DECODE, A, a, b, want_dmap=False)[0], dW)
        prior = np.random.default_rng(3).standard_normal(dmap.shape).astype(np.float32)
        acc = _bwd(c, beta, DECODE, A, a, b, dmap=_dev(prior))
        assert np.array_equal(acc[0], dW) and np.array_equal(acc[2], prior + dmap)
