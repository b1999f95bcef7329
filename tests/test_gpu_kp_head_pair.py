"""GPU: capf_kp_head_forward_pair on random maps whose two halves are INDEPENDENT frames (kp_head_pair_cases).

Nothing of the new kernels enters an expectation: the fused logits are compared EXACTLY with 0.5 * (h[b] + F(h)[b]) evaluated in float32 on
the host, h being the `heat` of the EXISTING capf_kp_head_forward on the same 2 * Bsrc-frame map and F the flip / swap / shift in numpy; the
argmax outputs EXACTLY with kp_head_cases' numpy decode of that float32 heatmap; the integral outputs with the float64 torch evaluation
within 4 x d32 + 1e-6 x scale (d32: torch's own float32 evaluation against float64); the stacks EXACTLY with their formulas and with
capf_preprocess_points(mode = 2).  Every test prints worst error / bound per case (pytest -s)."""
import numpy as np
import pytest
import torch

import kp_head_cases as K
import kp_head_pair_cases as KP
from capf import lib as capf

pytestmark = pytest.mark.gpu

DECODE = (3.7, 0.5, 4.0, -1.25)          # sx, ox, sy, oy: one product that rounds, one that is exact
MIRROR_W = 192.0
_CASES = {}


def _ids(shape):
    return "x".join(str(s) for s in shape)


def _case(shape, seed, dtype=torch.float32):
    """pair_case and the existing single entry's `heat` on its 2 * Bsrc-frame map: computed once per session, never modified"""
    key = (shape, seed, dtype)
    if key not in _CASES:
        torch.set_num_threads(min(16, torch.get_num_threads()))
        c = KP.pair_case(shape, seed, dtype)
        c["h"] = capf.kp_head_forward(_dev(c["X"], dtype), _dev(c["Wt"]), _dev(c["bias"]), capf.KP_ARGMAX, want_heat=True)[3].cpu().numpy()
        _CASES[key] = c
    return _CASES[key]


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(a).to(dtype).cuda().contiguous()


def _pair(c, mode, shift, beta=1.0, decode=DECODE, to_image=None, dtype=torch.float32, want_score=True, want_heat=False, X=None, mirror_width=MIRROR_W):
    out = capf.kp_head_forward_pair(_dev(c["X"] if X is None else X, dtype), _dev(c["Wt"]), _dev(c["bias"]), mode, beta, c["swap"], shift, decode,
                                    _dev(to_image), mirror_width, want_score, want_heat)
    torch.cuda.synchronize()
    return [None if t is None else t.cpu().numpy() for t in out]


def _check_fused_and_argmax(c, shift, dtype=torch.float32):
    """heat and the argmax outputs of one case, exactly; returns kcrop2[0]"""
    Bsrc = c["shape"][0]
    A = K.sample_to_image(Bsrc)
    want_heat = KP.fuse(c["h"], c["swap"], shift)
    assert want_heat.dtype == np.float32
    kcrop2, score, k2d2, heat = _pair(c, capf.KP_ARGMAX, shift, to_image=A, dtype=dtype, want_heat=True)
    assert np.array_equal(heat, want_heat)
    xy, sc, _ = K.decode_argmax(want_heat)
    kc = K.kcrop_f32(xy, DECODE)
    assert np.array_equal(kcrop2[0], kc) and np.array_equal(score, sc) and np.array_equal(k2d2[0], KP.image_f32(kc, A))
    # the same keypoints without heat / score / to_image, and the same heat under the integral decode
    k2, s2, a2, h2 = _pair(c, capf.KP_ARGMAX, shift, dtype=dtype, want_score=False)
    assert np.array_equal(k2, kcrop2) and s2 is None and a2 is None and h2 is None
    assert np.array_equal(_pair(c, capf.KP_INTEGRAL, shift, 3.0, dtype=dtype, want_heat=True)[3], want_heat)
    return kcrop2[0]


# ---- fused logits and the argmax decode: exact -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", KP.SHAPES, ids=_ids)
def test_fused_logits_and_argmax_are_exact(shape):
    moved = 0
    for seed in K.SEEDS:
        c = _case(shape, seed)
        k0, k1 = (_check_fused_and_argmax(c, shift) for shift in (False, True))
        moved += int((k0 != k1).any(-1).sum())
    print(f"  {_ids(shape)}: keypoints that differ between shift = 0 and shift = 1: {moved}")
    if shape[2] == 1:
        assert moved == 0                  # one column: the shift has nothing to shift
    if shape == (1, 8, 8, 32, 17):
        assert moved > 0                   # the flag cannot be ignored


def test_the_mirror_half_is_read_at_the_swapped_joint_and_the_mirrored_column():
    """a wrong x, a wrong swap or an ignored half would survive a true mirror: here the mirror half alone carries the maximum"""
    H, W, J = 5, 7, 17
    spots = {j: (j % H, (3 * j + 1) % W) for j in range(J)}
    hm = np.full((2, J, H, W), -1.0, np.float32)
    for j, (y, x) in spots.items():
        hm[1, j, y, x] = 5.0               # frame Bsrc + 0, joint j of the mirror
    X = np.zeros((2, H, W, 20), np.float32)
    X[..., :J] = hm.transpose(0, 2, 3, 1)
    c = {"X": X, "Wt": np.eye(J, 20, dtype=np.float32), "bias": None, "swap": KP.H36M_SWAP, "shape": (1, H, W, 20, J)}
    for shift in (False, True):
        kcrop2, score, _, heat = _pair(c, capf.KP_ARGMAX, shift, decode=(1.0, 0.0, 1.0, 0.0), want_heat=True)
        for j in range(J):
            y, x = spots[KP.H36M_SWAP[j]]
            # flip_back puts the spot on column W - 1 - x; the shift moves it one column to the right: the last column falls off, and
            # column 0 keeps its own value beside its copy in column 1
            cols = [W - 1 - x] if not shift else [cx for cx in ((0, 1) if x == W - 1 else (W - x,)) if cx < W]
            want = np.full((H, W), -1.0, np.float32)
            want[y, cols] = 2.0                              # 0.5 * (-1 + 5)
            assert np.array_equal(heat[0, j], want), (j, shift)
            if cols:                                         # (the spot's neighbours are equal: no quarter shift)
                assert score[0, j] == 2.0 and tuple(kcrop2[0, 0, j]) == (float(cols[0]), float(y)), (j, shift, kcrop2[0, 0, j])
            else:
                assert score[0, j] == -1.0 and tuple(kcrop2[0, 0, j]) == (0.0, 0.0)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16], ids=["bf16", "fp16"])
@pytest.mark.parametrize("shape", KP.DTYPE_SHAPES, ids=_ids)
def test_16_bit_maps(shape, dtype):
    A = K.sample_to_image(shape[0])
    for seed in K.SEEDS[:2]:
        c = _case(shape, seed, dtype)
        for shift in (False, True):
            _check_fused_and_argmax(c, shift, dtype)
            for beta in (1.0, 25.0):
                k64, a64, s64, bk, ba, bs = KP.integral_pair_case(c, shift, beta, DECODE, A)
                kcrop2, score, k2d2, _ = _pair(c, capf.KP_INTEGRAL, shift, beta, DECODE, A, dtype=dtype)
                ek, ea, es = np.abs(kcrop2[0] - k64).max(), np.abs(k2d2[0] - a64).max(), np.abs(score - s64).max()
                print(f"  {_ids(shape)} seed {seed} {dtype} shift {int(shift)} beta {beta:g}: kcrop {ek / bk:.2f}  k2d {ea / ba:.2f}  score {es / bs:.2f} of the bound")
                assert ek <= bk and ea <= ba and es <= bs


# ---- integral decode against float64 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", KP.SHAPES, ids=_ids)
def test_integral_decode_vs_fp64(shape):
    A = K.sample_to_image(shape[0])
    for seed in K.SEEDS:
        c = _case(shape, seed)
        for shift in (False, True):
            for beta, decode in ((1.0, DECODE), (25.0, DECODE), (25.0, (1.0, 0.0, 1.0, 0.0))):
                k64, a64, s64, bk, ba, bs = KP.integral_pair_case(c, shift, beta, decode, A)
                kcrop2, score, k2d2, _ = _pair(c, capf.KP_INTEGRAL, shift, beta, decode, A)
                ek, ea, es = np.abs(kcrop2[0] - k64).max(), np.abs(k2d2[0] - a64).max(), np.abs(score - s64).max()
                print(f"  {_ids(shape)} seed {seed} shift {int(shift)} beta {beta:g} sx {decode[0]:g}: kcrop {ek:.2e} / {bk:.2e} ({ek / bk:.2f})   "
                      f"k2d {ea:.2e} / {ba:.2e} ({ea / ba:.2f})   score {es:.2e} / {bs:.2e}")
                assert ek <= bk and ea <= ba and es <= bs


# ---- the stacks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", KP.SHAPES, ids=_ids)
def test_stacks_are_exact(shape):
    Bsrc, J = shape[0], shape[4]
    A = K.sample_to_image(Bsrc)
    c = _case(shape, 1)
    for mode, beta in ((capf.KP_ARGMAX, 1.0), (capf.KP_INTEGRAL, 7.0)):
        for mirror_width in (MIRROR_W, 47.5):
            kcrop2, _, k2d2, _ = _pair(c, mode, True, beta, DECODE, A, mirror_width=mirror_width)
            assert kcrop2.shape == (2, Bsrc, J, 2) and k2d2.shape == (2, Bsrc, J, 2)
            mc, md = KP.mirrored_set(kcrop2[0], k2d2[0], c["swap"], mirror_width)
            assert np.array_equal(kcrop2[1], mc) and np.array_equal(k2d2[1], md)
        if J == 17:            # (after the mirror_width = 192 run) the H36M table: capf_preprocess_points(mode = 2), bit for bit
            kcrop2, _, k2d2, _ = _pair(c, mode, True, beta, DECODE, A)
            _, d2, c2 = capf.preprocess_points(None, _dev(k2d2[0]), _dev(kcrop2[0]), mode=2)
            assert np.array_equal(d2.cpu().numpy(), k2d2) and np.array_equal(c2.cpu().numpy(), kcrop2)
    # without to_image: no k2d2, the same kcrop2
    k_only, _, none, _ = _pair(c, capf.KP_ARGMAX, True)
    assert none is None and np.array_equal(k_only, _pair(c, capf.KP_ARGMAX, True, to_image=A)[0])


# ---- NaN -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["mirror", "mirror column 0", "source"])
def test_nan_in_either_half_takes_the_whole_source_frame_and_nothing_else(where):
    """A 1x1 conv hands a NaN map value to every joint of its frame.  Under shift = 1 no pixel reads the mirror's column 0: a NaN there
    counts all the same (the rule names every logit of (Bsrc + b, swap[j]))."""
    shape = (3, 16, 12, 48, 17)
    Bsrc, b = shape[0], 1
    A = K.sample_to_image(Bsrc)
    c = _case(shape, 0)
    X = c["X"].copy()
    X[{"mirror": Bsrc + b, "mirror column 0": Bsrc + b, "source": b}[where], 9, {"mirror": 7, "mirror column 0": 0, "source": 7}[where], 5] = np.nan
    rest = [i for i in range(Bsrc) if i != b]
    for mode, beta in ((capf.KP_ARGMAX, 1.0), (capf.KP_INTEGRAL, 7.0)):
        for shift in (False, True):
            clean = _pair(c, mode, shift, beta, DECODE, A)
            kcrop2, score, k2d2, _ = _pair(c, mode, shift, beta, DECODE, A, X=X)
            assert np.isnan(kcrop2[:, b]).all() and np.isnan(k2d2[:, b]).all() and np.isnan(score[b]).all(), (where, mode, shift)
            assert np.array_equal(kcrop2[:, rest], clean[0][:, rest]) and np.array_equal(score[rest], clean[1][rest])
            assert np.array_equal(k2d2[:, rest], clean[2][:, rest])


# ---- batch independence, the scratch ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 16, 12, 48, 17), (3, 64, 48, 32, 17)], ids=_ids)
def test_a_source_frame_depends_on_its_two_frames_alone(shape):
    Bsrc = shape[0]
    c = _case(shape, 1)
    A = K.sample_to_image(Bsrc)
    for mode, beta in ((capf.KP_ARGMAX, 1.0), (capf.KP_INTEGRAL, 7.0)):
        kcrop2, score, k2d2, heat = _pair(c, mode, True, beta, DECODE, A, want_heat=True)
        junk = torch.full((1 << 20,), float("nan"), device="cuda")           # the lone runs' scratch lands on other, poisoned memory
        for b in range(Bsrc):
            k1, s1, a1, h1 = _pair(c, mode, True, beta, DECODE, A[b:b + 1], want_heat=True, X=c["X"][[b, Bsrc + b]])
            assert np.array_equal(k1[:, 0], kcrop2[:, b]) and np.array_equal(a1[:, 0], k2d2[:, b])
            assert np.array_equal(s1[0], score[b]) and np.array_equal(h1[0], heat[b])
        del junk


def test_single_entry_keeps_its_bits_around_a_pair_call_on_the_same_scratch():
    lib = capf.load_library()
    shape = (2, 16, 12, 48, 17)
    Bsrc, H, W, C, J = shape
    c = _case(shape, 2)
    x, w, bias, A = _dev(c["X"]), _dev(c["Wt"]), _dev(c["bias"]), _dev(K.sample_to_image(2 * Bsrc))
    nbytes = lib.capf_kp_head_scratch_bytes(2 * Bsrc, H, W, C, J, 0)
    assert nbytes >= lib.capf_kp_head_pair_scratch_bytes(Bsrc, H, W, C, J)
    scratch = torch.empty(nbytes // 4, device="cuda")
    dec = (capf.c_float * 4)(*DECODE)

    def single(mode):
        out = [torch.empty(2 * Bsrc, J, 2, device="cuda"), torch.empty(2 * Bsrc, J, 2, device="cuda"), torch.empty(2 * Bsrc, J, device="cuda"),
               torch.empty(2 * Bsrc, J, H, W, device="cuda")]
        capf._call("capf_kp_head_forward", capf._stream(x), capf._p(x), 0, capf._p(w), capf._p(bias), 2 * Bsrc, H, W, C, J, mode, 3.0, dec,
                   capf._p(A), *[capf._p(t) for t in out], capf._p(scratch), nbytes)
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in out]

    for mode in (0, 1):
        before = single(mode)
        kcrop2 = torch.empty(2, Bsrc, J, 2, device="cuda")
        capf._call("capf_kp_head_forward_pair", capf._stream(x), capf._p(x), 0, capf._p(w), capf._p(bias), Bsrc, H, W, C, J, mode, 3.0,
                   (capf.c_int32 * J)(*c["swap"]), 1, dec, None, MIRROR_W, capf._p(kcrop2), None, None, None, capf._p(scratch), nbytes)
        torch.cuda.synchronize()
        assert np.array_equal(kcrop2.cpu().numpy(), _pair(c, mode, True, 3.0)[0])          # (the pair call on that scratch: the binding's bits)
        assert all(np.array_equal(a, b) for a, b in zip(before, single(mode)))
        assert np.array_equal(before[3], c["h"])
