"""GPU: CPN's test-time flip -- capf_cpn_decode_pair against the EXISTING capf_cpn_decode on a host-folded map (bit for bit in every case,
decided or not: the arithmetic behind the fold is the same), its `fused` against the fold oracle (tests/cpn_flip_oracle.py), the decode
against tests/cpn_decode_oracle.py on the folded maps (bit for bit where the peaks are decided, undecided cases counted, at most 2 % outside
the 1 x 1 maps), the stacks against their formulas and capf_preprocess_points(mode = 2), hand-checkable pixels, the degenerate rule, the
independence of a pair from its batch, and CA_PF.detect_cpn_flip / forward_detect_cpn_flip.  Every case is one or a few launches on maps of
at most 96 x 72, or a module call at B = 3."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import cpn_decode_oracle as O
import cpn_flip_oracle as F
from capf import lib as capf
from capf import synth

pytestmark = pytest.mark.gpu
J = 17
TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DEC = (4.0, 2.0, 4.0, 2.0)


def _taps():
    return np.array(capf.cpn_decode_taps())


def _affines(B, seed):
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1.0, 1.0, (B, 2, 3)).astype(np.float32)
    A[:, :, :2] *= np.float32(0.01)
    return A


def _np(t):
    return None if t is None else t.cpu().numpy()


def _pair(z2, dtype, Jn, swap, dec=DEC, A=None, mirror_width=192.0, blurred=True, fused=True, prefill=None):
    """capf_cpn_decode_pair on host maps [2 Bsrc, H, W, C] float32 (exact in `dtype`): numpy (kcrop2, score, k2d2 | None, blurred, fused)"""
    heat = torch.from_numpy(z2).to(TORCH[dtype]).cuda().contiguous()
    a = None if A is None else torch.from_numpy(A).cuda()
    out = capf.cpn_decode_pair(heat, Jn, swap, dec, a, mirror_width, want_score=True, want_blurred=blurred, want_fused=fused)
    torch.cuda.synchronize()
    kcrop2, score, k2d2, D, zf = out
    return _np(kcrop2), _np(score), _np(k2d2), _np(D), _np(zf)


def _single(zf, Jn, dec=DEC, A=None, blurred=True):
    """the existing capf_cpn_decode on a float32 host map [B, H, W, J]"""
    heat = torch.from_numpy(np.ascontiguousarray(zf)).cuda()
    a = None if A is None else torch.from_numpy(A).cuda()
    kcrop, score, k2d, D = capf.cpn_decode(heat, Jn, dec, a, want_score=True, want_blurred=blurred)
    torch.cuda.synchronize()
    return _np(kcrop), _np(score), _np(k2d), _np(D)


def _bits32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(a, b):
    return np.array_equal(_bits32(a), _bits32(b))


def _same_bits64(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.int64), np.ascontiguousarray(b).view(np.int64))


def _swaps(Jn):
    return (capf.H36M_SWAP, capf.COCO_SWAP) if Jn == 17 else (F.involution(Jn), tuple(range(Jn)))


def _torch_fold(z2, swap):
    """0.5 * (z[:B] + z[B:].flip(2)[..., swap]) on the float32 values, as torch evaluates it"""
    z = torch.from_numpy(z2)
    B = z.shape[0] // 2
    return (0.5 * (z[:B, :, :, :len(swap)] + z[B:].flip(2)[..., list(swap)])).numpy()


# ---- 1. the same bits as the single decode on a host-folded map ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_pair_equals_the_single_decode_on_the_host_folded_map(dtype):
    cases = 0
    for si, (H, W) in enumerate(O.SHAPES):
        dec = DEC if si % 2 == 0 else (6.0, 3.0, 6.0, 3.0)
        for ji, (Jn, C) in enumerate(O.JC):
            for B in O.BATCHES:
                seed = 2000 * si + 20 * ji + B
                z2 = O.make_maps(2 * B, H, W, C, Jn, seed, dtype)
                A = _affines(B, seed)
                for swap in _swaps(Jn):
                    zf = _torch_fold(z2, swap)
                    assert _same_bits(zf, F.fold(z2, swap))
                    kcrop2, score, k2d2, D, fused = _pair(z2, dtype, Jn, swap, dec, A)
                    k1, s1, q1, D1 = _single(zf, Jn, dec, A)
                    what = (H, W, Jn, C, B, swap)
                    assert fused.shape == (B, Jn, H, W) and _same_bits(fused, zf.transpose(0, 3, 1, 2)), what
                    assert kcrop2.shape == (2, B, Jn, 2) and k2d2.shape == (2, B, Jn, 2) and score.shape == (B, Jn), what
                    assert _same_bits(kcrop2[0], k1) and _same_bits(score, s1) and _same_bits(k2d2[0], q1), what
                    assert D.shape == (B, Jn, H + 20, W + 20) and _same_bits64(D, D1), what
                    assert np.isfinite(kcrop2).all() and np.isfinite(k2d2).all() and np.isfinite(score).all()
                    cases += B * Jn
    print(f"{dtype}: {cases} (frame, joint) cases bit-equal to capf_cpn_decode on the host-folded map")


# ---- 2. against the decode oracle on the folded maps ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_pair_matches_the_decode_oracle_on_the_folded_maps(dtype):
    """test 1 ties every (J, C) of the pair entry to the single decode, which tests/test_gpu_cpn_detect.py holds to this oracle at every (J, C);
    here: every shape and batch at J = 1, 17 (H36M table, C = 20) and 32"""
    g = _taps()
    undecided = counted = checked = 0
    worst_blur = 0.0
    for si, (H, W) in enumerate(O.SHAPES):
        for Jn, C in ((1, 1), (17, 20), (32, 32)):
            swap = capf.H36M_SWAP if Jn == 17 else F.involution(Jn)
            for B in O.BATCHES:
                seed = 3000 * si + 10 * Jn + B
                z2 = O.make_maps(2 * B, H, W, C, Jn, seed, dtype)
                A = _affines(B, seed)
                zf = F.fold(z2, swap)
                kcrop2, score, k2d2, D, _ = _pair(z2, dtype, Jn, swap, DEC, A)
                for b in range(B):
                    for j in range(Jn):
                        r = O.decode(zf[b, :, :, j], DEC, A[b], g)
                        assert not r["degenerate"]
                        P = np.zeros_like(r["D"])
                        P[10:10 + H, 10:10 + W] = np.abs(zf[b, :, :, j] / zf[b, :, :, j].max())
                        gamma = 44 * O.U * O.blur(P, g)
                        ratio = float((np.abs(D[b, j] - r["D"]) / np.maximum(gamma, 1e-300)).max())
                        worst_blur = max(worst_blur, ratio)
                        assert ratio <= 1.0, (H, W, Jn, B, b, j, ratio)
                        tie_by_construction = (H, W) == (1, 1)
                        if not tie_by_construction:
                            counted += 1
                            undecided += not r["decided"]
                        if r["decided"] or tie_by_construction:
                            checked += 1
                            what = (H, W, Jn, B, b, j, r["peaks"], r["gap1"], r["gap2"])
                            assert _same_bits(kcrop2[0, b, j], r["kcrop"]), ("kcrop", kcrop2[0, b, j], r["kcrop"], what)
                            assert _same_bits(k2d2[0, b, j], r["k2d"]), ("k2d", k2d2[0, b, j], r["k2d"], what)
                            assert _same_bits(score[b, j], r["score"]), ("score", score[b, j], r["score"], what)
    print(f"{dtype}: {checked} (frame, joint) cases equal to the oracle, {undecided} of {counted} undecided and left out; "
          f"worst |blurred - oracle| = {worst_blur:.3f} gamma")
    assert undecided <= 0.02 * counted, (undecided, counted)


# ---- 3. the stacks ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_stacks_follow_their_formulas_and_preprocess_points(dtype):
    H, W = 16, 12
    for Jn, C in ((1, 1), (17, 20), (32, 32)):
        for B in O.BATCHES:
            z2 = O.make_maps(2 * B, H, W, C, Jn, 40 + Jn + B, dtype)
            A = _affines(B, 41)
            for swap in _swaps(Jn):
                for mw in (192.0, 250.5):
                    kcrop2, _, k2d2, _, _ = _pair(z2, dtype, Jn, swap, DEC, A, mw, blurred=False, fused=False)
                    assert not np.isnan(kcrop2).any() and not np.isnan(k2d2).any()          # (torch.empty hands out whatever was there ...
                    wc, wd = F.mirrored_stacks(kcrop2[0], k2d2[0], swap, mw)
                    assert _same_bits(kcrop2, wc) and _same_bits(k2d2, wd), (Jn, B, swap, mw)
                # without to_image: no k2d2, the same kcrop2
                k_only, _, none, _, _ = _pair(z2, dtype, Jn, swap, DEC, None, 250.5, blurred=False, fused=False)
                assert none is None and _same_bits(k_only, kcrop2)
    # ... so: every element of both stacks is written -- NaN-filled outputs handed to the C entry itself keep no NaN
    B, Jn, C = 3, 17, 20
    z2 = O.make_maps(2 * B, H, W, C, Jn, 43, dtype)
    heat = torch.from_numpy(z2).to(TORCH[dtype]).cuda()
    a = torch.from_numpy(_affines(B, 41)).cuda()
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    kc, kd, sc = nan(2, B, Jn, 2), nan(2, B, Jn, 2), nan(B, Jn)
    p = lambda t: capf.c_void_p(t.data_ptr())
    rc = capf.load_library().capf_cpn_decode_pair(capf.c_void_p(torch.cuda.current_stream().cuda_stream), p(heat), capf.F32 if dtype == "fp32" else capf.BF16,
                                                  B, H, W, C, Jn, (capf.c_int32 * Jn)(*capf.H36M_SWAP), (capf.c_float * 4)(*DEC), p(a), 192.0,
                                                  p(kc), p(kd), p(sc), None, None)
    torch.cuda.synchronize()
    assert rc == 0 and not torch.isnan(kc).any() and not torch.isnan(kd).any() and not torch.isnan(sc).any()
    # J = 17, the H36M table, mirror_width = 192: capf_preprocess_points(mode = 2) of set 0, bit for bit
    _, d2, c2 = capf.preprocess_points(None, kd[0].contiguous(), kc[0].contiguous(), mode=2)
    assert torch.equal(d2, kd) and torch.equal(c2, kc)


# ---- 4. hand-checkable single pixels ----------------------------------------------------------------------------------------------------------
def test_single_pixels_by_hand():
    H, W, Jn = 9, 7, 5
    swap = F.involution(Jn)                      # (0)(1 2)(3 4)
    v = np.float32(3.0)
    for (y, x) in [(4, 3), (1, 1), (7, 5), (3, 6), (0, 0)]:
        for j in range(Jn):
            src = np.zeros((2, H, W, Jn), dtype=np.float32)
            src[0, y, x, j] = v
            both = src.copy()
            both[1, y, W - 1 - x, swap[j]] = v
            mirror_only = np.zeros_like(src)
            mirror_only[1, y, W - 1 - x, swap[j]] = v
            # the single decode of the source pixel, every other joint degenerate (an all-zero map)
            single = np.zeros((1, H, W, Jn), dtype=np.float32)
            single[0, y, x, j] = v
            k1, s1, _, _ = _single(single, Jn, DEC)
            assert _same_bits(k1[0, j], [np.float32(4.0 * x + 2.0), np.float32(4.0) * np.float32(max(0.0, y - 0.25)) + np.float32(2.0)])
            assert _same_bits(s1[0, j], v / np.float32(255) + np.float32(0.5))
            kb, sb, _, _, fb = _pair(both, "fp32", Jn, swap, blurred=False)
            assert _same_bits(kb[0, 0, j], k1[0, j]) and _same_bits(sb[0, j], s1[0, j]), (y, x, j)           # (v + v) / 2 = v: the source's decode
            assert fb[0, j, y, x] == v and np.count_nonzero(fb) == 1
            km, sm, _, _, fm = _pair(mirror_only, "fp32", Jn, swap, blurred=False)
            assert _same_bits(km[0, 0, j], k1[0, j]), (y, x, j)                                             # n = zf / M: the same normalised map
            assert _same_bits(sm[0, j], (v / np.float32(2)) / np.float32(255) + np.float32(0.5))
            assert fm[0, j, y, x] == v / 2 and np.count_nonzero(fm) == 1
            ks, ss, _, _, _ = _pair(src, "fp32", Jn, swap, blurred=False)
            assert _same_bits(ks[0, 0, j], k1[0, j]) and _same_bits(ss[0, j], sm[0, j])
            # every other joint saw nothing: NaN, in both sets
            others = [q for q in range(Jn) if q != j]
            assert np.isnan(kb[0, 0, others]).all() and np.isnan(kb[1, 0, [swap[q] for q in others]]).all() and np.isnan(sb[0, others]).all()
            assert _same_bits(kb[1, 0, swap[j]], [(np.float32(192.0) - kb[0, 0, j, 0]) - np.float32(1.0), kb[0, 0, j, 1]])
    # a joint the table fixes reads its own channel of the mirror; an exchanged one does NOT read its own
    z = np.zeros((2, H, W, Jn), dtype=np.float32)
    z[1, 2, 1, 0] = v                                                       # mirror frame, joint 0 (fixed), column 1 -> column W - 2
    z[1, 5, 2, 1] = v                                                       # mirror frame, joint 1 -> lands on joint 2, column W - 3
    k, s, _, _, f = _pair(z, "fp32", Jn, swap, blurred=False)
    assert f[0, 0, 2, W - 2] == v / 2 and f[0, 2, 5, W - 3] == v / 2 and np.count_nonzero(f) == 2
    assert _same_bits(k[0, 0, 0], [np.float32(4.0 * (W - 2) + 2.0), np.float32(4.0 * 1.75 + 2.0)])
    assert _same_bits(k[0, 0, 2], [np.float32(4.0 * (W - 3) + 2.0), np.float32(4.0 * 4.75 + 2.0)]) and np.isnan(k[0, 0, 1]).all()


# ---- 5. degenerate maps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_degenerate_maps_touch_their_own_joint_only(dtype):
    B, H, W, C = 3, 16, 12, 20
    swap = capf.H36M_SWAP
    base = O.make_maps(2 * B, H, W, C, J, 78, dtype)
    A = _affines(B, 6)
    k0, s0, q0, D0, f0 = _pair(base, dtype, J, swap, DEC, A)
    assert np.isfinite(k0).all() and np.isfinite(s0).all() and np.isfinite(q0).all()

    def poisoned(b, j, how):
        m = base.copy()
        if how == "cancel":                      # zo = -zm everywhere: the fused map is all zeros, its maximum 0
            m[B + b, :, :, swap[j]] = -m[b, :, ::-1, j]
        elif how == "overflow":                  # two finite values whose fp32 sum is not
            m[b, H // 2, W // 3, j] = m[B + b, H // 2, W - 1 - W // 3, swap[j]] = np.float32(3e38)
        elif how[0] == "mirror":
            m[B + b, H // 2, W // 3, swap[j]] = how[1]
        else:
            m[b, H // 2, W // 3, j] = how[1]
        return m

    cases = [(1, 5, "cancel"), (0, 0, ("mirror", np.nan)), (2, 16, ("mirror", np.inf)), (1, 12, ("mirror", -np.inf)), (2, 2, ("source", np.nan)),
             (0, 11, ("source", np.inf))] + ([(1, 3, "overflow")] if dtype == "fp32" else [])
    for b, j, how in cases:
        k, s, q, D, f = _pair(poisoned(b, j, how), dtype, J, swap, DEC, A)
        assert np.isnan(k[0, b, j]).all() and np.isnan(q[0, b, j]).all() and np.isnan(s[b, j]) and np.isnan(D[b, j]).all(), (b, j, how)
        assert np.isnan(k[1, b, swap[j]]).all() and np.isnan(q[1, b, swap[j]]).all(), (b, j, how)
        if how == "cancel":
            assert (f[b, j] == 0).all()
        keep = np.ones((2, B, J), dtype=bool)
        keep[0, b, j] = keep[1, b, swap[j]] = False
        assert _same_bits(k[keep], k0[keep]) and _same_bits(q[keep], q0[keep]) and _same_bits(s[keep[0]], s0[keep[0]]), (b, j, how)
        assert np.array_equal(D[keep[0]], D0[keep[0]]) and _same_bits(f[keep[0]], f0[keep[0]])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_negative_fused_maximum_follows_the_arithmetic(dtype):
    g = _taps()
    B, H, W = 2, 16, 12
    swap = capf.H36M_SWAP
    z2 = O.round_to(-np.abs(O.make_maps(2 * B, H, W, J, J, 32)) - np.float32(1.0), dtype)
    kcrop2, score, _, _, fused = _pair(z2, dtype, J, swap)
    zf = F.fold(z2, swap)
    k1, s1, _, _ = _single(zf, J, DEC, blurred=False)
    assert (zf.max(axis=(1, 2)) < 0).all() and _same_bits(kcrop2[0], k1) and _same_bits(score, s1) and np.isfinite(kcrop2).all()
    n = 0
    for b in range(B):
        for j in range(J):
            r = O.decode(zf[b, :, :, j], DEC, None, g)
            assert not r["degenerate"]
            if r["decided"]:
                n += 1
                assert _same_bits(kcrop2[0, b, j], r["kcrop"]) and _same_bits(score[b, j], r["score"]), (b, j, r["peaks"])
    assert n >= 0.9 * B * J


# ---- 6. a pair's bits depend on its two frames alone --------------------------------------------------------------------------------------------
def test_result_does_not_depend_on_the_batch_the_position_or_the_channel_count():
    H, W = 64, 48
    swap = capf.H36M_SWAP
    A1 = _affines(1, 9)
    pair = O.make_maps(2, H, W, 32, J, 13, "bf16")                           # one source frame and its "mirror", 32 channels
    others = O.make_maps(4, H, W, 32, J, 14, "bf16")
    want = None
    for C in (17, 20, 32):
        alone = np.ascontiguousarray(pair[:, :, :, :C])
        got = _pair(alone, "bf16", J, swap, DEC, A1)
        if want is None:
            want = got
        assert all(_same_bits(x, y) if x.dtype == np.float32 else _same_bits64(x, y) for x, y in zip(got, want)), C
        for pos in range(3):
            src = [others[0, :, :, :C], others[1, :, :, :C]]
            mir = [others[2, :, :, :C], others[3, :, :, :C]]
            src.insert(pos, alone[0])
            mir.insert(pos, alone[1])
            A = np.repeat(_affines(1, 10), 3, axis=0)
            A[pos] = A1[0]
            k, s, q, D, f = _pair(np.ascontiguousarray(np.stack(src + mir)), "bf16", J, swap, DEC, A)
            assert _same_bits(k[:, pos], want[0][:, 0]) and _same_bits(s[pos], want[1][0]) and _same_bits(q[:, pos], want[2][:, 0]), (C, pos)
            assert _same_bits64(D[pos], want[3][0]) and _same_bits(f[pos], want[4][0]), (C, pos)


# ---- 7. the module --------------------------------------------------------------------------------------------------------------------------------
def _model(dtype, wseed=3):
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), "cpn")
    cfg.model.backbone.fix_weights = True
    with contextlib.redirect_stdout(io.StringIO()):
        m = CA_PF(cfg, compute_dtype=dtype, keypoint_head="cpn").eval()
    synth.load_synthetic(m, seed=wseed, bn_mode="random")
    return m.cuda()


def _release(*models):
    for m in models:
        for e in m._engines.values():
            e.close()
        m._engines.clear()


def _inputs(B, H, W, seed=9, u8=False):
    gen = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (B, H, W, 3), generator=gen, dtype=torch.uint8) if u8 else torch.randn(B, H, W, 3, generator=gen)
    A = torch.from_numpy(np.stack([capf.crop_to_image_matrix((480.0 + 20 * b, 510.0 - 10 * b), (1.2 + 0.1 * b, 1.6 + 0.1 * b), (W, H), 1000, 1002)
                                   for b in range(B)]).astype(np.float32))
    return images.cuda(), A.cuda()


@pytest.mark.parametrize("dtype,u8,H,W", [("fp32", False, 256, 192), ("bf16", True, 256, 192), ("bf16", False, 384, 288)],
                         ids=["fp32-float-256x192", "bf16-u8-256x192", "bf16-float-384x288"])
def test_module_detect_cpn_flip_and_forward_detect_cpn_flip(dtype, u8, H, W):
    B = 3
    m, fresh = _model(dtype), _model(dtype)
    try:
        images, A = _inputs(B, H, W, u8=u8)
        kcrop, score, k2d = m.detect_cpn_flip(images, A)          # (grad mode is on: the entry runs without it all the same)
        assert kcrop.shape == (B, J, 2) and score.shape == (B, J) and k2d.shape == (B, J, 2)
        assert not (kcrop.requires_grad or score.requires_grad or k2d.requires_grad)
        assert torch.isfinite(kcrop).all() and torch.isfinite(score).all() and torch.isfinite(k2d).all()
        assert (kcrop[..., 0] >= 0).all() and (kcrop[..., 0] <= W).all() and (kcrop[..., 1] >= 0).all() and (kcrop[..., 1] <= H).all()
        # detect_cpn_flip is capf_cpn_decode_pair on the heatmaps of the 2B frames the pass left, with CPN's cell-centre convention
        eng = m._engine_at(images.device, H, W)
        heat = eng.tensor_view("heat", 2 * B)
        assert heat.shape == (2 * B, 64, 48, 20) and heat.dtype == TORCH[dtype]
        sx, sy = W / 48.0, H / 64.0
        kc2, sc, kd2, _, _ = capf.cpn_decode_pair(heat, J, None, (sx, sx / 2, sy, sy / 2), A, 192.0)
        assert torch.equal(kc2[0], kcrop) and torch.equal(sc, score) and torch.equal(kd2[0], k2d)
        k_only, s_only, none = m.detect_cpn_flip(images)
        assert none is None and torch.equal(k_only, kcrop) and torch.equal(s_only, score)
        # the flip reaches the result: the plain detect() of the same crops differs somewhere
        assert not torch.equal(m.detect(images, A)[0], kcrop)
        # forward_detect_cpn_flip == forward_flip_test on detect_cpn_flip's keypoints through preprocess_points(mode = 2)
        out, kc_px, sc2 = m.forward_detect_cpn_flip(images, A)
        assert out.shape == (B, 1, J, 3) and not out.requires_grad and torch.isfinite(out).all()
        assert torch.equal(kc_px, kcrop) and torch.equal(sc2, score)                              # still pixels: the lifter normalised a copy
        _, k2d2, kcrop2 = capf.preprocess_points(None, k2d, kcrop, mode=2)
        assert torch.equal(k2d2, kd2) and torch.equal(kcrop2, kc2)
        with torch.no_grad():
            if u8:
                pred = m.forward_u8(images, k2d2.view(2 * B, J, 2), kcrop2.clone().view(2 * B, J, 2), mirror="pair")
                want = capf.fliptest_fuse(pred.view(2, B, 1, J, 3))
            else:
                want = m.forward_flip_test(torch.stack([images, torch.flip(images, [2])]), k2d2, kcrop2.clone())
        assert torch.equal(out, want)
        # a second call on the reused engine has a fresh engine's bits
        again, first = m.forward_detect_cpn_flip(images, A), fresh.forward_detect_cpn_flip(images, A)
        assert all(torch.equal(x, y) for x, y in zip(again, first)) and torch.equal(again[0], out)
        # the H36M table by name: the default's bits; the COCO table is accepted and changes the result
        named = m.forward_detect_cpn_flip(images, A, flip_pairs=capf.H36M_SWAP)
        assert all(torch.equal(x, y) for x, y in zip(named, (out, kcrop, score)))
        coco = m.forward_detect_cpn_flip(images, A, flip_pairs=capf.COCO_SWAP)
        assert torch.isfinite(coco[0]).all() and not torch.equal(coco[1], kcrop) and not torch.equal(coco[0], out)
        assert torch.equal(m.detect_cpn_flip(images, A, flip_pairs=capf.COCO_SWAP)[0], coco[1])
        if u8:       # the uint8 crops, their normalised float image and the [2,B,H,W,3] stack: the same bits
            imgf = capf.preprocess(images, None, k2d, kcrop.clone(), "cpn", 0)[0]
            stack = capf.preprocess(images, None, k2d, kcrop.clone(), "cpn", 2)[0]
            assert imgf.shape == (B, H, W, 3) and stack.shape == (2, B, H, W, 3)
            for form in (imgf, stack):
                assert all(torch.equal(x, y) for x, y in zip(m.detect_cpn_flip(form, A), (kcrop, score, k2d)))
                assert all(torch.equal(x, y) for x, y in zip(m.forward_detect_cpn_flip(form, A), (out, kcrop, score)))
        # HRNet's entries keep refusing this head
        for entry in (m.detect_flip_test, m.forward_detect_flip_test):
            with pytest.raises(NotImplementedError, match="flip"):
                entry(images, A)
        # a final_predict parameter that requires grad raises under grad, and not without
        next(m.backbone.refine_net.final_predict.parameters()).requires_grad_(True)
        with pytest.raises(NotImplementedError, match="final_predict"):
            m.forward_detect_cpn_flip(images, A)
        with pytest.raises(NotImplementedError, match="final_predict"):
            m.detect_cpn_flip(images, A)
        with torch.no_grad():
            assert torch.equal(m.detect_cpn_flip(images, A)[0], kcrop)
    finally:
        _release(m, fresh)
