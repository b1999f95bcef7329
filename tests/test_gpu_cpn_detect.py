"""GPU: CPN's own keypoint detector -- capf_cpn_decode against tests/cpn_decode_oracle.py, its tie and edge rules, the head's ops under
CAPF_PLAN_CPN_PREDICT held to the layer-wise bound on both sides of their routing thresholds, everything else unmoved by the flag, and
CA_PF(keypoint_head="cpn").detect / forward_detect.

What is equal is asserted equal: the decode's float32 outputs against the oracle's wherever the peaks are DECIDED (cpn_decode_oracle: both
gaps above 4 gamma), bit for bit; the blurred plane within gamma = 44 x 2^-53 x blur(|P|) of the oracle's (fma against multiply-then-add, two
passes of 21 taps); the head's convs within op_oracle.compare's per-op bound of the oracle on the engine's own operands.  Undecided cases are
left out and counted: at most 2 % of all (frame, joint) cases outside the 1 x 1 maps, every case of which is an exact four-way tie (n = 1,
D = g (x) g: tests/test_cpn_detect.py) and is held to equality like a decided one."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import cpn_decode_oracle as O
import op_oracle
import workspace_guard as wg
from capf import lib as capf
from capf import synth
from capf.lib import PLAN_CPN_PREDICT

pytestmark = pytest.mark.gpu
J = 17
FP = "backbone.refine_net.final_predict"
BNECK = [FP + ".0.conv1", FP + ".0.conv2", FP + ".0.downsample.0", FP + ".0.conv3"]
TORCH = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _taps():
    return np.array(capf.cpn_decode_taps())


def _affines(B, seed):
    rng = np.random.default_rng(seed)
    A = rng.uniform(-1.0, 1.0, (B, 2, 3)).astype(np.float32)
    A[:, :, :2] *= np.float32(0.01)
    return A


def _decode(maps, dtype, Jn, dec, A=None, blurred=True):
    """capf_cpn_decode on host maps [B, H, W, C] float32 (exact in `dtype`): numpy (kcrop, score, k2d | None, blurred | None)"""
    heat = torch.from_numpy(maps).to(TORCH[dtype]).cuda().contiguous()
    a = None if A is None else torch.from_numpy(A).cuda()
    kcrop, score, k2d, D = capf.cpn_decode(heat, Jn, dec, a, want_score=True, want_blurred=blurred)
    torch.cuda.synchronize()
    return kcrop.cpu().numpy(), score.cpu().numpy(), None if k2d is None else k2d.cpu().numpy(), None if D is None else D.cpu().numpy()


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, dtype=np.float32).view(np.int32), np.asarray(b, dtype=np.float32).view(np.int32))


# ---- 1. the decode against the oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_decode_matches_the_oracle(dtype):
    g = _taps()
    undecided = counted = checked = 0
    worst_blur = 0.0
    for si, (H, W) in enumerate(O.SHAPES):
        dec = (4.0, 2.0, 4.0, 2.0) if si % 2 == 0 else (6.0, 3.0, 6.0, 3.0)          # CPN's convention at 256 x 192 / 384 x 288 crops
        for ji, (Jn, C) in enumerate(O.JC):
            for B in O.BATCHES:
                seed = 1000 * si + 10 * ji + B
                maps = O.make_maps(B, H, W, C, Jn, seed, dtype)
                A = _affines(B, seed)
                kcrop, score, k2d, D = _decode(maps, dtype, Jn, dec, A)
                assert kcrop.shape == (B, Jn, 2) and score.shape == (B, Jn) and k2d.shape == (B, Jn, 2) and D.shape == (B, Jn, H + 20, W + 20)
                for b in range(B):
                    for j in range(Jn):
                        r = O.decode(maps[b, :, :, j], dec, A[b], g)
                        assert not r["degenerate"]
                        P = np.zeros_like(r["D"])
                        P[10:10 + H, 10:10 + W] = np.abs(maps[b, :, :, j] / maps[b, :, :, j].max())
                        gamma = 44 * O.U * O.blur(P, g)
                        ratio = float((np.abs(D[b, j] - r["D"]) / np.maximum(gamma, 1e-300)).max())
                        worst_blur = max(worst_blur, ratio)
                        assert ratio <= 1.0, (H, W, Jn, C, B, b, j, ratio)
                        tie_by_construction = (H, W) == (1, 1)
                        if not tie_by_construction:
                            counted += 1
                            undecided += not r["decided"]
                        if r["decided"] or tie_by_construction:
                            checked += 1
                            what = (H, W, Jn, C, B, b, j, r["peaks"], r["gap1"], r["gap2"])
                            assert _same_bits(kcrop[b, j], r["kcrop"]), ("kcrop", kcrop[b, j], r["kcrop"], what)
                            assert _same_bits(k2d[b, j], r["k2d"]), ("k2d", k2d[b, j], r["k2d"], what)
                            assert _same_bits(score[b, j], r["score"]), ("score", score[b, j], r["score"], what)
                            assert 0 <= (kcrop[b, j, 0] - dec[1]) / dec[0] <= W - 1 and 0 <= (kcrop[b, j, 1] - dec[3]) / dec[2] <= H - 1
    print(f"{dtype}: {checked} (frame, joint) cases equal to the oracle, {undecided} of {counted} undecided and left out; "
          f"worst |blurred - oracle| = {worst_blur:.3f} gamma")
    assert undecided <= 0.02 * counted, (undecided, counted)


# ---- 2. tie and edge rules, exact ----------------------------------------------------------------------------------------------------------
def _single_pixel(H, W, y, x, value=3.0, C=1):
    m = np.zeros((1, H, W, C), dtype=np.float32)
    m[0, y, x, 0] = value
    return m


def test_single_pixel_ties_go_to_the_first_neighbour():
    """One non-zero pixel: D = g (x) g scaled by n = 1; its four neighbours tie bit for bit (symmetric taps, every other term an exact zero),
    the first in row-major order is (y1 - 1, x1), so the keypoint is (x1, y1 - 0.25)."""
    g = _taps()
    H, W, dec = 9, 7, (4.0, 2.0, 4.0, 2.0)
    for (y, x) in [(4, 3), (1, 1), (7, 5), (3, 4)]:                      # interior cells
        maps = _single_pixel(H, W, y, x)
        kcrop, score, _, D = _decode(maps, "fp32", 1, dec)
        want = np.zeros((H + 20, W + 20))
        want[y:y + 21, x:x + 21] = np.outer(g, g)                        # (rounded products of two taps: what one fma onto +0 gives)
        assert np.array_equal(D[0, 0], want)
        c = D[0, 0]
        py, px = y + 10, x + 10
        assert c[py - 1, px] == c[py + 1, px] == c[py, px - 1] == c[py, px + 1] < c[py, px] == c.max()
        assert _same_bits(kcrop[0, 0], [np.float32(4.0 * x + 2.0), np.float32(4.0) * np.float32(y - 0.25) + np.float32(2.0)])
        assert _same_bits(score[0, 0], np.float32(3.0) / np.float32(255) + np.float32(0.5))
        r = O.decode(maps[0, :, :, 0], dec, None, g)
        assert r["peaks"] == ((py, px), (py - 1, px)) and _same_bits(kcrop[0, 0], r["kcrop"])


def test_single_pixel_at_corners_and_edges_is_clamped():
    g = _taps()
    H, W, dec = 6, 5, (4.0, 2.0, 4.0, 2.0)
    cells = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, 2), (H - 1, 2), (3, 0), (3, W - 1)]
    for (y, x) in cells:
        maps = _single_pixel(H, W, y, x, value=0.5)
        for dtype in ("fp32", "bf16"):
            kcrop, score, _, D = _decode(maps, dtype, 1, dec)
            r = O.decode(maps[0, :, :, 0], dec, None, g)
            hx, hy = (kcrop[0, 0, 0] - 2.0) / 4.0, (kcrop[0, 0, 1] - 2.0) / 4.0
            assert 0.0 <= hx <= W - 1 and 0.0 <= hy <= H - 1
            assert hx == x and hy == max(0.0, y - 0.25), (y, x, hx, hy)   # the tie goes up; row 0 is clamped back
            assert r["peaks"] == ((y + 10, x + 10), (y + 9, x + 10))
            assert _same_bits(kcrop[0, 0], r["kcrop"]) and _same_bits(score[0, 0], r["score"])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_degenerate_maps_touch_their_own_joint_only(dtype):
    """an all-zero map, a NaN, an Inf: NaN for that (frame, joint) -- keypoint in both coordinate systems, score, its blurred plane -- and
    every other joint and frame bit-identical to a run without it"""
    B, H, W, C, dec = 3, 16, 12, 20, (4.0, 2.0, 4.0, 2.0)
    base = O.make_maps(B, H, W, C, J, 77, dtype)
    A = _affines(B, 5)
    k0, s0, q0, D0 = _decode(base, dtype, J, dec, A)
    assert np.isfinite(k0).all() and np.isfinite(s0).all() and np.isfinite(q0).all()

    def poisoned(b, j, how):
        m = base.copy()
        if how == "zero":
            m[b, :, :, j] = 0.0
        else:
            m[b, H // 2, W // 3, j] = how
        return m

    for b, j, how in [(1, 5, "zero"), (0, 0, np.nan), (2, 16, np.inf), (1, 9, -np.inf)]:
        k, s, q, D = _decode(poisoned(b, j, how), dtype, J, dec, A)
        assert np.isnan(k[b, j]).all() and np.isnan(q[b, j]).all() and np.isnan(s[b, j]) and np.isnan(D[b, j]).all()
        keep = np.ones((B, J), dtype=bool)
        keep[b, j] = False
        assert _same_bits(k[keep], k0[keep]) and _same_bits(q[keep], q0[keep]) and _same_bits(s[keep], s0[keep])
        assert np.array_equal(D[keep], D0[keep])


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_negative_maximum_follows_the_arithmetic(dtype):
    g = _taps()
    B, H, W, dec = 2, 16, 12, (4.0, 2.0, 4.0, 2.0)
    maps = O.round_to(-np.abs(O.make_maps(B, H, W, J, J, 31)) - np.float32(1.0), dtype)
    kcrop, score, _, D = _decode(maps, dtype, J, dec)
    n = 0
    for b in range(B):
        for j in range(J):
            r = O.decode(maps[b, :, :, j], dec, None, g)
            assert maps[b, :, :, j].max() < 0 and not r["degenerate"]
            if r["decided"]:
                n += 1
                assert _same_bits(kcrop[b, j], r["kcrop"]) and _same_bits(score[b, j], r["score"]), (b, j, r["peaks"])
    assert n >= 0.9 * B * J


def test_result_does_not_depend_on_the_position_in_the_batch():
    H, W, dec = 64, 48, (4.0, 2.0, 4.0, 2.0)
    maps = O.make_maps(3, H, W, 20, J, 12, "bf16")
    k, s, _, D = _decode(maps, "bf16", J, dec)
    alone = np.ascontiguousarray(maps[2:3, :, :, 4:5])
    k1, s1, _, D1 = _decode(alone, "bf16", 1, dec)
    assert _same_bits(k1[0, 0], k[2, 4]) and _same_bits(s1[0, 0], s[2, 4]) and np.array_equal(D1[0, 0], D[2, 4])


# ---- 3. the head's ops ----------------------------------------------------------------------------------------------------------------------
def _model(dtype, wseed=71, flags=PLAN_CPN_PREDICT, head=None):
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), "cpn")
    cfg.model.backbone.fix_weights = True
    with contextlib.redirect_stdout(io.StringIO()):
        m = CA_PF(cfg, compute_dtype=dtype, plan_flags=flags, keypoint_head=head).eval()
    sd = synth.load_synthetic(m, seed=wseed, bn_mode="random")
    return m.cuda(), sd


def _release(*models):
    for m in models:
        for e in m._engines.values():
            e.close()
        m._engines.clear()


def _family(kernel):
    return kernel.split("<")[0]


# batches on both sides of every routing threshold the four convs cross: fp32 5 (the two-fp16-piece GEMM and, for conv2, the split-fp32 tile
# from batch 5), bf16 24 (conv2 on the 2-D halo tile from 1 GFLOP per conv and batch 24); the head's maps are 64 x 48 at every crop size
SIDES = {"fp32": (2, 6), "bf16": (2, 24)}
HEAD_CASES = [(dtype, B, H, W) for dtype in ("fp32", "bf16") for B in SIDES[dtype] for (H, W) in ((32, 32), (256, 192))]


@pytest.mark.parametrize("dtype,B,H,W", HEAD_CASES, ids=[f"{d}-B{b}-{h}x{w}" for d, b, h, w in HEAD_CASES])
def test_bottleneck_convs_layerwise(dtype, B, H, W):
    from test_gpu_layerwise import layerwise
    kernels = layerwise("cpn", dtype, B, H, W, [0, B - 1], plan_flags=PLAN_CPN_PREDICT, only=set(BNECK))
    assert set(layerwise.kernel_of) == set(BNECK)
    # this batch and its partner lie on different sides of a threshold: together they run at least two kernel families
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), "cpn")
    plan = capf.Engine(_native.make_capf_config(cfg, H, W, compute_dtype=dtype, plan_flags=PLAN_CPN_PREDICT), device=None)
    other = [b for b in SIDES[dtype] if b != B][0]
    here = {n: _family(k) for n, k, _ in plan.op_table(B) if n in BNECK}
    there = {n: _family(k) for n, k, _ in plan.op_table(other) if n in BNECK}
    assert here == {n: _family(k) for n, k in layerwise.kernel_of.items()}          # what ran is what the plan names
    assert len(set(here.values()) | set(there.values())) >= 2 and here != there, (here, there)
    assert {_family(k) for k in kernels} == set(here.values())


@pytest.mark.parametrize("dtype,B", [("fp32", 2), ("fp32", 6), ("bf16", 2), ("bf16", 24)])
def test_concat_and_last_conv(dtype, B):
    H, W = 64, 96
    model, sd = _model(dtype)
    try:
        img = synth.synth_inputs(B, H, W, seed=72, crop_range=(W, H))[0].cuda()
        eng = model.engine_for(img)
        table = eng.op_table(B)
        names = [n for n, _, _ in eng.schema()]
        index = {n: i for i, (n, _, _) in enumerate(table) if "final_predict" in n}
        stream = torch.cuda.current_stream().cuda_stream
        dt = 2 if dtype == "bf16" else 0
        # the concatenation, read as conv1's operand behind the Bottleneck's join: torch.cat of feat0..3, exactly
        d1 = eng.op_describe(index[BNECK[0]])
        eng.forward_prefix(img, d1.checkpoint, stream)
        torch.cuda.synchronize()
        cat = eng.op_tensor(index[BNECK[0]], 0, (B, 64, 48, 1024), dt).clone()
        feats = [eng.tensor(f"feat{l}") for l in range(4)]
        assert all(f.shape == (B, 64, 48, 256) for f in feats)
        assert torch.equal(cat.view(torch.int16 if dt else torch.int32), torch.cat(feats, 3).view(torch.int16 if dt else torch.int32))
        # the last conv: 17 channels against the oracle on the engine's own operand, three exact zeros behind them
        i = index[FP + ".1"]
        d = eng.op_describe(i)
        assert (d.Cin, d.Cout, d.ks, d.stride, d.pad, d.act, d.has_residual) == (256, 20, 3, 1, 1, 0, 0)
        assert names[d.p_weight] == FP + ".1.weight" and names[d.p_bn_weight] == FP + ".2.weight"
        eng.forward_prefix(img, d.checkpoint, stream)
        torch.cuda.synchronize()
        x = eng.op_tensor(i, 0, (B, 64, 48, 256), d.in_dtype).cpu()
        got = eng.op_tensor(i, 5, (B, 64, 48, 20), d.out_dtype).cpu()
        heat = eng.tensor("heat").cpu()
        assert heat.dtype == TORCH[dtype] and torch.equal(heat.float(), got.float())
        with torch.no_grad():
            want, mass, term = op_oracle.conv_bn_act(sd, FP + ".1", FP + ".2", x, None, 3, 1, 1, 0, bool(d.mfma_bf16))
        r = op_oracle.compare(got[..., :17], want, d.out_dtype == 2, mass, term)
        print(f"{dtype} B={B} {table[i][1]}: last conv {r}")
        assert r["ok"] and r["weight_flips"] <= 4, r                   # (test_gpu_layerwise's rules: compare's bound, its allowance of flips)
        assert bool((got[..., 17:].float() == 0).all())
        assert want.abs().max() > 0.1                                   # (a live head: the comparison is not of zeros)
    finally:
        _release(model)


# ---- 4. nothing else moved --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_flag_leaves_maps_and_joints_alone(dtype):
    B, H, W = 2, 256, 192
    plain, _ = _model(dtype, flags=0)
    flagged, _ = _model(dtype)
    try:
        img, k2d, kc = (t.cuda() for t in synth.synth_inputs(B, H, W, seed=12, crop_range=(W, H)))
        with torch.no_grad():
            a = plain(img, k2d, kc.clone())
            b = flagged(img, k2d, kc.clone())
        assert torch.isfinite(a).all() and torch.equal(a, b)
        ea, eb = plain.engine_for(img), flagged.engine_for(img)
        for l in range(4):
            fa, fb = ea.tensor(f"feat{l}"), eb.tensor(f"feat{l}")
            assert fa.dtype == fb.dtype and torch.equal(fa, fb)
        assert torch.isfinite(eb.tensor("heat").float()).all()
        assert eb.workspace_bytes(B) > ea.workspace_bytes(B)
    finally:
        _release(plain, flagged)


# ---- 5. the module -----------------------------------------------------------------------------------------------------------------------------
def _inputs(B, H, W, seed=9, u8=False):
    gen = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (B, H, W, 3), generator=gen, dtype=torch.uint8) if u8 else torch.randn(B, H, W, 3, generator=gen)
    A = torch.from_numpy(np.stack([capf.crop_to_image_matrix((480.0 + 20 * b, 510.0 - 10 * b), (1.2 + 0.1 * b, 1.6 + 0.1 * b), (W, H), 1000, 1002)
                                   for b in range(B)]).astype(np.float32))
    return images.cuda(), A.cuda()


@pytest.mark.parametrize("dtype,u8,H,W", [("fp32", False, 256, 192), ("bf16", True, 256, 192), ("bf16", False, 384, 288)],
                         ids=["fp32-float-256x192", "bf16-u8-256x192", "bf16-float-384x288"])
def test_module_detect_and_forward_detect(dtype, u8, H, W):
    B = 3
    m, _ = _model(dtype, wseed=3, flags=0, head="cpn")
    fresh, _ = _model(dtype, wseed=3, flags=0, head="cpn")
    try:
        images, A = _inputs(B, H, W, u8=u8)
        with torch.no_grad():
            kcrop, score, k2d = m.detect(images, A)
            assert kcrop.shape == (B, J, 2) and score.shape == (B, J) and k2d.shape == (B, J, 2)
            assert torch.isfinite(kcrop).all() and torch.isfinite(score).all() and torch.isfinite(k2d).all()
            assert (kcrop[..., 0] >= 0).all() and (kcrop[..., 0] <= W).all() and (kcrop[..., 1] >= 0).all() and (kcrop[..., 1] <= H).all()
            # detect() is capf_cpn_decode on the heatmaps the backbone pass left, with CPN's cell-centre convention
            eng = m._engine_at(images.device, H, W)
            heat = eng.tensor_view("heat", B)
            assert heat.shape == (B, 64, 48, 20) and heat.dtype == TORCH[dtype] and bool((heat[..., 17:] == 0).all())
            sx, sy = W / 48.0, H / 64.0
            k_d, s_d, q_d, _ = capf.cpn_decode(heat, J, (sx, sx / 2, sy, sy / 2), A)
            assert torch.equal(k_d, kcrop) and torch.equal(s_d, score) and torch.equal(q_d, k2d)
            k_only, s_only, none = m.detect(images)
            assert none is None and torch.equal(k_only, kcrop) and torch.equal(s_only, score)
            # forward_detect == forward on detect's keypoints; kcrop stays in pixels
            out, kc2, sc2 = m.forward_detect(images, A)
            assert torch.equal(kc2, kcrop) and torch.equal(sc2, score)
            fwd = m.forward_u8 if u8 else m.forward
            want = fwd(images, k2d, kcrop.clone())
            assert out.shape == (B, 1, J, 3) and torch.isfinite(out).all() and torch.equal(out, want)
            # a second forward_detect on the reused engine has a fresh engine's bits
            again = m.forward_detect(images, A)
            first = fresh.forward_detect(images, A)
            for x, y in zip(again, first):
                assert torch.equal(x, y)
            assert torch.equal(again[0], out)
            if u8:       # the uint8 crops and their normalised float image: the same keypoints, bit for bit
                imgf = capf.preprocess(images, None, k2d, kcrop.clone(), "cpn", 0)[0]
                kf, sf, k2f = m.detect(imgf, A)
                assert torch.equal(kf, kcrop) and torch.equal(sf, score) and torch.equal(k2f, k2d)
            for entry, args in ((m.detect_flip_test, (images, A)), (m.forward_detect_flip_test, (images, A))):
                with pytest.raises(NotImplementedError):
                    entry(*args)
    finally:
        _release(m, fresh)


def test_module_lifter_trains_under_forward_detect():
    """the head has no derivative; the lifter trains as in forward(): same loss, same gradients as forward on detect's keypoints"""
    B, H, W = 2, 256, 192
    m, _ = _model("fp32", wseed=3, flags=0, head="cpn")
    try:
        m.train(); m.backbone.eval()
        m.drop_path_rate = 0.0
        images, A = _inputs(B, H, W)
        gt = 0.3 * torch.randn(B, 1, J, 3, generator=torch.Generator().manual_seed(4)).cuda()
        out, kcrop, _ = m.forward_detect(images, A)
        assert out.requires_grad and not kcrop.requires_grad
        (out - gt).pow(2).mean().backward()
        grads = {n: p.grad.clone() for n, p in m.volume_net.named_parameters()}
        assert all(torch.isfinite(g).all() for g in grads.values()) and any(bool(g.abs().max() > 0) for g in grads.values())
        m.zero_grad(set_to_none=True)
        with torch.no_grad():
            _, _, k2d = m.detect(images, A)
        out2 = m(images, k2d, kcrop.clone())
        assert torch.equal(out2, out)
        (out2 - gt).pow(2).mean().backward()
        for n, p in m.volume_net.named_parameters():
            assert torch.equal(p.grad, grads[n]), n
        assert all(p.grad is None for p in m.backbone.parameters())
    finally:
        _release(m)


# ---- 6. an exact-size, NaN-filled, banded workspace ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_flagged_plan_on_a_poisoned_workspace(dtype):
    """the flagged plan on a workspace of exactly capf_workspace_bytes(B) bytes between guard bands, every byte 0xFF (NaN in fp32 and bf16):
    a finite heat, the same bits as on a zero-filled one, bands intact (tests/workspace_guard.py)"""
    from mvn.models import _native
    B, H, W = 3, 64, 96
    model, _ = _model(dtype)
    eng = None
    try:
        cfg = _native.make_capf_config(model._config, H, W, context_blocks=model.context_blocks, compute_dtype=dtype, plan_flags=model.plan_flags)
        cfg.training = 0          # (the arena ends at the band: tests/test_gpu_workspace_hygiene.py _inference_engine)
        stream = torch.cuda.current_stream().cuda_stream
        eng = capf.Engine(cfg, device=torch.cuda.current_device())
        eng.bind_state({k: v.data for k, v in model.state_dict(keep_vars=True).items()}, stream)
        img = synth.synth_inputs(B, H, W, seed=22, crop_range=(W, H))[0]
        ws = wg.install(eng, B, 0x00)
        heats = []
        for fill in (0x00, 0xFF):
            ws.refill(fill)
            x = wg.flush(img.cuda(), fill)
            eng.backbone_forward(x, stream)
            ws.check(f"workspace under fill 0x{fill:02X}")
            wg.check_all((x,), "images")
            heats.append(eng.tensor("heat"))
        assert torch.isfinite(heats[1].float()).all() and torch.equal(heats[0], heats[1])
        assert bool((heats[1][..., 17:] == 0).all()) and bool(heats[1][..., :17].float().abs().max() > 0)
    finally:
        if eng is not None:
            eng.close()
        _release(model)
