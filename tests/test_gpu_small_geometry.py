"""GPU: the small-map and odd-geometry plans of tests/small_geometry_cases.py, executed and held to the oracle with the suite's existing
walkers and bounds (no tolerance of its own).

The stand-alone op tests reach tiny maps as single launches on buffers of their own; what they cannot see is what goes wrong BETWEEN ops at
these sizes: a grouped launch whose list mixes kernel families (an F(4,3) group, a lone F(2,3) conv and two-piece GEMMs in one level), the
per-geometry unit tables, workspace offsets, the planner handing a kernel a shape its own test should have refused, a 256-pixel tile that
spans 64 frames of a 2 x 2 branch and ends ragged, samplers on a 1 x 1 map (size - 1 = 0 under the align_corners rule).

* backbone, op by op:  test_gpu_layerwise.layerwise (16-bit: under f16_report / the fp32-stream walker) for every row of the table;
* lifter, op by op:    test_gpu_lifter_ops.lifter_ops (fp32, float64 restatements; both samplers' cells == ATen's rule bit for bit) and
                       test_gpu_layerwise.lifter_layerwise (16-bit) on the 1 x 1, 1 x 2, 5 x 3 and CPN top maps, crop keypoints drawn
                       over the actual crop plus one adversarial frame;
* end to end:          fp32 rows against capf_oracle.ca_pf_forward at test_gpu_parity.TOL_OUT, 16-bit rows by bf16_report's rules;
* schedules:           capf_set_lanes 0 / 2 / 3 bit-identical on the levels whose grouped lists mix families;
* training:            HRNet-32 32 x 64 (maps 8 x 16 .. 1 x 2) against float64 in both map-gradient modes, the ordered one twice."""
import contextlib

import numpy as np
import pytest
import torch

import capf_oracle as oracle
import small_geometry_cases as sg
import test_gpu_layerwise as lw
from bf16_report import bf16_stage_report, check_bf16_report
from capf import synth
from f16_report import fp16_emulation, layerwise_in_fp16
from test_gpu_fullsize import _model
from test_gpu_parity import TOL_OUT

pytestmark = pytest.mark.gpu

ROW_IDS = [sg.row_id(r) for r in sg.ROWS]


def _kcrop(B, H, W, seed):
    """crop keypoints over the actual crop, the last frame adversarial (on / next to cell edges of every map, on and beyond +-1)"""
    kc = synth.synth_inputs(B, H, W, seed=seed, crop_range=(W, H))[2].clone()
    kc[B - 1] = synth.adversarial_crop_keypoints(1, seed=seed + 1)[0]
    return kc


# ---- backbone, op by op ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", sg.ROWS, ids=ROW_IDS)
def test_backbone_op_by_op(row):
    frames, flags = list(row.frames_to_check), sg.flag_bits(row.plan_flags)
    if row.plan_flags == "BF16_F32_STREAM":
        from test_gpu_bf16_f32_stream import stream_layerwise
        k = stream_layerwise(row.backbone, row.batch, frames, H=row.H, W=row.W)
    else:
        with (layerwise_in_fp16() if row.dtype == "fp16" else contextlib.nullcontext()):
            k = lw.layerwise(row.backbone, row.dtype, row.batch, row.H, row.W, frames, plan_flags=flags)
        if row.backbone == "cpn" and (1, 1) in sg.branch_maps(row.H, row.W):
            assert any((h, w) == (1, 1) and ho > 2 * h for h, w, ho, wo in lw.layerwise.resizes), lw.layerwise.resizes
    assert sg.prefixes_hold(k, row.expected_kernel_prefixes) == [], sorted(k)


# ---- lifter, op by op --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone,H,W,B", sg.LIFTER_FP32, ids=[f"{c[0]}-{c[1]}x{c[2]}-B{c[3]}" for c in sg.LIFTER_FP32])
def test_lifter_op_by_op_fp32(backbone, H, W, B):
    """every lifter op in float64 from the engine's own operands; idx{l} (zeros mode) and cidx{n} (border mode) are ATen's rule bit for bit
    on the 1 x 1, 1 x 2 and 5 x 3 maps (lifter_ops: check_idx, cells_and_positions)"""
    from lifter_models import lifter_model
    from test_gpu_lifter_ops import lifter_ops
    model, sd = lifter_model(backbone)
    lifter_ops(model, sd, B, H, W, kcrop=_kcrop(B, H, W, 84))
    assert {"embed", "ctx_attn", "mlp_chain", "res_chain", "head"} <= lifter_ops.kernels
    eng = model.engine_for(torch.empty(B, H, W, 3, device="cuda"))
    top = sg.branch_maps(H, W)[3] if backbone != "cpn" else None
    if top is not None:
        assert tuple(eng.tensor("feat3").shape[1:3]) == top


@pytest.mark.parametrize("backbone,H,W,B,dtype", sg.LIFTER_16BIT, ids=[f"{c[0]}-{c[1]}x{c[2]}-B{c[3]}-{c[4]}" for c in sg.LIFTER_16BIT])
def test_lifter_op_by_op_16bit(backbone, H, W, B, dtype):
    with (layerwise_in_fp16() if dtype == "fp16" else contextlib.nullcontext()):
        c = lw.lifter_layerwise(backbone, B, H, W, list(range(B)), kcrop=_kcrop(B, H, W, 85))
    assert c.get("qkv bf16") == 8 and c.get("proj bf16") == 8 and c.get("fc1+gelu bf16") == 12 and c.get("fc2 bf16") == 12
    assert c.get("layernorm") == 20 and c.get("attention") == 8


def _tiny_grid(H, W):
    from test_gpu_sampling import adversarial_grid
    with np.errstate(all="ignore"):                      # (a size of 1 has no pixel-centre spacing: k / (size - 1) is 0 / 0, dropped below)
        g = adversarial_grid(H, W)
    return np.ascontiguousarray(g[np.isfinite(g).all(axis=1)])


@pytest.mark.parametrize("H,W", [(1, 1), (1, 2), (2, 1), (5, 3)])
def test_corner_rule_on_the_tiny_top_maps(H, W):
    """test_gpu_sampling.test_corner_rule_on_adversarial_coordinates at the top-map sizes of the plans above: indices and fractional
    weights bit for bit in both padding modes (size - 1 = 0: every coordinate unnormalises to 0)"""
    from capf.lib import bilinear_corners
    grid = _tiny_grid(H, W)
    assert len(grid) > 8000
    dev = torch.from_numpy(grid).cuda()
    for mode in ("border", "zeros"):
        idx, frac = bilinear_corners(dev, H, W, border=(mode == "border"))
        want = oracle.bilinear_corners(grid, H, W, mode)
        np.testing.assert_array_equal(idx.cpu().numpy()[:, 0], want["ix0"])
        np.testing.assert_array_equal(idx.cpu().numpy()[:, 1], want["iy0"])
        np.testing.assert_array_equal(frac.cpu().numpy()[:, 0], want["wx1"])
        np.testing.assert_array_equal(frac.cpu().numpy()[:, 1], want["wy1"])


# ---- end to end --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", sg.ROWS, ids=ROW_IDS)
def test_end_to_end(row):
    """fp32: the joints of the checked frames against capf_oracle.ca_pf_forward on fresh inputs at TOL_OUT.  16-bit: H = the engine, E = the
    oracle with the engine's storage roundings, F = the fp32 oracle, stage by stage by bf16_report's rules
    (test_gpu_sampling.test_bf16_path_matches_the_bf16_emulating_oracle).  The engine runs the whole batch, the oracle the first
    E2E_FRAMES of frames_to_check."""
    bb, B, H, W = row.backbone, row.batch, row.H, row.W
    pick = list(row.frames_to_check[:sg.E2E_FRAMES])
    model, sd = _model(bb, row.dtype, 21, sg.flag_bits(row.plan_flags))
    img, k2d, kc = synth.synth_inputs(B, H, W, seed=22, crop_range=(W, H))
    torch.set_num_threads(min(16, torch.get_num_threads()))
    tag = sg.row_id(row)
    with torch.no_grad():
        if row.dtype == "fp32":
            want = oracle.ca_pf_forward(sd, img[pick], k2d[pick], kc[pick].clone(), backbone=bb)
            got = model(img.cuda(), k2d.cuda(), kc.clone().cuda()).cpu()
            assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(want).all())
            err = (got[pick] - want).abs().max().item()
            mpj = (got[pick] - want).norm(dim=-1).mean().item()
            print(f"{tag}: max|hip - oracle| {err:.3e}   mean per-joint distance {mpj:.3e}   ({len(pick)} frames)")
            assert err <= TOL_OUT
            return
        taps_e, taps_f = {}, {}
        emulate = "stream_fp32" if row.plan_flags == "BF16_F32_STREAM" else True
        with (fp16_emulation() if row.dtype == "fp16" else contextlib.nullcontext()):
            want_e = oracle.ca_pf_forward(sd, img[pick], k2d[pick], kc[pick].clone(), backbone=bb, taps=taps_e, emulate_bf16=emulate)
        want_f = oracle.ca_pf_forward(sd, img[pick], k2d[pick], kc[pick].clone(), backbone=bb, taps=taps_f)
        eng = model.engine_for(img.cuda())
        eng.set_debug(True)
        got = model(img.cuda(), k2d.cuda(), kc.clone().cuda()).cpu()
        assert bool(torch.isfinite(got).all())
        rep = bf16_stage_report(tag, eng, got, pick, taps_e, want_e, taps_f, want_f)
    check_bf16_report(rep)


# ---- schedules ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone,H,W,dtype,B", sg.SCHEDULES, ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[3]}-B{c[4]}" for c in sg.SCHEDULES])
def test_schedules_are_bit_identical(backbone, H, W, dtype, B):
    """capf_set_lanes 0 (program order), 2 (grouped launches, one chain) and 3 (two chains on two streams): the same kernels on the same
    operands -> the same bits (test_gpu_ops.test_engine_modes_are_bit_identical / test_two_chain_schedule_is_bit_identical_to_one_chain at
    full size); twice under 3, where a missing event dependency would show as a run-to-run difference."""
    model, _ = _model(backbone, dtype, 3)
    img, k2d, kc = (t.cuda() for t in synth.synth_inputs(B, H, W, seed=5, crop_range=(W, H)))
    outs = {}
    with torch.no_grad():
        for mode in (0, 2, 3, 3):
            model.engine_for(img).set_lanes(mode)
            outs.setdefault(mode, []).append(model(img, k2d, kc.clone()).clone())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(outs[0][0]).all())
    assert torch.equal(outs[0][0], outs[2][0]) and torch.equal(outs[2][0], outs[3][0]) and torch.equal(outs[3][0], outs[3][1])


# ---- training through tiny maps ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone,hw,B,mode", sg.TRAIN_TINY, ids=[f"{c[0]}-{c[1][0]}x{c[1][1]}-B{c[2]}-{'ordered' if c[3] else 'atomic'}" for c in sg.TRAIN_TINY])
def test_training_step_through_tiny_maps_vs_fp64(backbone, hw, B, mode):
    """test_gpu_features.test_map_gradients_vs_fp64 on maps of 8 x 16 .. 1 x 2 (on the top map every sample of every joint collides): the
    parameter gradients and dL/d(maps) within GRAD_L2_BOUND / GRAD_MAX_BOUND of float64 in both map-gradient modes; the ordered mode twice,
    the same bits."""
    from test_gpu_features import _empty_like_maps, _engine_step, _flat_to_named, _hrnet, _inputs, _map_errors, _maps
    from train_yardstick import check_gradients, engine_cells, engine_clip_sides, lifter64
    torch.set_num_threads(min(16, torch.get_num_threads()))
    H, W = hw
    model = _hrnet(backbone, 51 + B)
    img, k2d, kc, gt = _inputs(B, H, W, 52 + B, (H // 4, W // 4))
    img, k2d = img.cuda(), k2d.cuda()
    eng = model.engine_for(img)
    eng.set_debug(True)
    eng.set_map_grad_mode(mode)
    assert eng.map_grad_mode() == mode
    assert eng.feature_shapes() == [(h, w, c) for (h, w), c in zip(sg.branch_maps(H, W), (32, 64, 128, 256))]
    dfeat = _empty_like_maps(eng, B, float("nan"))
    pred, loss, ref, flat = _engine_step(model, eng, img, k2d, kc, gt, None, dfeat)
    if mode == 1:
        again = _empty_like_maps(eng, B, 1e30)
        _, _, _, flat2 = _engine_step(model, eng, img, k2d, kc, gt, None, again)
        assert torch.equal(flat, flat2) and all(torch.equal(a, b) for a, b in zip(dfeat, again))

    feats = [m.cpu().double().permute(0, 3, 1, 2).contiguous().requires_grad_(True) for m in _maps(eng, B)]
    params = {"volume_net." + n: p for n, p in model.volume_net.named_parameters()}
    tag = f"{backbone} {H}x{W} B={B} map_grad_mode {mode}"
    g64, w64, l64 = lifter64(params, k2d, ref, gt, feats, engine_cells(eng, B), None, engine_clip_sides(eng, B))
    perr, lerr = (pred.double() - w64).abs().max().item(), abs(loss - l64) / abs(l64)
    print(f"  {tag}: prediction max|hip - fp64| {perr:.2e}, loss {loss:.6f} (relative error {lerr:.2e})")
    assert perr <= 1e-5 and lerr <= 1e-6, (perr, lerr)
    print(f"  {tag}: map gradients vs fp64 (relative L2 | max entry / max):")
    l2, mx = _map_errors(tag, dfeat, [f.grad for f in feats])
    pl2, pmx = check_gradients(tag, _flat_to_named(model, eng, flat), g64)
    print(f"  {tag}: worst map gradient {l2:.2e} relative L2, {mx:.2e} of max; worst parameter gradient {pl2:.2e}, {pmx:.2e}")
