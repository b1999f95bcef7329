"""GPU: the lifter at every kind of joint count and head count Engine::build() accepts (tests/test_lifter_config_space.py holds the acceptance
rule itself, on the CPU), against float64.

Every other module pins num_joints = 17 and num_heads = 8.  The joint count J is the token count of the joint blocks and a factor of every
per-(b, p) grid; the head count sets both head dimensions, d = C / heads on the res rows (5 tokens a joint) and 5 C / heads on the joint
rows (J tokens a frame), and with them the attention instance (restated: test_gpu_lifter_ops.attention_instance for the forward,
test_gpu_train_widths.attention_bwd_instance for the backward).  hrnet_32 at 128 x 96 (maps 32 x 24 .. 4 x 3) unless said.  Bounds are the
existing ones, imported: the walker's 2e-5 x sum |terms| per op (bf16: the same or the adjacent number), _hold_to_yardstick's for the step
(prediction 1e-5, loss 1e-6 relative, gradients 2e-5 relative L2 and 2e-5 of the largest entry), the index rule bit for bit, and
test_gpu_features._map_errors / test_gpu_points_grad._hold (the same 2e-5 pair) for the map and keypoint gradients.

(a) every op of the inference schedule (lifter_ops) at C = 128, heads = 8, J in {1, 4, 5, 6, 16, 17} x B in {1, 7}: J = 1 is a one-token
    softmax and a one-row grid (and the only J whose res blocks leave the one-launch chain: one group a frame); 5 | 6 the two sides of the
    <5> / <17> switch on joint rows (J <= 5: attention_split_kernel<5,4> at d = 80, which otherwise only sees d = C / heads); J = 17 at
    (C, heads) = (128, 1) split<17> d = 640, (128, 2) d = 320, 1172 bytes over attention_lds_kernel's LDS limit: split<17>, (128, 4)
    lds<17> d = 160, (128, 32) d = 20 and attention_kernel<5> at d = 4, (96, 3) an odd head count, (288, 4) d = 360 and 72, no multiple of
    16: the plain attention_kernel<17> and <5>; J = 5 at (96, 8): attention_kernel<5> on joint rows (d = 60); a bf16 plan (hrnet_48, 96, 3
    heads, J = 16) and a PLAN_NO_FUSED_LIFTER plan at J = 6, 4 heads.
(b) the training step (_step, _hold_to_yardstick, check_cells_against_index_rule) at (J, C, heads, B, DropPath) of STEP_CASES; B = 2 and
    B >= 5 are the two GEMM pipes; the DropPath cases inject the host's masks, laid out ctx{B} | res{B * J} | joint{B}.
(c) capf_backward_maps (both sums) and capf_backward_points on caller-supplied maps (capf_set_features: no backbone run) at J in
    {1, 4, 5, 16, 17}: the ordered sum sorts J * 64 keys padded to a power of two from 256 up -- J = 4 (256) and J = 16 (1024) are the
    unpadded counts, J = 1 (64) sits under the floor, and only J = 17 (1088 in 2048) had ever run.  White-noise maps
    (feature_cases.synth_maps) with the sampling_offsets scaled by 0.05 (points_grad_cases.tame_): the conditioning under which
    test_gpu_points_grad.py holds the plain 2e-5 bounds; frame 0 has every joint on one pixel (the longest segments of the sort).
(d) a field that is silently ignored must fail: the engine at 4 heads against the oracle at 8, and the engine at 16 joints against the
    oracle on the first 16 joints of a 17-joint position table, both at least 100 x the prediction bound away.

Measured (MI355X; EXPERIMENTS.md R38.1).  (a) worst op, as a fraction of its allowance: J = 1: 1.9e-2 (B = 1) | 3.7e-2 (B = 7), J = 4:
3.7e-2 | 6.2e-2, J = 5: 8.0e-2 | 7.4e-2, J = 6: 5.7e-2 | 5.7e-2, J = 16: 4.5e-2 | 1.1e-1, J = 17: 1.1e-1 | 3.3e-1 (layernorm_kernel<10> at C = 640,
as at 256 x 192); J = 17 at (128, 1) 1.0e-1, (128, 2) 5.3e-2, (128, 4) 7.5e-2, (128, 32) 6.2e-2, (96, 3) 5.0e-2, (288, 4) 1.3e-1; J = 5 at
(96, 8) 4.3e-2; unfused J = 6, 4 heads 8.4e-2; bf16: 0.997 (every result the same or the adjacent bf16 number).  (b) worst of the 191
gradients, relative L2 | of max: 1.8e-6 | 1.8e-6 (J = 1), 8.7e-7 | 1.4e-6 (5), 1.8e-6 | 2.7e-6 (6), 6.7e-7 | 1.0e-6 (16), 4.4e-7 | 9.3e-7
(17, 4 heads), 7.0e-7 | 8.5e-7 (32 heads), 4.4e-7 | 7.9e-7 (96, 3 heads), 7.1e-7 | 9.7e-7 (288).  (c) worst map gradient in ordered mode |
dk2d | dref, relative L2: 2.4e-6 | 1.9e-6 | 2.5e-6 (J = 1), 1.2e-6 | 1.7e-6 | 1.0e-6 (4), 1.2e-6 | 9.2e-7 | 1.1e-6 (5), 1.1e-6 | 1.3e-6 | 1.4e-6
(16), 6.5e-7 | 8.5e-7 | 1.6e-6 (17); the float32 oracle on the same inputs, cells and clip sides sits 5e-7 .. 2.3e-6 from float64 (measured
on the CPU), so the plain 2e-5 bounds apply and no head dimension needed a bound from the float32 oracle.  (d) 1.2e-6 against 1.1e-1
(heads), 1.1e-6 against 5.9e-2 (joints).
Found here: no kernel error.  The host always asked for a training plan, which the new rule refuses at a joint head dimension above 230:
make_capf_config now asks the library and takes the inference plan there (asserted per case in (a))."""
import copy
import re

import pytest
import torch

import capf_oracle as oracle
from capf import synth
from capf.lib import PLAN_NO_FUSED_LIFTER, CapfError, Engine
from feature_cases import HRNET32_128x96, synth_maps
from lifter_models import lifter_model
from points_grad_cases import MARGIN_PX, margin_px, tame_
from test_gpu_features import _map_errors
from test_gpu_lifter_ops import attention_instance, lifter_ops
from test_gpu_points_grad import _hold, _mpjpe_grad, _nhwc, _release, _stream
from test_gpu_train_matrix import _hold_to_yardstick, _step
from test_gpu_train_widths import attention_bwd_instance
from test_lifter_config_space import attention_bwd_takes
from train_yardstick import check_cells_against_index_rule, engine_cells, engine_clip_sides

pytestmark = pytest.mark.gpu

LEVELS = 4
RES, JOINT = "res rows", "joint rows"


# ---- routes, restated -----------------------------------------------------------------------------------------------------------------------
def res_chain_taken(J, C, heads, fused):
    """csrc/plan.cpp attn_blocks (:895) / lifter_chain.hip res_chain_ok: the res blocks as one launch -- the fused fp32 plan at C = 128 with 8
    heads and more than one group (joint) a frame"""
    return fused and C == 128 and heads == 8 and J > 1


def forward_routes(J, C, heads, bf16=False, fused=True):
    """{(attention template, rows): instance name in op_table} of an inference plan; the res rows inside the chain launch have none"""
    out = {}
    for rows, N, d in ((RES, LEVELS + 1, C // heads), (JOINT, J, (LEVELS + 1) * C // heads)):
        if rows == RES and res_chain_taken(J, C, heads, fused and not bf16 and C <= 256):
            continue
        inst = attention_instance(N, d, bf16)
        out[(re.match(r"(\w+<\d+)", inst).group(1) + ">", rows)] = inst
    return out


def backward_routes(J, C, heads):
    """{(attention_bwd instance, rows): (name, LDS bytes)} of a training step"""
    out = {}
    for rows, N, d in ((RES, LEVELS + 1, C // heads), (JOINT, J, (LEVELS + 1) * C // heads)):
        name, lds = attention_bwd_instance(N, d)
        out[(name.split(" ")[0], rows)] = (name, lds)
    return out


# every template launch_attention can pick for a configuration Engine::build accepts, by the rows it runs on: the res rows are 5 tokens
# whatever J is (no <17> there), attention_lds_kernel exists as <17> alone.  (The bf16 / fp16 writers are the same bodies with a narrowing
# store; the bf16 case below reaches two of them.)
FORWARD_REACHABLE = {("attention_split_kernel<5>", RES), ("attention_kernel<5>", RES), ("attention_split_kernel<5>", JOINT),
                     ("attention_kernel<5>", JOINT), ("attention_lds_kernel<17>", JOINT), ("attention_split_kernel<17>", JOINT),
                     ("attention_kernel<17>", JOINT)}
BACKWARD_REACHABLE = {("attention_bwd<5>", RES), ("attention_bwd<5>", JOINT), ("attention_bwd<17>", JOINT)}      # (<17> on res rows: 5 tokens, never)


# ---- (a) every op, inference ------------------------------------------------------------------------------------------------------------------
OPS_CASES = ([("hrnet_32", "fp32", J, 128, 8, B, 0) for J in (1, 4, 5, 6, 16, 17) for B in (1, 7)] +
             [("hrnet_32", "fp32", 17, C, heads, 3, 0) for C, heads in ((128, 1), (128, 2), (128, 4), (128, 32), (96, 3), (288, 4))] +
             [("hrnet_32", "fp32", 5, 96, 8, 2, 0), ("hrnet_48", "bf16", 16, 96, 3, 3, 0), ("hrnet_32", "fp32", 6, 128, 4, 3, PLAN_NO_FUSED_LIFTER)])
# the instances each case is here for, written out (the rule above must agree: asserted before the run)
OPS_PINS = {
    (1, 128, 8): {"attention_split_kernel<5,4> d=80", "attention_split_kernel<5,4> d=16"},
    (4, 128, 8): {"attention_split_kernel<5,4> d=80"}, (5, 128, 8): {"attention_split_kernel<5,4> d=80"},
    (6, 128, 8): {"attention_lds_kernel<17> d=80"}, (16, 128, 8): {"attention_lds_kernel<17> d=80"}, (17, 128, 8): {"attention_lds_kernel<17> d=80"},
    (17, 128, 1): {"attention_split_kernel<17,4> d=640", "attention_split_kernel<5,4> d=128"},
    (17, 128, 2): {"attention_split_kernel<17,4> d=320", "attention_split_kernel<5,4> d=64"},
    (17, 128, 4): {"attention_lds_kernel<17> d=160", "attention_split_kernel<5,4> d=32"},
    (17, 128, 32): {"attention_lds_kernel<17> d=20", "attention_kernel<5> d=4"},
    (17, 96, 3): {"attention_lds_kernel<17> d=160", "attention_split_kernel<5,4> d=32"},
    (17, 288, 4): {"attention_kernel<17> d=360", "attention_kernel<5> d=72"},
    (5, 96, 8): {"attention_kernel<5> d=60", "attention_kernel<5> d=12"},
    (16, 96, 3): {"attention_lds_kernel<17,bf16> d=160", "attention_split_kernel<5,4,bf16> d=32"},
    (6, 128, 4): {"attention_lds_kernel<17> d=160", "attention_split_kernel<5,4> d=32"},
}


def _ops_id(c):
    return f"{c[0]}-{c[1]}-J{c[2]}-E{c[3]}-h{c[4]}-B{c[5]}" + ("-unfused" if c[6] else "")


@pytest.mark.parametrize("case", OPS_CASES, ids=[_ops_id(c) for c in OPS_CASES])
def test_lifter_ops_at_joint_and_head_counts(case):
    backbone, dtype, J, C, heads, B, flags = case
    torch.set_num_threads(min(16, torch.get_num_threads()))
    fused = not flags
    want = forward_routes(J, C, heads, dtype == "bf16", fused)
    assert OPS_PINS[(J, C, heads)] == set(want.values()), (sorted(want.values()), sorted(OPS_PINS[(J, C, heads)]))
    model, sd = lifter_model(backbone, dtype=dtype, embed=C, plan_flags=flags, joints=J, heads=heads, wseed=81 + J + heads)
    try:
        assert tuple(sd["volume_net.Spatial_pos_embed"].shape) == (1, LEVELS + 1, J, C)
        w = lifter_ops(model, sd, B, 128, 96, iseed=82 + J + B)
        kernels = lifter_ops.kernels
        # the host asks for a training plan wherever the library accepts one (fp32, bf16), and for the inference plan a head count keeps
        trains = attention_bwd_takes(J, (LEVELS + 1) * C // heads) and attention_bwd_takes(LEVELS + 1, C // heads)
        assert [e.cfg.training for e in model._engines.values()] == [int(trains)]
        for inst in want.values():
            assert inst in w, (inst, sorted(k for k in w if k.startswith("attention")))
        assert ("res_chain" in kernels) == res_chain_taken(J, C, heads, fused and dtype == "fp32" and C <= 256), sorted(kernels)
        assert len([k for k in w if k.startswith("attention")]) == len(want)
        if flags:
            assert {"prep_embed", "sample_ref", "deform_sample"} <= kernels
        worst = max(e for _, e, _ in w.values())
        print(f"  {_ops_id(case)}: worst op {worst:.2e} of the allowance")
    finally:
        _release(model)
        del model
        torch.cuda.empty_cache()


# ---- (b) the training step ----------------------------------------------------------------------------------------------------------------------
STEP_CASES = [
    # J, C, heads, B, DropPath, the attention_bwd instances the case is here for
    (1, 128, 8, 2, 0.0, {"attention_bwd<5> d=80", "attention_bwd<5> d=16"}),
    (5, 128, 8, 6, 0.2, {"attention_bwd<5> d=80"}),
    (6, 128, 8, 2, 0.0, {"attention_bwd<17> d=80"}),
    (16, 128, 8, 13, 0.2, {"attention_bwd<17> d=80"}),
    (17, 128, 4, 6, 0.0, {"attention_bwd<17> d=160", "attention_bwd<5> d=32"}),
    (17, 128, 32, 2, 0.0, {"attention_bwd<17> d=20", "attention_bwd<5> d=4"}),
    (17, 96, 3, 6, 0.0, {"attention_bwd<17> d=160", "attention_bwd<5> d=32"}),
    (17, 288, 8, 2, 0.0, {"attention_bwd<17> d=180", "attention_bwd<5> d=36"}),      # (the LDS limit case: 51 680 bytes)
]


def _step_id(c):
    return f"J{c[0]}-E{c[1]}-h{c[2]}-B{c[3]}" + ("-droppath" if c[4] else "")


@pytest.mark.parametrize("case", STEP_CASES, ids=[_step_id(c) for c in STEP_CASES])
def test_training_step_vs_fp64_yardstick_at_joint_and_head_counts(case):
    J, C, heads, B, drop, pins = case
    torch.set_num_threads(min(16, torch.get_num_threads()))
    bwd = backward_routes(J, C, heads)
    assert pins <= {name for name, _ in bwd.values()}, (pins, bwd)
    assert all(lds <= 64 * 1024 for _, lds in bwd.values())
    if (C, heads) == (288, 8):
        assert bwd[("attention_bwd<17>", JOINT)][1] == 51680
    model, _ = lifter_model("hrnet_32", embed=C, joints=J, heads=heads, wseed=61 + B + C + J)
    try:
        model.train(); model.backbone.eval(); model.volume_net.train()
        model.drop_path_rate = drop
        assert sum(1 for _ in model.volume_net.parameters()) == 191
        assert tuple(model.volume_net.Spatial_pos_embed.shape) == (1, LEVELS + 1, J, C)
        img, k2d, kc, gt = synth.synth_inputs(B, 128, 96, seed=62 + B + C + J, crop_range=(192, 256), with_gt=True, joints=J)
        masks = None
        if drop:
            torch.manual_seed(7)
            masks = model._drop_masks(B, torch.device("cuda"))
            assert (masks == 0).any() and masks.numel() == 2 * 4 * (B + J * B + B)
            parts = oracle.split_drop_masks(masks.cpu(), B, J)
            assert [tuple(m.shape) for m in parts["res"][0]] == [(B * J, 1, 1)] * 2 and [tuple(m.shape) for m in parts["joint"][3]] == [(B, 1, 1)] * 2
            assert torch.equal(parts["res"][0][0].flatten(), masks.cpu()[2 * 4 * B:][:B * J])
            model._drop_masks = lambda b, dev: masks             # the step below uses exactly these multipliers
        eng = model.engine_for(img.cuda())
        assert (eng.cfg.num_joints, eng.cfg.num_heads, eng.cfg.training) == (J, heads, 1)
        eng.set_debug(True)                                    # cidx / cpos taps of the deformable samplers
        pred, loss, ref = _step(model, img, k2d, kc, gt)
        assert tuple(pred.shape) == (B, 1, J, 3)
        tag = f"J={J} E={C} heads={heads} B={B} DropPath {drop} [" + ", ".join(sorted(name for name, _ in bwd.values())) + "]"
        check_cells_against_index_rule(eng, B, tag)
        (l2, mx), _ = _hold_to_yardstick(tag, model, eng, B, k2d, ref, gt, pred, loss, masks)
        print(f"  {_step_id(case)}: worst gradient {l2:.2e} relative L2, {mx:.2e} of max")
    finally:
        _release(model)
        del model
        torch.cuda.empty_cache()


# ---- (c) map and keypoint gradients on caller-supplied maps ------------------------------------------------------------------------------------
ATOMIC, ORDERED = 0, 1
GRAD_CASES = [(1, 2), (4, 2), (5, 6), (16, 6), (17, 2)]        # J, B: both GEMM pipes; ordered keys 64, 256, 320, 1024, 1088


def _grad_inputs(J, B):
    maps = synth_maps(B, HRNET32_128x96, 140 + J)
    _, k2d, kc, gt = synth.synth_inputs(B, 128, 96, seed=141 + J, crop_range=(192, 256), with_gt=True, joints=J)
    kc = kc.clone()
    kc[0] = torch.tensor([50.3, 70.7])                         # frame 0: every joint on one pixel of every map
    return maps, k2d, kc, gt


def _grad_model(J, heads=None, wseed=None):
    model, _ = lifter_model("hrnet_32", joints=J, heads=heads, wseed=wseed or 142 + J)
    tame_(dict(model.volume_net.named_parameters()))
    model.train(); model.backbone.eval(); model.volume_net.train()
    model.drop_path_rate = 0.0
    eng = model._engine_at(torch.zeros(1, device="cuda").device, 128, 96)
    eng.set_debug(True)
    return model, eng


def _forward_on_maps(eng, maps, k2d, kc):
    B, J = k2d.shape[:2]
    k2d_dev, kc_dev, out = k2d.cuda(), kc.clone().cuda(), torch.full((B, 1, J, 3), float("nan"), device="cuda")
    eng.set_features(_nhwc(maps), _stream())
    eng.lifter_forward_train(k2d_dev, kc_dev, out, _stream(), None)
    torch.cuda.synchronize()
    return out, kc_dev, k2d_dev


def _yardstick64(model, eng, k2d, ref, gt, maps, heads=8, params=None, fixed=True):
    """points_grad_cases.points64's recipe with the maps as leaves too: (dmaps, dk2d, dref, prediction, loss) in float64"""
    B = k2d.shape[0]
    P = params or {"volume_net." + n: p.detach().cpu().double() for n, p in model.volume_net.named_parameters()}
    k, r = (t.detach().cpu().double().clone().requires_grad_(True) for t in (k2d, ref))
    fs = [m.detach().cpu().double().clone().requires_grad_(True) for m in maps]
    w = oracle.lifter_forward(P, k, r, fs, cells=engine_cells(eng, B) if fixed else None, unclipped=engine_clip_sides(eng, B) if fixed else None,
                              heads=heads)
    loss = oracle.mpjpe(w, gt.double())
    loss.backward()
    return [f.grad for f in fs], k.grad, r.grad, w.detach(), loss.item()


def _backward_maps(eng, dout, B, mode, fill):
    _, total = eng.grad_layout_cached()
    eng.set_map_grad_mode(mode)
    flat = torch.full((total,), float("nan"), device="cuda")
    dfeat = [torch.full((B, h, w, c), fill, device="cuda") for h, w, c in eng.feature_shapes()]
    eng.backward_maps(dout, flat, dfeat, _stream(), None)
    torch.cuda.synchronize()
    assert torch.isfinite(flat).all()
    return flat, dfeat


@pytest.mark.parametrize("J,B", GRAD_CASES, ids=[f"J{j}-B{b}" for j, b in GRAD_CASES])
def test_map_and_keypoint_gradients_on_supplied_maps(J, B):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    maps, k2d, kc, gt = _grad_inputs(J, B)
    model, eng = _grad_model(J)
    model2 = None
    try:
        out, ref_dev, k2d_dev = _forward_on_maps(eng, maps, k2d, kc)
        ref = ref_dev.cpu()
        assert margin_px(ref) >= MARGIN_PX
        loss, dout = _mpjpe_grad(out, gt)
        dmaps, dk2d, dref, w64, l64 = _yardstick64(model, eng, k2d, ref, gt, maps)
        perr = (out.cpu().double() - w64).abs().max().item()
        print(f"  J={J} B={B}: prediction max|hip - fp64| {perr:.2e}, loss {loss:.6f} vs {l64:.6f}")
        assert perr <= 1e-5 and abs(loss - l64) <= 1e-6 * abs(l64)
        flat_a, df_atomic = _backward_maps(eng, dout, B, ATOMIC, float("nan"))
        flat_o, df_ordered = _backward_maps(eng, dout, B, ORDERED, float("nan"))
        flat_o2, df_again = _backward_maps(eng, dout, B, ORDERED, 1e30)
        assert torch.equal(flat_a, flat_o) and torch.equal(flat_o, flat_o2)
        _map_errors(f"J={J} B={B} atomic", df_atomic, dmaps)
        l2, mx = _map_errors(f"J={J} B={B} ordered", df_ordered, dmaps)
        assert all(torch.equal(a, b) for a, b in zip(df_ordered, df_again))
        # the keypoint gradients of the same saved step
        _, total = eng.grad_layout_cached()
        flat_p = torch.full((total,), float("nan"), device="cuda")
        got_k, got_r = torch.full((B, J, 2), float("nan"), device="cuda"), torch.full((B, J, 2), float("nan"), device="cuda")
        eng.backward_points(dout, flat_p, _stream(), None, None, got_k, got_r)
        torch.cuda.synchronize()
        assert torch.equal(flat_p, flat_a) and torch.isfinite(got_k).all() and torch.isfinite(got_r).all()
        kl2, kmx = _hold(f"J={J} B={B} dk2d", got_k, dk2d)
        rl2, rmx = _hold(f"J={J} B={B} dref", got_r, dref)
        print(f"  J{J}-B{B}: worst map gradient (ordered) {l2:.2e} | {mx:.2e}, dk2d {kl2:.2e} | {kmx:.2e}, dref {rl2:.2e} | {rmx:.2e}")
        # a second model and handle from the same seeds, other addresses: the same bits in ordered mode
        pad = torch.empty(12345, device="cuda")
        model2, eng2 = _grad_model(J)
        assert eng2 is not eng
        out2, keep_r, keep_k = _forward_on_maps(eng2, maps, k2d, kc)
        assert torch.equal(out2, out)
        flat2, df2 = _backward_maps(eng2, dout, B, ORDERED, float("nan"))
        assert torch.equal(flat2, flat_o) and all(torch.equal(a, b) for a, b in zip(df2, df_ordered))
        del pad
    finally:
        _release(*(m for m in (model, model2) if m is not None))
        torch.cuda.empty_cache()


# ---- (d) a field that is silently ignored must fail --------------------------------------------------------------------------------------------
PREDICTION_BOUND = 1e-5          # (_hold_to_yardstick's, and the assertion on perr above)


def test_an_ignored_head_count_would_fail():
    """the engine at 4 heads against the oracle at 8 on the same weights: the oracle at 4 is within the bound, at 8 at least 100 x outside"""
    J, B = 17, 2
    maps, k2d, kc, gt = _grad_inputs(J, B)
    model, eng = _grad_model(J, heads=4)
    try:
        assert eng.cfg.num_heads == 4
        out, ref_dev, _ = _forward_on_maps(eng, maps, k2d, kc)
        errs = {}
        for heads in (4, 8):
            w64 = _yardstick64(model, eng, k2d, ref_dev.cpu(), gt, maps, heads=heads)[3]
            errs[heads] = (out.cpu().double() - w64).abs().max().item()
        print(f"  engine at 4 heads: {errs[4]:.2e} from the oracle at 4 heads, {errs[8]:.2e} from the oracle at 8")
        assert errs[4] <= PREDICTION_BOUND and errs[8] >= 100 * PREDICTION_BOUND, errs
    finally:
        _release(model)


def test_an_ignored_joint_count_would_fail():
    """the engine at 16 joints against the oracle fed the first 16 joints of a 17-joint position table (what a library that ignored the
    field and kept 17 would read): within the bound on its own table, at least 100 x outside on that one"""
    J, B = 16, 2
    maps, k2d, kc, gt = _grad_inputs(J, B)
    model, eng = _grad_model(J)
    try:
        assert eng.cfg.num_joints == 16
        out, ref_dev, _ = _forward_on_maps(eng, maps, k2d, kc)
        P = {"volume_net." + n: p.detach().cpu().double() for n, p in model.volume_net.named_parameters()}
        own = P["volume_net.Spatial_pos_embed"]
        table17 = torch.from_numpy(synth.synth_tensor("volume_net.Spatial_pos_embed", (1, 5, 17, own.shape[-1]), 142 + J, {})).double()
        assert torch.equal(own.float(), torch.from_numpy(synth.synth_tensor("volume_net.Spatial_pos_embed", tuple(own.shape), 142 + J, {})))
        errs = {}
        for name, table in (("own", own), ("first 16 of 17", table17[:, :, :16].contiguous())):
            w64 = _yardstick64(model, eng, k2d, ref_dev.cpu(), gt, maps, params=dict(P, **{"volume_net.Spatial_pos_embed": table}))[3]
            errs[name] = (out.cpu().double() - w64).abs().max().item()
        print(f"  engine at 16 joints: {errs['own']:.2e} from the oracle on its table, {errs['first 16 of 17']:.2e} on the first 16 joints of a 17-joint table")
        assert errs["own"] <= PREDICTION_BOUND and errs["first 16 of 17"] >= 100 * PREDICTION_BOUND, errs
    finally:
        _release(model)


# ---- refused at create, on a device handle as on a plan-only one ---------------------------------------------------------------------------------
@pytest.mark.parametrize("J,C,heads,training,field", [(18, 128, 8, 0, "num_joints"), (17, 128, 2, 1, "num_heads"), (17, 64, 1, 1, "num_heads"),
                                                      (17, 256, 4, 1, "num_heads")])
def test_refused_at_create_on_a_device_handle(J, C, heads, training, field):
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    c = _native.make_capf_config(backbone_preset(copy.deepcopy(config), "hrnet_32"), 128, 96)
    c.num_joints, c.embed_dim_ratio, c.num_heads, c.training = J, C, heads, training
    for device in (None, torch.cuda.current_device()):
        with pytest.raises(CapfError, match=field):
            Engine(c, device=device)


# what the cases cover together: a later edit of the cases cannot silently drop an instance
_fwd = set().union(*(set(forward_routes(c[2], c[3], c[4], False, not c[6])) for c in OPS_CASES if c[1] == "fp32"))
assert _fwd >= FORWARD_REACHABLE, sorted(FORWARD_REACHABLE - _fwd)
_bwd = set().union(*(set(backward_routes(c[0], c[1], c[2])) for c in STEP_CASES))
assert _bwd >= BACKWARD_REACHABLE, sorted(BACKWARD_REACHABLE - _bwd)
