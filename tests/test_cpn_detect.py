"""CPU: CPN's own keypoint detector -- the yardstick of its decode (tests/cpn_decode_oracle.py: the blur against scipy, the taps, how many
generated cases leave the peaks undecided), the plan flag on plan-only handles (accepted, refused, nothing moved without it, what it adds),
capf_cpn_decode's refusals (none needs a device) and the constructor argument of CA_PF."""
import contextlib
import copy
import io
from fractions import Fraction

import numpy as np
import pytest

import cpn_decode_oracle as O
from capf import lib as capf

INVALID, UNSUPPORTED = -1, -2          # include/capf.h :: CAPF_ERR_INVALID, CAPF_ERR_UNSUPPORTED
FP = "backbone.refine_net.final_predict"
HEAD_CONVS = [FP + ".0.conv1", FP + ".0.conv2", FP + ".0.downsample.0", FP + ".0.conv3", FP + ".1"]


def _cfg(backbone):
    from mvn.utils.cfg import backbone_preset, config
    c = backbone_preset(copy.deepcopy(config), backbone)
    c.model.backbone.fix_weights = True
    return c


def _plan(backbone, dtype, flags=0, H=256, W=192):
    from mvn.models import _native
    return capf.Engine(_native.make_capf_config(_cfg(backbone), H, W, compute_dtype=dtype, plan_flags=flags), device=None)


# ---- the yardstick ---------------------------------------------------------------------------------------------------------------------
def test_oracle_blur_is_scipys_mirror_correlation():
    ndimage = pytest.importorskip("scipy.ndimage")
    g = O.taps()
    for H, W in O.SHAPES:
        z = O.make_maps(1, H, W, 1, 1, seed=7 * H + W)[0, :, :, 0]
        P = np.zeros((H + 20, W + 20))
        P[10:10 + H, 10:10 + W] = z / z.max()
        want = ndimage.correlate1d(ndimage.correlate1d(P, g, axis=1, mode="mirror"), g, axis=0, mode="mirror")
        gamma = 44 * O.U * O.blur(np.abs(P), g)
        assert (np.abs(O.blur(P, g) - want) <= gamma).all(), (H, W)


def test_taps_are_bit_symmetric_and_sum_to_one():
    lib_taps = capf.cpn_decode_taps()
    for g in (list(O.taps()), lib_taps):
        assert len(g) == 21 and all(g[i] == g[20 - i] for i in range(21)) and all(v > 0 for v in g)
        assert abs(sum(Fraction(v) for v in g) - 1) <= Fraction(1, 2 ** 52)
        assert g[10] == max(g)
    # the library's taps are the oracle's: each is e_i / sum(e) rounded to within an ulp of the exact quotient
    assert all(abs(a - b) <= 2 * np.spacing(b) for a, b in zip(lib_taps, O.taps()))
    e = [float(np.exp(-((i - 10) ** 2) / (2 * 3.5 ** 2))) for i in range(21)]
    assert np.allclose(O.taps(), np.array(e) / sum(e), rtol=1e-14, atol=0)


def _undecided(H, W, dtype):
    maps = O.make_maps(3, H, W, 20, 17, seed=100 * H + W, dtype=dtype)
    res = [O.decode(maps[b, :, :, j]) for b in range(3) for j in range(17)]
    return sum(not r["decided"] for r in res), len(res), res


def test_generated_maps_leave_few_cases_undecided():
    """The generator of the GPU test, all shapes, fp32 and bf16 values: at most 2 % of the (frame, joint) cases may fail `decided`.
    A 1 x 1 map is counted apart: it normalises to n = 1 whatever its value, D = g (x) g, and the four neighbours of the centre tie EXACTLY
    (gap2 = 0) in every evaluation with bit-symmetric taps -- undecided by the rule, every case of it, and no generator can change that; the
    GPU test holds those cases to equality all the same (the tie is exact on both sides, so "first in row-major order" decides it)."""
    bad = total = 0
    for H, W in O.SHAPES:
        for dtype in ("fp32", "bf16"):
            u, n, res = _undecided(H, W, dtype)
            if (H, W) == (1, 1):
                assert u == n and all(r["gap2"] == 0.0 and r["gap1"] > 4 * r["gamma1"] for r in res)
                assert all(r["peaks"] == ((10, 10), (9, 10)) for r in res)
                continue
            bad += u
            total += n
    print(f"undecided: {bad} of {total} (frame, joint) cases")
    assert bad <= 0.02 * total, (bad, total)


def test_oracle_degenerate_and_negative_maps():
    z = np.zeros((4, 3), dtype=np.float32)
    assert O.decode(z)["degenerate"] and np.isnan(O.decode(z)["kcrop"]).all()
    z[1, 1] = np.inf
    assert O.decode(z)["degenerate"]
    z = -np.abs(O.make_maps(1, 8, 6, 1, 1, seed=3)[0, :, :, 0]) - 1          # maximum negative: n = z / M >= 1, the "peak" is the minimum
    r = O.decode(z)
    assert not r["degenerate"] and np.isfinite(r["kcrop"]).all()


# ---- the plan flag on plan-only handles -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_flag_adds_the_head_and_moves_nothing_else(dtype):
    base, flagged = _plan("cpn", dtype), _plan("cpn", dtype, capf.PLAN_CPN_PREDICT)
    assert flagged.schema() == base.schema()
    for B in (1, 2, 6, 24, 128):
        tb, tf = base.op_table(B), flagged.op_table(B)
        assert not any("final_predict" in n for n, _, _ in tb)
        added = [t for t in tf if "final_predict" in t[0]]
        assert [n for n, _, _ in added] == [FP + ".cat", HEAD_CONVS[0], HEAD_CONVS[1], HEAD_CONVS[2], HEAD_CONVS[3], HEAD_CONVS[4]]
        at = [i for i, t in enumerate(tf) if "final_predict" in t[0]]
        # ... the concat right behind the cascades' join, then fork, conv1, conv2, downsample, join, conv3, the last conv; the lifter follows
        first = at[0]
        assert [n for n, _, _ in tf[first:first + 8]] == [FP + ".cat", "fork", HEAD_CONVS[0], HEAD_CONVS[1], HEAD_CONVS[2], "join",
                                                          HEAD_CONVS[3], HEAD_CONVS[4]]
        assert tf[:first] + tf[first + 8:] == tb                     # names, kernels and FLOPs of every other op
        assert added[0][1] == "concat_channels" and added[0][2] == 0.0
        want_flops = [2.0 * 64 * 48 * co * k * B for co, k in ((128, 1024), (128, 9 * 128), (256, 1024), (256, 128), (20, 9 * 256))]
        assert [t[2] for t in added[1:]] == want_flops
    assert flagged.workspace_bytes(1) > base.workspace_bytes(1) and flagged.workspace_bytes(8) > base.workspace_bytes(8)
    assert flagged.feature_shapes() == base.feature_shapes()
    assert flagged.tensor_shape("heat") == (2 if dtype == "bf16" else 0, (64, 48, 20))
    with pytest.raises(capf.CapfError):
        base.tensor_shape("heat")
    # the head's ops are backbone ops, and the walkers skip the concat by its kind
    descs = {flagged.op_table(1)[i][0]: flagged.op_describe(i) for i in range(len(flagged.op_table(1)))}
    assert descs[FP + ".cat"].kind == -1 and descs[FP + ".cat"].backbone
    assert all(descs[n].kind == 0 and descs[n].backbone for n in HEAD_CONVS)
    assert descs[HEAD_CONVS[4]].Cout == 20 and descs[HEAD_CONVS[4]].Cin == 256 and descs[HEAD_CONVS[4]].act == 0
    assert descs[HEAD_CONVS[3]].has_residual and descs[HEAD_CONVS[0]].Cin == 1024


def test_unflagged_plan_is_the_same_at_another_crop():
    base, flagged = _plan("cpn", "bf16", 0, 384, 288), _plan("cpn", "bf16", capf.PLAN_CPN_PREDICT, 384, 288)
    assert flagged.schema() == base.schema() and flagged.tensor_shape("heat") == (2, (64, 48, 20))
    assert [t for t in flagged.op_table(128) if "final_predict" not in t[0] and t[0] not in ("fork", "join")] == \
           [t for t in base.op_table(128) if t[0] not in ("fork", "join")]


def test_flag_is_refused_where_it_does_not_apply():
    with pytest.raises(capf.CapfError, match="CAPF_PLAN_CPN_PREDICT"):
        _plan("hrnet_32", "fp32", capf.PLAN_CPN_PREDICT)
    with pytest.raises(capf.CapfError, match="CAPF_PLAN_CPN_PREDICT"):
        _plan("hrnet_48", "bf16", capf.PLAN_CPN_PREDICT)
    with pytest.raises(capf.CapfError):
        _plan("cpn", "fp16", capf.PLAN_CPN_PREDICT)                  # (fp16 is an HRNet plan)
    for dtype in ("fp32", "bf16"):
        with pytest.raises(capf.CapfError, match="unknown capf_plan_flag"):
            _plan("cpn", dtype, 1 << 14)
        with pytest.raises(capf.CapfError, match="unknown capf_plan_flag"):
            _plan("cpn", dtype, capf.PLAN_CPN_PREDICT | 1 << 14)
    assert capf.PLAN_CPN_PREDICT == 1 << 17


# ---- capf_cpn_decode: refusals before any launch ---------------------------------------------------------------------------------------------
P = 0x10000        # a well-aligned non-NULL "pointer": every call below is refused before anything could read it


def _args(**kw):
    a = dict(stream=None, map=P, dtype=capf.F32, B=2, H=8, W=6, C=20, J=17, decode=(capf.c_float * 4)(4, 2, 4, 2), to_image=None, kcrop=P,
             k2d=None, score=None, blurred=None)
    a.update(kw)
    return list(a.values())


REFUSALS = [
    ("NULL map", dict(map=None), INVALID), ("NULL kcrop", dict(kcrop=None), INVALID), ("NULL decode", dict(decode=None), INVALID),
    ("k2d without to_image", dict(k2d=P), INVALID),
    ("J > C", dict(J=21), INVALID), ("C > 32", dict(C=33, J=33), INVALID), ("C = 36", dict(C=36), INVALID), ("J = 0", dict(J=0), INVALID),
    ("H = 0", dict(H=0), INVALID), ("W = 0", dict(W=0), INVALID), ("B = 0", dict(B=0), INVALID),
    ("misaligned fp32 map", dict(map=P + 8), INVALID), ("misaligned 16-bit map", dict(map=P + 4, dtype=capf.BF16), INVALID),
    ("misaligned blurred", dict(blurred=P + 4), INVALID),
    ("dtype 3", dict(dtype=3), INVALID), ("dtype -1", dict(dtype=-1), INVALID),
    ("plane too large for the LDS", dict(H=128, W=128), UNSUPPORTED), ("far too large", dict(H=4096, W=4096), UNSUPPORTED),
]


@pytest.mark.parametrize("why,kw,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_decode_refusals_need_no_device(why, kw, code):
    assert capf.load_library().capf_cpn_decode(*_args(**kw)) == code, why


def test_decode_lds_budget():
    lib = capf.load_library()
    limit = 160 * 1024
    for H, W in O.SHAPES:
        assert lib.capf_cpn_decode_lds_bytes(H, W) == 256 + 8 * (H + 20) * (W + 20) + 4 * H * W <= limit
    assert lib.capf_cpn_decode_lds_bytes(96, 72) > 64 * 1024         # (upstream CPN's 384 x 288 output needs more than the default dynamic LDS)
    assert lib.capf_cpn_decode_lds_bytes(128, 128) > limit and lib.capf_cpn_decode_lds_bytes(0, 8) == 0
    # a 16-bit map needs 8-byte alignment only
    assert lib.capf_cpn_decode(*_args(map=P + 8, dtype=capf.BF16, H=128, W=128)) == UNSUPPORTED


# ---- the host module -------------------------------------------------------------------------------------------------------------------
def _module(backbone, **kw):
    from mvn.models.conpose import CA_PF
    with contextlib.redirect_stdout(io.StringIO()):
        return CA_PF(_cfg(backbone), **kw)


def test_module_registers_nothing_new():
    plain, cpn = _module("cpn"), _module("cpn", keypoint_head="cpn")
    assert list(cpn.state_dict().keys()) == list(plain.state_dict().keys())
    assert [n for n, _ in cpn.named_parameters()] == [n for n, _ in plain.named_parameters()]
    assert not hasattr(cpn, "keypoint_head") and cpn.keypoint_head_mode == "cpn"
    assert cpn.plan_flags & capf.PLAN_CPN_PREDICT and not plain.plan_flags & capf.PLAN_CPN_PREDICT
    assert _module("cpn", keypoint_head="cpn", compute_dtype="bf16").plan_flags & capf.PLAN_CPN_PREDICT
    assert "final_predict" in type(cpn).__init__.__doc__
    # "argmax" / "integral" on CPN keep their fresh head
    assert "keypoint_head.final_layer.weight" in _module("cpn", keypoint_head="argmax").state_dict()


@pytest.mark.parametrize("backbone", ["hrnet_32", "hrnet_48"])
def test_module_refuses_the_cpn_head_on_hrnet(backbone):
    with pytest.raises(ValueError, match="CPN"):
        _module(backbone, keypoint_head="cpn")
    with pytest.raises(ValueError):
        _module("cpn", keypoint_head="CPN")


def test_module_flip_test_entries_are_not_implemented():
    import torch
    m = _module("cpn", keypoint_head="cpn")
    x = torch.zeros(1, 256, 192, 3)
    with pytest.raises(NotImplementedError, match="flip"):
        m.detect_flip_test(x)
    with pytest.raises(NotImplementedError, match="flip"):
        m.forward_detect_flip_test(x, torch.zeros(1, 2, 3))
    # the head has no derivative: a final_predict parameter that asks for a gradient is refused under grad, before anything runs
    next(m.backbone.refine_net.final_predict.parameters()).requires_grad_(True)
    with pytest.raises(NotImplementedError, match="final_predict"):
        m.forward_detect(x, torch.zeros(1, 2, 3))
