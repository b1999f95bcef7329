"""CPU: the lifter configurations capf_create accepts are exactly those every launcher on their way takes.

A plan-only handle (capf_create with device < 0) is created for every point of
    num_joints 1..40  x  embed_dim_ratio 32..288 in steps of 32  x  num_heads 1..72  x  training 0 / 1
on hrnet_32 at 128 x 96, and the library's answer is compared with the launchers' own conditions, restated below with their csrc lines
(as test_gpu_train_widths.py restates its routes).  A refusal must name the field and the limit in capf_last_error: a configuration the
plan accepts and a launcher then refuses would surface as CAPF_ERR_HIP in the middle of a forward or a backward (before this test:
num_joints = 18 in the first joint block's attention; training = 1 with a joint head dimension above 230 in launch_attention_bwd).
tests/test_gpu_lifter_joints_heads.py runs the instances these conditions select on the GPU.

Also here: CA_PF's parameter tree, its input checks and its engine take the joint and head counts from one place (make_capf_config)."""
import copy
from ctypes import byref, c_void_p

import pytest

LEVELS, DEFORM_HEADS = 4, 4
JOINTS, WIDTHS, HEADS = range(1, 41), range(32, 289, 32), range(1, 73)
LDS_LIMIT = 64 * 1024


# ---- the launchers' conditions, restated ------------------------------------------------------------------------------------------------
def attention_takes(N, d):
    """csrc/lifter.hip attention_ok / launch_attention: the per-query kernels keep NMAX = 5 or 17 scores in registers and read a head's d
    values as float4s; attention_lds_kernel<17> is only a faster route inside these limits"""
    return 1 <= N <= 17 and d >= 4 and d % 4 == 0


def attention_bwd_lds(N, d):
    """csrc/train_kernels.hip attention_bwd_lds_bytes: q, k, v, dO [NMAX][d + 1] and P, dS [NMAX][NMAX + 1] floats of dynamic LDS, NMAX by
    the token count"""
    nmax = 5 if N <= 5 else 17
    return (4 * nmax * (d + 1) + 2 * nmax * (nmax + 1)) * 4


def attention_bwd_takes(N, d):
    """csrc/train_kernels.hip attention_bwd_ok / launch_attention_bwd"""
    return attention_takes(N, d) and attention_bwd_lds(N, d) <= LDS_LIMIT


def violations(J, E, heads, training):
    """The fields a configuration breaks a launcher's condition with: {field: a word of the limit its message must carry}.  Empty: every
    launcher of the forward (training: and of the backward) takes it.
    embed_dim_ratio: the deformable sampler's 4 heads of float4s (E % 16), the LayerNorm and head kernels' 24 values per lane of one wave
    over a joint row (5 E <= 1536) -- never broken on this grid, restated so that the grid cannot grow past them unnoticed."""
    out = {}
    if E % (4 * DEFORM_HEADS) or (LEVELS + 1) * E > 1536:
        out["embed_dim_ratio"] = ""
    if E % (4 * heads):                                        # a head's d = E / heads values are read four at a time (res rows; joint rows 5 d)
        out["num_heads"] = "embed_dim_ratio / 4"
        d = None
    else:
        d = E // heads
    if not 1 <= J <= 17:                                       # the joint blocks' token count
        out["num_joints"] = "1..17"
    if d is not None and not out:
        assert attention_takes(LEVELS + 1, d) and attention_takes(J, (LEVELS + 1) * d)
        if training and not (attention_bwd_takes(LEVELS + 1, d) and attention_bwd_takes(J, (LEVELS + 1) * d)):
            out["num_heads"] = str(LDS_LIMIT)
    return out


@pytest.fixture(scope="module")
def create():
    from capf.lib import load_library
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    lib = load_library()
    cfg = backbone_preset(copy.deepcopy(config), "hrnet_32")

    base = _native.make_capf_config(cfg, 128, 96)

    def _create(J, E, heads, training):
        c = type(base).from_buffer_copy(base)
        c.num_joints, c.embed_dim_ratio, c.num_heads, c.training = J, E, heads, training
        h = c_void_p()
        rc = lib.capf_create(byref(c), -1, byref(h))
        if rc == 0:
            lib.capf_destroy(h)
            return 0, ""
        return rc, lib.capf_last_error(None).decode()
    return _create


def test_restated_rule_limits():
    """the limits, from the restated conditions: d <= 230 on attention_bwd<17>, d <= 815 on <5>; the three training
    configurations at a joint head dimension of 320"""
    assert attention_bwd_takes(17, 228) and not attention_bwd_takes(17, 232) and attention_bwd_lds(17, 180) == 51680
    assert attention_bwd_takes(5, 812) and not attention_bwd_takes(5, 816)
    for E, heads in ((128, 2), (64, 1), (256, 4)):
        assert violations(17, E, heads, 1) == {"num_heads": "65536"} and not violations(17, E, heads, 0)
    assert violations(18, 128, 8, 0) == {"num_joints": "1..17"}
    assert not violations(5, 128, 1, 1) and violations(5, 288, 1, 1) and violations(6, 128, 2, 1)


def test_capf_create_accepts_exactly_what_the_launchers_take(create):
    n_ok = n_refused = 0
    for training in (0, 1):
        for E in WIDTHS:
            for heads in HEADS:
                for J in JOINTS:
                    bad = violations(J, E, heads, training)
                    rc, msg = create(J, E, heads, training)
                    at = f"num_joints {J} embed_dim_ratio {E} num_heads {heads} training {training}"
                    assert (rc == 0) == (not bad), (at, rc, msg, bad)
                    if bad:
                        assert rc == -2, (at, rc)                            # CAPF_ERR_INVALID
                        assert any(field in msg and limit in msg for field, limit in bad.items()), (at, msg, bad)
                        n_refused += 1
                    else:
                        n_ok += 1
    # 17 joint counts x the divisors of E / 4 over the nine widths (68) for inference
    assert n_ok + n_refused == 2 * 40 * 9 * 72 and n_ok > 17 * 68
    print(f"  {n_ok} configurations accepted, {n_refused} refused with the field and the limit named")


@pytest.mark.parametrize("J,E,heads,training,field", [(18, 128, 8, 0, "num_joints"), (17, 128, 2, 1, "num_heads"), (17, 64, 1, 1, "num_heads"),
                                                      (17, 256, 4, 1, "num_heads")])
def test_known_refusals_name_the_field(create, J, E, heads, training, field):
    rc, msg = create(J, E, heads, training)
    assert rc == -2 and field in msg, (rc, msg)
    if training:                                               # the same head count is an inference plan
        assert create(J, E, heads, 0) == (0, "")


def test_module_tree_checks_and_engine_agree_on_the_joint_count():
    """A config with 16 joints and 4 heads: the schema's Spatial_pos_embed is [1, 5, 16, E] (the engine's joint count, not a literal 17),
    the C struct carries both counts, and a (B, 17, 2) keypoint tensor is refused by the module's own shape check."""
    import torch
    from mvn.models import _native
    from mvn.models.conpose import CA_PF, _Source
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), "hrnet_32")
    cfg.model.backbone.fix_weights = True
    cfg.model.backbone.num_joints = 16
    cfg.model.poseformer.num_heads = 4
    c = _native.make_capf_config(cfg, 128, 96)
    assert (c.num_joints, c.num_heads) == (16, 4)
    assert _native.make_capf_config(backbone_preset(copy.deepcopy(config), "hrnet_32")).num_heads == 8
    model = CA_PF(cfg)
    E = cfg.model.poseformer.embed_dim_ratio
    assert model.num_joints == 16 and tuple(model.volume_net.Spatial_pos_embed.shape) == (1, 5, 16, E)
    B = 2
    img = torch.zeros(B, 128, 96, 3)
    src = _Source("images", img.device, B, "images", img)
    with pytest.raises(ValueError, match=r"keypoints_2d_cpn must have shape \(2, 16, 2\), got \(2, 17, 2\)"):
        model._lift(src, None, torch.zeros(B, 17, 2), torch.zeros(B, 17, 2), False)
    with pytest.raises(ValueError, match=r"keypoints_2d_cpn_crop must have shape \(2, 16, 2\), got \(2, 17, 2\)"):
        model._lift(src, None, torch.zeros(B, 16, 2), torch.zeros(B, 17, 2), False)
