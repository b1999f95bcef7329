"""CPU: batch-statistics BatchNorm for the frozen HRNet backbone in train mode -- the yardstick, the plan flag, the host argument.

1. The swapped oracle (tests/bn_train_report.py batch_stat_bn) replays tests/golden/mpi_bn_train_w32_64x64.npz, recorded from the REAL
   reference backbone of the MPI-INF-3DHP app under .train() (tools/make_bn_train_golden.py), at test_oracle_golden's tolerance for map
   slices; and the batch-statistics maps are nowhere near the running-statistics maps.
2. CAPF_PLAN_BN_BATCH_STATS on plan-only handles: accepted exactly for HRNet-32 / 48 + fp32 + training, four refusals with their reasons,
   the plan it describes is the flagless handle's, the workspace may only grow; header, EXPORTS and capf.map agree at revision 12.
3. CA_PF / VolumetricTriangulationNet(backbone_bn=...): default, unknown values, forward_u8 under a training backbone."""
import contextlib
import copy
import io
import os
import re

import numpy as np
import pytest
import torch

import bn_train_report as bnr
import capf_oracle as oracle
from bn_train_cases import GOLDEN, NAMED_LAYERS, golden_frames
from capf import lib as capf
from capf import synth
from test_oracle_golden import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mpi_model(backbone="hrnet_32", **kw):
    from model.conpose import VolumetricTriangulationNet, mpi_preset
    from mvn.utils.cfg import config
    with contextlib.redirect_stdout(io.StringIO()):
        return VolumetricTriangulationNet(mpi_preset(copy.deepcopy(config), backbone), **kw)


# ---- 1. the yardstick ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def replay():
    """three train-mode forwards of the swapped fp32 oracle on the fixture's seeded case: maps per step, eval maps before / after, the dict"""
    g = np.load(os.path.join(ROOT, "tests", "golden", "mpi_bn_train_w32_64x64.npz"))
    sd = synth.load_synthetic(_mpi_model(GOLDEN["backbone"]), seed=GOLDEN["wseed"], bn_mode="random")
    P = bnr.clone_sd(sd)
    x0 = golden_frames(0).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        before = oracle.hrnet_forward(P, x0)
        steps = [bnr.train_maps(P, golden_frames(s), GOLDEN["backbone"]) for s in range(GOLDEN["steps"])]
        after = oracle.hrnet_forward(P, x0)
    return g, sd, P, before, steps, after


def test_swapped_oracle_replays_the_reference_backbone_in_train_mode(replay):
    g, sd, P, before, steps, after = replay
    for tag, maps in (("eval_before", before), ("step1", steps[0]), ("step3", steps[-1]), ("eval_after", after)):
        for l in range(4):
            np.testing.assert_allclose(maps[l].numpy(), g[f"{tag}_feat{l}"], atol=TOL, err_msg=f"{tag} feat{l}")
    for name in NAMED_LAYERS:
        np.testing.assert_allclose(P[f"backbone.{name}.running_mean"].numpy(), g["mean:" + name], atol=TOL, err_msg=name)
        np.testing.assert_allclose(P[f"backbone.{name}.running_var"].numpy(), g["var:" + name], atol=TOL, err_msg=name)
    bns = sorted(bnr.backbone_keys(P))                  # (the fixture's digest rows are in name order)
    assert len(bns) == 292 == len(g["digest_mean"]) and (g["num_batches_tracked"] == GOLDEN["steps"]).all()
    for what, rows in (("running_mean", g["digest_mean"]), ("running_var", g["digest_var"])):
        got = np.array([[P[f"{b}.{what}"].double().sum().item(), P[f"{b}.{what}"].double().abs().sum().item()] for b in bns])
        np.testing.assert_allclose(got[:, 1], rows[:, 1], rtol=1e-5, err_msg=what)
        np.testing.assert_allclose(got[:, 0], rows[:, 0], rtol=1e-5, atol=1e-5 * float(np.abs(rows[:, 1]).max()), err_msg=what)
    # the swap is undone: outside the context the oracle normalises with the running statistics and moves nothing
    Q = bnr.clone_sd(P)
    with torch.no_grad():
        again = oracle.hrnet_forward(Q, golden_frames(0).permute(0, 3, 1, 2).contiguous())
    assert all(torch.equal(a, b) for a, b in zip(again, after)) and all(torch.equal(Q[k], P[k]) for k in P)


def test_batch_statistics_maps_are_far_from_running_statistics_maps(replay):
    g, sd, P, before, steps, after = replay
    for l in range(4):
        d = bnr.rel_dist(steps[0][l], before[l])
        moved = bnr.rel_dist(after[l], before[l])
        print(f"  feat{l}: batch-statistics vs running-statistics maps {d:.3f} of the maximum; eval maps moved by {moved:.3f} after three steps")
        assert d >= 0.5 and moved > 0.1


def test_swapped_oracle_works_in_fp64_and_updates_the_dict_it_is_given(replay):
    g, sd, P32, before, steps, after = replay
    P = bnr.to_double(sd)
    maps = bnr.train_maps(P, golden_frames(0), GOLDEN["backbone"])
    k = "backbone.bn1.running_mean"
    assert maps[0].dtype == torch.float64 and P[k].dtype == torch.float64 and not torch.equal(P[k], sd[k].double())
    for l in range(4):
        assert bnr.rel_dist(steps[0][l], maps[l]) < 1e-3


# ---- 2. the plan flag ------------------------------------------------------------------------------------------------------------
def _cfg(backbone, dtype="fp32", flags=0, H=64, W=64, mpi=False):
    from model.conpose import mpi_preset
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    cfg = (mpi_preset if mpi else backbone_preset)(copy.deepcopy(config), backbone)
    return _native.make_capf_config(cfg, H, W, context_blocks=not mpi, compute_dtype=dtype, plan_flags=flags)


@pytest.mark.parametrize("backbone", ["hrnet_32", "hrnet_48"])
@pytest.mark.parametrize("mpi", [False, True])
def test_flag_leaves_the_plan_as_it_is(backbone, mpi):
    a = capf.Engine(_cfg(backbone, flags=capf.PLAN_BN_BATCH_STATS, mpi=mpi))
    b = capf.Engine(_cfg(backbone, mpi=mpi))
    assert a.schema() == b.schema()
    assert a.lib.capf_num_ops(a.h) == b.lib.capf_num_ops(b.h)
    for batch in (1, 5, 64):
        assert a.op_table(batch) == b.op_table(batch)
        assert a.workspace_bytes(batch) >= b.workspace_bytes(batch) > 0
        assert a.workspace_bytes(batch) - b.workspace_bytes(batch) < 64 << 20       # the statistics scratch: four slots of slab partials
    assert a.max_batch() == b.max_batch()


@pytest.mark.parametrize("why,make", [
    ("CPN50", lambda: _cfg("cpn", flags=capf.PLAN_BN_BATCH_STATS)),
    ("CAPF_F32", lambda: _cfg("hrnet_32", "bf16", capf.PLAN_BN_BATCH_STATS)),
    ("CAPF_F32", lambda: _cfg("hrnet_32", "fp16", capf.PLAN_BN_BATCH_STATS)),
    ("training = 1", lambda: _cfg("hrnet_32", flags=capf.PLAN_BN_BATCH_STATS)),
    ("CAPF_PLAN_BF16_F32_STREAM", lambda: _cfg("hrnet_32", flags=capf.PLAN_BN_BATCH_STATS | capf.PLAN_BF16_F32_STREAM)),
])
def test_flag_refusals_name_the_flag(why, make):
    c = make()
    if why == "training = 1":
        c.training = 0
    h = capf.c_void_p()
    lib = capf.load_library()
    assert lib.capf_create(capf.byref(c), -1, capf.byref(h)) == -2       # CAPF_ERR_UNSUPPORTED
    msg = lib.capf_last_error(None).decode()
    assert "CAPF_PLAN_BN_BATCH_STATS" in msg and why in msg, msg


def test_flag_bit_header_exports_and_map_agree():
    lib = capf.load_library()
    assert lib.capf_abi_version() == 12 == capf.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "capf.h")).read()
    assert re.search(r"#define CAPF_ABI_VERSION 12\b", header)
    m = re.search(r"CAPF_PLAN_BN_BATCH_STATS\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == capf.PLAN_BN_BATCH_STATS == 1 << 16 and capf.PLAN_BN_BATCH_STATS > capf.PLAN_BF16_F32_STREAM
    declared = set(re.findall(r"^[a-z][\w \*]*?\b(capf_\w+)\(", header, re.M))
    new = {"capf_backbone_forward_bn", "capf_op_bn_stats_scratch_bytes", "capf_op_bn_stats", "capf_op_bn_apply"}
    assert new <= declared and new <= set(capf.EXPORTS) and declared == set(capf.EXPORTS)
    for s in new:
        assert hasattr(lib, s), s
    assert "capf_*" in open(os.path.join(ROOT, "contextaware-poseformer_amd", "csrc", "capf.map")).read()
    # a plan-only handle refuses the run entry like every other: CAPF_ERR_STATE, flag or no flag
    for flags in (0, capf.PLAN_BN_BATCH_STATS):
        e = capf.Engine(_cfg("hrnet_32", flags=flags))
        x = torch.zeros(2, 64, 64, 3)
        assert lib.capf_backbone_forward_bn(e.h, None, capf.c_void_p(x.data_ptr()), 2, 0.1) == -4
        assert ("CAPF_PLAN_BN_BATCH_STATS" if not flags else "plan-only") in lib.capf_last_error(e.h).decode()
    assert lib.capf_op_bn_stats_scratch_bytes(1 << 15, 32) > 0 and lib.capf_op_bn_stats_scratch_bytes(8, 30) == 0


# ---- 3. the host argument --------------------------------------------------------------------------------------------------------
def test_backbone_bn_argument():
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    m = _mpi_model()
    assert m.backbone_bn == "running" and m.plan_flags == 0 and not m._bn_batch_active()
    m.train()
    assert not m._bn_batch_active()                     # the default keeps today's route for a frozen backbone left in train mode
    with contextlib.redirect_stdout(io.StringIO()):
        assert CA_PF(backbone_preset(copy.deepcopy(config), "hrnet_32")).backbone_bn == "running"
    for bad in ("sync", "Batch", None, 1):
        with pytest.raises(ValueError, match="backbone_bn"):
            _mpi_model(backbone_bn=bad)
    with pytest.raises(ValueError, match="backbone_bn"), contextlib.redirect_stdout(io.StringIO()):
        CA_PF(backbone_preset(copy.deepcopy(config), "cpn"), backbone_bn="batch")
    with pytest.raises(ValueError, match="backbone_bn"):
        _mpi_model(backbone_bn="batch", compute_dtype="bf16")
    b = _mpi_model(backbone_bn="batch")
    assert b.plan_flags == capf.PLAN_BN_BATCH_STATS
    b.train()
    assert b._bn_batch_active()
    u8, k = torch.zeros(2, 64, 64, 3, dtype=torch.uint8), torch.zeros(2, 17, 2)
    with pytest.raises(NotImplementedError, match="batch-statistics"):
        b.forward_u8(u8, k, k.clone())
    b.backbone.eval()                                   # an explicit backbone.eval() wins
    assert not b._bn_batch_active()
    with pytest.raises(capf.CapfError):                 # ... and forward_u8 is back to its usual checks (CPU tensors: no device, no fallback)
        b.forward_u8(u8, k, k.clone())
