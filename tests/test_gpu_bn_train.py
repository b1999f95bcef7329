"""GPU: batch-statistics BatchNorm for the frozen HRNet backbone in train mode (CAPF_PLAN_BN_BATCH_STATS, capf_backbone_forward_bn,
capf_op_bn_stats / capf_op_bn_apply, CA_PF(backbone_bn="batch")).

Yardsticks.  The stand-alone ops go against torch's F.batch_norm(training=True) in float64; the backbone against the CPU oracle with its
BatchNorm swapped to batch statistics (tests/bn_train_report.py), evaluated in float64.  Every bound is 4 x d32 + floor, where d32 is the
distance of the SAME fp32 CPU evaluation (torch's F.batch_norm, the fp32 oracle) from float64 on the same input, computed here and never
taken from the GPU, and the floor is 1e-6 (ops) / 1e-5 (network) of the quantity's largest magnitude.  Expected ratio about 1; the factor
covers a different but fixed summation order and stays orders of magnitude below what a cancelling variance (ops) or running statistics
in place of batch statistics (0.8 - 0.99 of a map's maximum) produce.

Shapes: every BatchNorm of the network sees at least 8 values per channel (HRNet at 64x64 from batch 2: the deepest map is 2x2); below
that the network is ill-conditioned, not the kernel (the fp32 oracle is 0.2 - 0.5 of a map's maximum from its own fp64 evaluation)."""
import contextlib
import copy
import io

import pytest
import torch
import torch.nn.functional as F

import bn_train_report as bnr
import capf_oracle as oracle
from capf import lib as capf
from capf import synth

pytestmark = pytest.mark.gpu

ROWS = (2, 3, 63, 64, 65, 4097, 8 * 64 * 64)
CHANNELS = (32, 48, 64, 96, 128, 192, 256, 384)


# ---- 5. the stand-alone ops against torch in fp64 ------------------------------------------------------------------------------
def _bn_case(x, gamma, beta, rm, rv, res, relu, momentum=0.1, eps=1e-5):
    """(out, running_mean, running_var) of torch's train-mode batch norm (+ residual) (ReLU) on x [rows, C], in x's dtype"""
    rm, rv = rm.clone(), rv.clone()
    y = F.batch_norm(x.t().unsqueeze(0), rm, rv, gamma, beta, True, momentum, eps)[0].t()      # [1, C, rows]: statistics over rows
    if res is not None:
        y = y + res
    if relu:
        y = F.relu(y)
    return y, rm, rv


def _run_op(x, gamma, beta, rm, rv, res, relu, in_place, track):
    xd = x.cuda()
    rmd, rvd = (rm.cuda(), rv.cuda()) if track else (None, None)
    scale, shift = capf.bn_stats(xd, gamma.cuda(), beta.cuda(), 1e-5, 0.1, rmd, rvd)
    y = capf.bn_apply(xd, scale, shift, res.cuda() if res is not None else None, relu, out=xd if in_place else None)
    torch.cuda.synchronize()
    return y.cpu(), (rmd.cpu() if track else None), (rvd.cpu() if track else None), scale.cpu(), shift.cpu()


def _check_op(tag, x, gamma, beta, rm, rv, res, relu, in_place, track):
    d = lambda t: t.double() if t is not None else None
    want = _bn_case(d(x), d(gamma), d(beta), d(rm), d(rv), d(res), relu)
    ref32 = _bn_case(x, gamma, beta, rm, rv, res, relu)
    got = _run_op(x, gamma, beta, rm, rv, res, relu, in_place, track)
    ratios = []
    for name, g, w, r in zip(("out", "running_mean", "running_var"), got, want, ref32):
        if g is None:
            continue
        assert torch.isfinite(g).all(), (tag, name)
        d32 = (r.double() - w).abs().max().item()
        err = (g.double() - w).abs().max().item()
        bound = 4.0 * d32 + 1e-6 * w.abs().max().item()
        ratios.append((name, err / max(d32, 1e-300), err, bound))
        assert err <= bound, (tag, name, err, d32, bound)
    return ratios


@pytest.mark.parametrize("C", CHANNELS)
def test_bn_ops_against_fp64(C):
    g = torch.Generator().manual_seed(100 + C)
    worst = {}
    for k, rows in enumerate(ROWS):
        x = torch.randn(rows, C, generator=g) * (0.5 + 2.0 * torch.rand(C, generator=g)) + 3.0 * torch.randn(C, generator=g)
        gamma, beta = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g)
        rm, rv = torch.randn(C, generator=g), 0.5 + torch.rand(C, generator=g)
        res = torch.randn(rows, C, generator=g)
        for v in range(2):      # with / without residual + ReLU, in place / out of place, statistics tracked / NULL: every option both ways per size pair
            with_res, relu, in_place, track = bool((k + v) & 1), bool((k + v) & 1), bool(v), bool((k >> 1) + v & 1) or rows == ROWS[-1]
            for name, ratio, err, bound in _check_op(f"rows {rows} C {C} v{v}", x, gamma, beta, rm, rv, res if with_res else None, relu, in_place, track):
                worst[name] = max(worst.get(name, 0.0), ratio)
    print(f"  C {C}: worst error / d32 " + ", ".join(f"{k} {v:.2f}" for k, v in worst.items()))


@pytest.mark.parametrize("mean,spread", [(1e3, 1.0), (1e-3, 1e-5)])
def test_bn_ops_mean_far_above_spread(mean, spread):
    """Raw conv outputs are not centred: a plain fp32 E[x^2] - E[x]^2 loses the variance here (1e6 - 1e6 at unit spread)."""
    g = torch.Generator().manual_seed(7)
    for rows, C in ((4097, 64), (8 * 64 * 64, 32)):
        x = mean + spread * torch.randn(rows, C, generator=g)
        gamma, beta = 0.5 + torch.rand(C, generator=g), torch.randn(C, generator=g)
        rm, rv = torch.zeros(C), torch.ones(C)
        for name, ratio, err, bound in _check_op(f"mean {mean} spread {spread} rows {rows}", x, gamma, beta, rm, rv, None, False, False, True):
            print(f"  mean {mean:g} spread {spread:g} rows {rows} {name}: error {err:.3e} = {ratio:.2f} x d32 (bound {bound:.3e})")
        # the variance itself, from running_var with momentum 1: within 1e-5 of the fp64 variance (a cancelling sum is off by O(1))
        rvd = torch.ones(C).cuda()
        lib = capf.load_library()
        xd = x.cuda()
        nbytes = lib.capf_op_bn_stats_scratch_bytes(rows, C)
        scratch = torch.empty(nbytes // 8, dtype=torch.float64, device="cuda")
        sc, sh = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        capf._call("capf_op_bn_stats", capf._stream(xd), capf._p(xd), rows, C, capf._p(gamma.cuda()), capf._p(beta.cuda()), 1e-5, 1.0, None, capf._p(rvd),
                   capf._p(sc), capf._p(sh), capf._p(scratch), nbytes)
        var64 = x.double().var(0, unbiased=True)
        assert ((rvd.cpu().double() - var64).abs() / var64).max().item() < 1e-5


def test_bn_ops_refusals_and_repeat():
    x = torch.randn(1, 32).cuda()
    ones = torch.ones(32).cuda()
    with pytest.raises(capf.CapfError):                 # n = 1: "Expected more than 1 value per channel when training"
        capf.bn_stats(x, ones, ones)
    with pytest.raises(capf.CapfError):                 # C % 4 != 0
        capf.bn_stats(torch.randn(8, 30).cuda(), ones[:30], ones[:30])
    x = (5.0 + torch.randn(4097, 96, generator=torch.Generator().manual_seed(3))).cuda()
    g, b = torch.rand(96).cuda(), torch.rand(96).cuda()
    runs = []
    for _ in range(2):
        rm, rv = torch.zeros(96).cuda(), torch.ones(96).cuda()
        sc, sh = capf.bn_stats(x, g, b, 1e-5, 0.1, rm, rv)
        runs.append((sc.cpu(), sh.cpu(), rm.cpu(), rv.cpu(), capf.bn_apply(x, sc, sh, None, True).cpu()))
    for a, c in zip(*runs):
        assert torch.equal(a, c)


# ---- 6 - 9. the backbone ---------------------------------------------------------------------------------------------------------
def _model(backbone, mpi=True, backbone_bn="batch", wseed=0):
    from mvn.utils.cfg import backbone_preset, config
    with contextlib.redirect_stdout(io.StringIO()):
        if mpi:
            from model.conpose import VolumetricTriangulationNet, mpi_preset
            m = VolumetricTriangulationNet(mpi_preset(copy.deepcopy(config), backbone), backbone_bn=backbone_bn)
        else:
            from mvn.models.conpose import CA_PF
            cfg = backbone_preset(copy.deepcopy(config), backbone)
            cfg.model.backbone.fix_weights = True
            m = CA_PF(cfg, backbone_bn=backbone_bn)
    sd = synth.load_synthetic(m, seed=wseed, bn_mode="random")
    return m.cuda(), {k: v.clone() for k, v in sd.items()}


def _frames(B, H, W, step):
    return synth.synth_inputs(B, H, W, seed=40 + step)


_REF = {}


def _reference(backbone, B, H, W):
    """fp64 and fp32 oracle runs of three train-mode forwards: maps per step and the final running statistics.  Computed once per case."""
    key = (backbone, B, H, W)
    if key not in _REF:
        _, sd = _model(backbone)
        out = []
        for P in (bnr.to_double(sd), bnr.clone_sd(sd)):
            maps = [bnr.train_maps(P, _frames(B, H, W, s)[0], backbone) for s in range(3)]
            out.append((maps, {k: P[k] for k in P if k.endswith(("running_mean", "running_var")) and k.startswith("backbone.")}))
        _REF[key] = out
    return _REF[key]


def _three_steps(backbone, B, H, W, lanes=None, guard=False, mpi=True):
    """Three train-mode forwards through the host module (no grad): maps after each, the backbone's buffers at the end."""
    import workspace_guard
    m, _ = _model(backbone, mpi=mpi)
    m.train()
    maps, ws = [], None
    with torch.no_grad():
        for s in range(3):
            img, k2d, kc = _frames(B, H, W, s)
            if s == 0:
                eng = m.engine_for(img.cuda())
                if lanes is not None:
                    eng.set_lanes(lanes)
                if guard:
                    ws = workspace_guard.install(eng, B, 0xFF)
            m(img.cuda(), k2d.cuda(), kc.cuda())
            torch.cuda.synchronize()
            maps.append([eng.tensor(f"feat{l}")[:B].permute(0, 3, 1, 2).contiguous().cpu() for l in range(4)])
    if ws is not None:
        ws.check("workspace after three batch-statistics forwards")
    stats = {"backbone." + n: b.detach().cpu().clone() for n, b in m.backbone.named_buffers()}
    return maps, stats


def _check_against_fp64(tag, backbone, B, H, W, maps, stats):
    (maps64, st64), (maps32, st32) = _reference(backbone, B, H, W)
    worst_map = worst_stat = 0.0
    for s in range(3):
        for l in range(4):
            w = maps64[s][l]
            d32 = (maps32[s][l].double() - w).abs().max().item()
            err = (maps[s][l].double() - w).abs().max().item()
            bound = 4.0 * d32 + 1e-5 * w.abs().max().item()
            worst_map = max(worst_map, err / bound)
            assert torch.isfinite(maps[s][l]).all() and err <= bound, (tag, "step", s, "feat", l, err, d32, bound)
    assert len(st64) == 2 * 292
    for k, w in st64.items():
        d32 = (st32[k].double() - w).abs().max().item()
        err = (stats[k].double() - w).abs().max().item()
        bound = 4.0 * d32 + 1e-5 * w.abs().max().item()
        worst_stat = max(worst_stat, err / bound)
        assert err <= bound, (tag, k, err, d32, bound)
    nbt = [v for k, v in stats.items() if k.endswith("num_batches_tracked")]
    assert len(nbt) == 292 and all(int(v) == 3 for v in nbt)
    print(f"  {tag}: worst error / bound: maps {worst_map:.3f}, running statistics {worst_stat:.3f}")


CASES = [("hrnet_32", 2, 64, 64), ("hrnet_32", 5, 64, 64), ("hrnet_32", 3, 96, 64), ("hrnet_48", 2, 64, 64)]
_RUNS = {}


def _default_run(case):
    if case not in _RUNS:
        _RUNS[case] = _three_steps(*case)
    return _RUNS[case]


@pytest.mark.parametrize("case", CASES, ids=lambda c: "{}-b{}-{}x{}".format(*c))
def test_backbone_bn_against_fp64(case):
    maps, stats = _default_run(case)
    _check_against_fp64("{} batch {} {}x{}".format(*case), *case, maps, stats)
    # and nowhere near the running-statistics route: at least 0.5 of the map's maximum away
    m, _ = _model(case[0])
    m.train(); m.backbone.eval()
    img, k2d, kc = _frames(case[1], case[2], case[3], 0)
    with torch.no_grad():
        m(img.cuda(), k2d.cuda(), kc.cuda())
    eng = m.engine_for(img.cuda())
    for l in range(4):
        run = eng.tensor(f"feat{l}")[:case[1]].permute(0, 3, 1, 2).cpu()
        assert bnr.rel_dist(run, maps[0][l]) >= 0.5


def _same_bits(a, b):
    (ma, sa), (mb, sb) = a, b
    for s in range(3):
        for l in range(4):
            assert torch.equal(ma[s][l], mb[s][l]), ("step", s, "feat", l)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_backbone_bn_reproducible_on_a_fresh_engine():
    case = CASES[1]
    _same_bits(_default_run(case), _three_steps(*case))


@pytest.mark.parametrize("lanes", [0, 2, 3])
def test_backbone_bn_same_bits_in_every_lane_mode(lanes):
    case = CASES[0]
    _same_bits(_default_run(case), _three_steps(*case, lanes=lanes))


def test_backbone_bn_with_context_blocks_on_a_guarded_workspace():
    """The H36M model (context blocks), on the exact-size, banded, NaN-filled workspace."""
    case = CASES[0]
    maps, stats = _three_steps(*case, guard=True, mpi=False)
    _check_against_fp64("guarded, context blocks", *case, maps, stats)


def test_backbone_bn_refusals_touch_nothing():
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    m, sd = _model("hrnet_32")
    m.train()
    img, k2d, kc = _frames(2, 64, 64, 0)
    with torch.no_grad():
        m(img.cuda(), k2d.cuda(), kc.cuda())
    eng = m.engine_for(img.cuda())
    torch.cuda.synchronize()
    gen = eng.train_generation()
    before = {n: b.clone() for n, b in m.backbone.named_buffers()}
    maps = [eng.tensor(f"feat{l}") for l in range(4)]
    stream = torch.cuda.current_stream().cuda_stream
    lib, P = eng.lib, capf.c_void_p
    imgd = img.cuda()
    assert lib.capf_backbone_forward_bn(eng.h, P(stream), P(imgd.data_ptr()), 0, 0.1) == -1
    assert lib.capf_backbone_forward_bn(eng.h, P(stream), P(imgd.data_ptr()), eng.cfg.max_batch + 1, 0.1) == -1
    assert lib.capf_backbone_forward_bn(eng.h, P(stream), None, 2, 0.1) == -1
    torch.cuda.synchronize()
    assert eng.train_generation() == gen
    for n, b in m.backbone.named_buffers():
        assert torch.equal(b, before[n]), n
    for l in range(4):
        assert torch.equal(eng.tensor(f"feat{l}"), maps[l])
    # n < 2: batch 1 at a 32x32 crop, where the deepest map is 1x1
    small = m.engine_for(torch.zeros(1, 32, 32, 3, device="cuda"))
    small.ensure_workspace(2)
    g2 = small.train_generation()
    with pytest.raises(capf.CapfError, match="more than 1 value per channel"):
        small.backbone_forward_bn(torch.zeros(1, 32, 32, 3, device="cuda"), stream)
    assert small.train_generation() == g2
    # no workspace: CAPF_ERR_STATE, as for every run entry
    small._check(lib.capf_set_workspace(small.h, None, 0), "set_workspace")
    g3 = small.train_generation()
    two = torch.zeros(2, 32, 32, 3, device="cuda")
    assert lib.capf_backbone_forward_bn(small.h, P(stream), P(two.data_ptr()), 2, 0.1) == -4
    assert "workspace" in lib.capf_last_error(small.h).decode() and small.train_generation() == g3
    torch.cuda.synchronize()
    for n, b in m.backbone.named_buffers():
        assert torch.equal(b, before[n]), n
    # a handle without the flag: CAPF_ERR_STATE naming it; one without parameters or workspace: CAPF_ERR_STATE
    plain, _ = _model("hrnet_32", backbone_bn="running")
    pe = plain.engine_for(imgd)
    pe.ensure_workspace(2)
    with pytest.raises(capf.CapfError, match="CAPF_PLAN_BN_BATCH_STATS"):
        pe.backbone_forward_bn(imgd, stream)
    cfg = backbone_preset(copy.deepcopy(config), "hrnet_32")
    bare = capf.Engine(_native.make_capf_config(cfg, 64, 64, plan_flags=capf.PLAN_BN_BATCH_STATS), device=0)
    assert bare.lib.capf_backbone_forward_bn(bare.h, P(stream), P(imgd.data_ptr()), 2, 0.1) == -4


# ---- 8. composition --------------------------------------------------------------------------------------------------------------
def test_bn_backbone_then_training_step_against_fp64():
    """capf_backbone_forward_bn + capf_lifter_forward_train + capf_backward at batch 5 (fixed DropPath multipliers): prediction, loss and
    every gradient against the fp64 lifter on the engine's own maps, at test_gpu_mpi_train's bounds."""
    import test_gpu_mpi_train as mt
    B = 5
    m, _ = _model("hrnet_32")
    m.train()
    m.drop_path_rate = 0.2
    img, k2d, kc, gt = synth.synth_inputs(B, 64, 64, seed=21, with_gt=True)
    torch.manual_seed(5)
    masks = {}
    real = m._drop_masks
    m._drop_masks = lambda n, dev: masks.setdefault("m", real(n, dev))
    pred, loss, ref = mt._step(m, img, k2d, kc, gt)
    eng = m.engine_for(img.cuda())
    assert all(int(b) == 1 for n, b in m.backbone.named_buffers() if n.endswith("num_batches_tracked"))
    mt._check("bn backbone + training step, batch 5", m, eng, B, 4, k2d, ref, gt, pred, loss, masks["m"])


def test_host_two_steps_then_eval_refolds_the_moved_statistics():
    """Two AdamW steps in .train() with backbone_bn='batch', then .eval(): one forward equals the oracle's eval forward on the UPDATED
    state dict -- which fails if the folded packs are not rebuilt from the moved running statistics."""
    import test_gpu_mpi_train as mt
    from test_gpu_parity import TOL_OUT
    B = 4
    m, _ = _model("hrnet_32")
    m.train()
    m.drop_path_rate = 0.0
    opt = torch.optim.AdamW(m.volume_net.parameters(), lr=1e-4, weight_decay=0.1)
    for s in range(2):
        img, k2d, kc, gt = synth.synth_inputs(B, 64, 64, seed=60 + s, with_gt=True)
        opt.zero_grad()
        mt._step(m, img, k2d, kc, gt)
        opt.step()
    m.eval()
    img, k2d, kc = synth.synth_inputs(B, 64, 64, seed=70)
    with torch.no_grad():
        got, _ = m(img.cuda(), k2d.cuda(), kc.clone().cuda())
        sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
        ref = oracle.normalise_crop_keypoints_(kc.clone())
        feats = oracle.hrnet_forward(sd, img.permute(0, 3, 1, 2).contiguous())
        want = oracle.lifter_forward(sd, k2d, ref, feats, context_blocks=False, depth=4)
    got = got.permute(0, 2, 3, 4, 1).reshape(B, 1, 17, 3).cpu()
    assert all(int(v) == 2 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    err = (got - want.reshape(B, 1, 17, 3)).abs().max().item()
    print(f"  eval after two batch-statistics steps: max|hip - oracle| {err:.3e}")
    assert err <= TOL_OUT, err


def test_eval_backbone_before_any_step_equals_the_default_module():
    a, _ = _model("hrnet_32", backbone_bn="batch")
    b, _ = _model("hrnet_32", backbone_bn="running")
    img, k2d, kc = synth.synth_inputs(3, 64, 64, seed=80)
    outs = []
    for m in (a, b):
        m.train(); m.backbone.eval()
        with torch.no_grad():
            outs.append(m(img.cuda(), k2d.cuda(), kc.clone().cuda())[0].cpu())
    assert torch.equal(outs[0], outs[1])
