"""GPU: where the engine writes and what else it reads -- every plan on an exact-size, banded, poisoned workspace (tests/workspace_guard.py).

include/capf.h: the workspace is caller-owned, capf_set_workspace invalidates whatever the engine kept in it.  So every call sequence must
give the same bits whatever the workspace held before, and must write nothing outside [ptr, ptr + capf_workspace_bytes(batch)).  Here the
workspace is exactly that many bytes between two 4 MiB bands, filled with 0x00 / 0xFF / 0x7F (0 / NaN / 3.39e38, fp16: NaN) before each
call sequence; every input is a copy whose last element is followed by band bytes equal to the fill, every output starts as the fill.

* a store past the arena, an input or an output changes a band byte: check() names its offset;
* a read of workspace bytes no earlier op of the SAME call wrote, or past an operand's end, that reaches a result makes the result depend on
  the fill: outputs are compared bit for bit across the three fills (0 * NaN = NaN, and the two-piece kernels take their block scale from
  what they read);
* an int32 region read before it is written would index with -1 / 2139062143.

No tolerance of its own: everything is torch.equal, except the atomic map gradient (not reproducible by design), which is held to the
ordered one within test_gpu_features.py's GRAD_L2_BOUND / GRAD_MAX_BOUND.  Every fixed number is a condition: the 4 MiB band, the three fill
bytes, the rows and batches."""
import functools

import pytest
import torch

import capf_oracle as oracle
import small_geometry_cases as sg
import workspace_guard as wg
from capf import synth
from capf.lib import PLAN_NO_BATCHED_REDUCE
from test_gpu_fullsize import _model

pytestmark = pytest.mark.gpu

FILLS = wg.FILLS
J = 17

# ---- rows ------------------------------------------------------------------------------------------------------------------------------------
# every (plan, batch) row of small_geometry_cases.py, plus the two fp32 plans it has none of: the three exact bf16 pieces and the fp32 matrix
# pipe (CAPF_PLAN_NO_F32X3 | CAPF_PLAN_NO_F32H2_GEMM: every conv and linear on igemm_f32 / Winograd), at batches on both sides of 5 and 24
# and one ragged tile batch
EXTRA = [sg.Row("hrnet_32", 64, 64, "fp32", fl, B, (), ()) for fl in ("F32X3_EXACT", "NO_F32X3|NO_F32H2_GEMM") for B in (4, 24, 83)]
ROWS = list(sg.ROWS) + EXTRA
ROW_IDS = [sg.row_id(r) for r in ROWS]
COVERED = set()           # what the tests below actually ran, for test_coverage


def _stream():
    return torch.cuda.current_stream().cuda_stream


@functools.lru_cache(maxsize=None)
def _plan_model(backbone, dtype, plan_flags):
    """one host model per plan for the whole module (its engines are per crop size); weights as test_gpu_small_geometry.test_end_to_end"""
    return _model(backbone, dtype, 21, sg.flag_bits(plan_flags))[0]


def _inference_engine(model, H, W):
    """a handle of the model's plan with training = 0: its workspace is the inference arena alone, so the arena's end IS the trailing band
    (the host model's own handles are training = 1 wherever the plan allows: there the training region lies behind the arena, and a store
    past the arena's end would land in it unseen).  Bound to the model's parameters like CA_PF._engine_at does."""
    from capf.lib import Engine
    from mvn.models import _native
    cache = model.__dict__.setdefault("_hygiene_engines", {})
    if (H, W) not in cache:
        cfg = _native.make_capf_config(model._config, H, W, context_blocks=model.context_blocks, compute_dtype=model.compute_dtype,
                                       plan_flags=model.plan_flags)
        cfg.training = 0
        eng = Engine(cfg, device=torch.cuda.current_device())
        eng.bind_state({k: v.data for k, v in model.state_dict(keep_vars=True).items()}, _stream())
        cache[(H, W)] = eng
    return cache[(H, W)]


def _inputs(row_or_B, H=None, W=None, seed=22):
    if H is None:
        row_or_B, H, W = row_or_B.batch, row_or_B.H, row_or_B.W
    return synth.synth_inputs(row_or_B, H, W, seed=seed, crop_range=(W, H))


def _want_kcrop(kc):
    ref = kc.clone()
    oracle.normalise_crop_keypoints_(ref)
    return ref


def _call(eng, ws, fill, host_inputs, run):
    """one poisoned call sequence: refill the workspace, flush the inputs against band bytes == fill, pre-fill the output with the fill,
    run(eng, img, k2d, kc, out), check every band; -> (out, kcrop) clones"""
    ws.refill(fill)
    img, k2d, kc = (wg.flush(t.cuda(), fill) for t in host_inputs)
    out = wg.filled((img.shape[0], 1, J, 3), torch.float32, "cuda", fill)
    run(eng, img, k2d, kc, out)
    ws.check(f"workspace under fill 0x{fill:02X}")
    wg.check_all((img, k2d, kc, out), f"(images, k2d, kcrop, out) under fill 0x{fill:02X}")
    return out.clone(), kc.clone()


def _same_bits(results, tag):
    (o0, k0) = results[0]
    assert bool(torch.isfinite(o0).all()), f"{tag}: non-finite output under fill 0x{FILLS[0]:02X}"
    for fill, (o, k) in zip(FILLS[1:], results[1:]):
        assert bool(torch.isfinite(o).all()), f"{tag}: non-finite output under fill 0x{fill:02X}"
        bad = (o.view(torch.int32) != o0.view(torch.int32)).flatten(1).any(dim=1).nonzero().flatten().tolist()
        assert not bad, f"{tag}: the output depends on the workspace fill (0x{fill:02X} vs 0x00) in frames {bad[:8]} ({len(bad)} of {o.shape[0]})"
        assert torch.equal(k, k0), f"{tag}: kcrop depends on the fill"


def _forward(eng, img, k2d, kc, out):
    eng.forward(img, k2d, kc, out, _stream())


def _two_calls(eng, img, k2d, kc, out):
    eng.backbone_forward(img, _stream())
    eng.lifter_forward(k2d, kc, out, _stream())


def _note(row, *what):
    tags = {"fp32": "default fp32 plan", "bf16": "bf16", "fp16": "fp16"}
    plan = {"0": tags[row.dtype], "BF16_F32_STREAM": "BF16_F32_STREAM", "F32X3_EXACT": "CAPF_PLAN_F32X3_EXACT",
            "NO_F32X3|NO_F32H2_GEMM": "fp32 matrix pipe"}[row.plan_flags]
    if row.backbone == "cpn":
        plan = f"CPN {row.dtype}"
    for w in what:
        COVERED.add((plan, w))


# ---- forward, every row --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_forward_is_blind_to_the_workspace_fill_and_stays_inside(row):
    """capf_forward on an inference-only handle (training = 0: the arena ends at the band) under the three fills: `out` bit-identical and
    finite (fp16 saturates, it does not overflow), kcrop the reference normalisation bit for bit, all bands intact"""
    model = _plan_model(row.backbone, row.dtype, row.plan_flags)
    host = _inputs(row)
    with torch.no_grad():
        eng = _inference_engine(model, row.H, row.W)
        assert eng.cfg.training == 0
        ws = wg.install(eng, row.batch, FILLS[0])
        assert ws.nbytes == eng.workspace_bytes(row.batch) and eng._ws.numel() * 4 == ws.nbytes
        res = [_call(eng, ws, f, host, _forward) for f in FILLS]
    _same_bits(res, sg.row_id(row))
    assert torch.equal(res[0][1].cpu(), _want_kcrop(host[2]))
    _note(row, "forward")


@pytest.mark.parametrize("row", ROWS, ids=ROW_IDS)
def test_backbone_then_lifter_as_two_calls(row):
    """capf_backbone_forward + capf_lifter_forward on the host model's own handle (training = 1 except fp16) with ONE refill before the
    pair: the same assertions, and the same bits as capf_forward"""
    model = _plan_model(row.backbone, row.dtype, row.plan_flags)
    host = _inputs(row)
    with torch.no_grad():
        eng = model.engine_for(host[0].cuda())
        ws = wg.install(eng, row.batch, FILLS[0])
        res = [_call(eng, ws, f, host, _two_calls) for f in FILLS]
        one = _call(eng, ws, 0xFF, host, _forward)
    _same_bits(res, sg.row_id(row))
    assert torch.equal(res[0][1].cpu(), _want_kcrop(host[2]))
    assert torch.equal(one[0], res[0][0])
    _note(row, "two calls")


# ---- lane modes ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone,H,W,dtype,B", sg.SCHEDULES, ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[3]}-B{c[4]}" for c in sg.SCHEDULES])
def test_lane_modes_on_a_poisoned_workspace(backbone, H, W, dtype, B):
    """capf_set_lanes 0 / 2 / 3 under 0xFF: bit-identical to each other and to the 0x00 run; mode 1 (side streams, no split-K scratch) only
    to itself across the fills"""
    model = _plan_model(backbone, dtype, "0")
    host = _inputs(B, H, W, seed=5)
    with torch.no_grad():
        eng = model.engine_for(host[0].cuda())
        ws = wg.install(eng, B, FILLS[0])
        try:
            base = _call(eng, ws, 0x00, host, _forward)
            got = {}
            for mode in (0, 2, 3):
                eng.set_lanes(mode)
                got[mode] = _call(eng, ws, 0xFF, host, _forward)
            eng.set_lanes(1)
            side = [_call(eng, ws, f, host, _forward) for f in FILLS]
        finally:
            eng.set_lanes(3)
    for mode in (0, 2, 3):
        assert bool(torch.isfinite(got[mode][0]).all())
        assert torch.equal(got[mode][0], base[0]) and torch.equal(got[mode][1], base[1]), f"capf_set_lanes({mode}) under 0xFF vs the 0x00 run"
    _same_bits(side, "capf_set_lanes(1)")
    COVERED.add(("lanes", f"{dtype}"))


# ---- training ----------------------------------------------------------------------------------------------------------------------------------
# (lifter width, (H, W), batch, DropPath): HRNet-32 at 32 x 64 and 64 x 64; widths 32, 96, 288; batches 2, 5 (H2G_MIN_BATCH), 13, 100 -- width
# 32 at batch 100 is the case whose tA / tB overrun commit b5aee0f fixed; each width once without and once with DropPath masks
TRAIN = [(32, (32, 64), 100, 0.0), (32, (64, 64), 2, 0.2), (96, (32, 64), 5, 0.2), (96, (64, 64), 13, 0.0), (288, (32, 64), 13, 0.2),
         (288, (64, 64), 2, 0.0)]


def _release(model):
    for e in model._engines.values():
        e.close()
    model._engines.clear()
    torch.cuda.empty_cache()


def _train_mode(model, drop):
    model.train(); model.backbone.eval(); model.volume_net.train()
    model.drop_path_rate = drop
    return model


def _masks(model, B, drop):
    if not drop:
        return None
    torch.manual_seed(7)
    m = model._drop_masks(B, torch.device("cuda"))
    assert m is not None and bool((m == 0).any())
    return m


def _train_steps(model, B, H, W, drop, tag, seed=62):
    """capf_forward_train + capf_backward under the three fills, one refill before the pair; flat_grad starts as NaN (every element is
    written exactly once: no NaN may survive); -> (out, flat_grad) of the 0x00 run"""
    img, k2d, kc, _ = synth.synth_inputs(B, H, W, seed=seed + B, crop_range=(W, H), with_gt=True)
    dout = torch.randn(B, 1, J, 3, generator=torch.Generator().manual_seed(3))
    eng = model.engine_for(img.cuda())
    masks = _masks(model, B, drop)
    _, total = eng.grad_layout_cached()
    ws = wg.install(eng, B, FILLS[0])
    first = None
    for fill in FILLS:
        ws.refill(fill)
        i, k, c, d = (wg.flush(t.cuda(), fill) for t in (img, k2d, kc, dout))
        m = wg.flush(masks, fill) if masks is not None else None
        out = wg.filled((B, 1, J, 3), torch.float32, "cuda", fill)
        flat = wg.filled((total,), torch.float32, "cuda", 0xFF)
        eng.forward_train(i, k, c, out, _stream(), m)
        eng.backward(d, flat, _stream(), m)
        ws.check(f"{tag}: training workspace under fill 0x{fill:02X}")
        wg.check_all([t for t in (i, k, c, d, m, out, flat) if t is not None], f"{tag}: (images, k2d, kcrop, dout, masks, out, flat_grad) under 0x{fill:02X}")
        assert bool(torch.isfinite(out).all()), f"{tag}: non-finite prediction under fill 0x{fill:02X}"
        n_nan = int(torch.isnan(flat).sum())
        assert n_nan == 0, f"{tag}: {n_nan} of {total} flat_grad elements are NaN under fill 0x{fill:02X} (first at {int(torch.isnan(flat).nonzero()[0, 0])})"
        if first is None:
            first = (out.clone(), flat.clone(), c.clone())
        else:
            assert torch.equal(out, first[0]), f"{tag}: the prediction depends on the fill (0x{fill:02X} vs 0x00)"
            same = flat.view(torch.int32) == first[1].view(torch.int32)
            assert bool(same.all()), (f"{tag}: flat_grad depends on the fill (0x{fill:02X} vs 0x00): {int((~same).sum())} elements, "
                                      f"first at {int((~same).nonzero()[0, 0])}")
            assert torch.equal(c, first[2])
    assert torch.equal(first[2].cpu(), _want_kcrop(kc))
    return first[0], first[1]


@pytest.mark.parametrize("E,hw,B,drop", TRAIN, ids=[f"E{c[0]}-{c[1][0]}x{c[1][1]}-B{c[2]}" + ("-droppath" if c[3] else "") for c in TRAIN])
def test_training_step_on_a_poisoned_workspace(E, hw, B, drop):
    """training = 1 handles, both settings of CAPF_PLAN_NO_BATCHED_REDUCE (include/capf.h: identical bits)"""
    from lifter_models import lifter_model
    H, W = hw
    got = []
    for flags in (0, PLAN_NO_BATCHED_REDUCE):
        model = _train_mode(lifter_model("hrnet_32", embed=E, plan_flags=flags, wseed=61 + E)[0], drop)
        try:
            assert model.volume_net.Spatial_pos_embed.shape[-1] == E
            got.append(_train_steps(model, B, H, W, drop, f"E={E} {H}x{W} B={B} DropPath {drop} flags {flags}"))
        finally:
            _release(model)
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][1], got[1][1]), "CAPF_PLAN_NO_BATCHED_REDUCE changes bits"
    COVERED.update({("train", f"E{E}"), ("train", f"B{B}"), ("train", f"{H}x{W}"), ("train", "droppath" if drop else "no droppath"),
                    ("train", "CAPF_PLAN_NO_BATCHED_REDUCE")})


def test_mpi_training_step_on_a_poisoned_workspace():
    """the MPI-INF-3DHP variant (no context blocks; embed 64, depth 2) through test_gpu_mpi_train's model helper"""
    from test_gpu_mpi_train import _model as mpi_model
    model = mpi_model("hrnet_32", 2, wseed=80)
    try:
        assert model.volume_net.Spatial_pos_embed.shape[-1] == 64
        _train_steps(model, 13, 64, 64, 0.0, "MPI-INF-3DHP embed 64 depth 2 64x64 B=13")
    finally:
        _release(model)
    COVERED.add(("train", "MPI-INF-3DHP"))


# ---- caller-supplied maps ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,drop", [(2, 0.0), (6, 0.2)], ids=["B2", "B6-droppath"])
def test_caller_supplied_maps_on_a_poisoned_workspace(B, drop):
    """capf_set_features + capf_lifter_forward_train + capf_backward_maps at 32 x 64 (maps 8 x 16 .. 1 x 2).  Ordered mode: dfeat and flat_grad
    bit-identical across the fills.  Atomic mode: flat_grad bit-identical; dfeat (fp32 atomic adds, not reproducible) within
    test_gpu_features.py's GRAD_L2_BOUND / GRAD_MAX_BOUND of the ordered sum, the bit-reproducible form of the same gradient."""
    from test_gpu_features import _hrnet
    from train_yardstick import GRAD_L2_BOUND, GRAD_MAX_BOUND
    H, W = 32, 64
    model = _hrnet("hrnet_32", 51 + B, drop)
    try:
        img, k2d, kc, _ = synth.synth_inputs(B, H, W, seed=52 + B, crop_range=(W, H), with_gt=True)
        dout = torch.randn(B, 1, J, 3, generator=torch.Generator().manual_seed(3))
        eng = model.engine_for(img.cuda())
        masks = _masks(model, B, drop)
        _, total = eng.grad_layout_cached()
        ws = wg.install(eng, B, FILLS[0])
        eng.backbone_forward(img.cuda(), _stream())
        maps = [eng.tensor(f"feat{l}")[:B].contiguous() for l in range(4)]
        assert all(bool(torch.isfinite(m).all()) for m in maps)
        ordered = None
        for mode in (1, 0):
            eng.set_map_grad_mode(mode)
            first = None
            for fill in FILLS:
                ws.refill(fill)
                k, c, d = (wg.flush(t.cuda(), fill) for t in (k2d, kc, dout))
                fm = [wg.flush(m, fill) for m in maps]
                m = wg.flush(masks, fill) if masks is not None else None
                out = wg.filled((B, 1, J, 3), torch.float32, "cuda", fill)
                flat = wg.filled((total,), torch.float32, "cuda", 0xFF)
                dfeat = [wg.filled(t.shape, torch.float32, "cuda", fill) for t in maps]
                eng.set_features(fm, _stream())
                eng.lifter_forward_train(k, c, out, _stream(), m)
                eng.backward_maps(d, flat, dfeat, _stream(), m)
                tag = f"map-grad mode {mode} fill 0x{fill:02X}"
                ws.check(tag)
                wg.check_all([t for t in [k, c, d, m, out, flat] + fm + dfeat if t is not None], tag)
                assert bool(torch.isfinite(out).all()) and not bool(torch.isnan(flat).any()), tag
                assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in dfeat), tag
                if first is None:
                    first = (out.clone(), flat.clone(), [g.clone() for g in dfeat])
                    if mode == 1:
                        ordered = first
                    continue
                assert torch.equal(out, first[0]) and torch.equal(flat, first[1]), tag
                if mode == 1:
                    assert all(torch.equal(a, b) for a, b in zip(dfeat, first[2])), tag
            if mode == 0:
                assert torch.equal(first[0], ordered[0]) and torch.equal(first[1], ordered[1])
            for l, (g, t) in enumerate(zip(dfeat, ordered[2])):          # (mode 1: zero; mode 0: the last fill's atomic sum against the ordered one)
                dd = g.double() - t.double()
                l2, mx = float(dd.norm() / t.double().norm()), float(dd.abs().max() / t.abs().max())
                assert l2 <= GRAD_L2_BOUND and mx <= GRAD_MAX_BOUND, (mode, l, l2, mx)
    finally:
        _release(model)
    COVERED.update({("maps", "ordered"), ("maps", "atomic")})


# ---- debug and profiling entry points ------------------------------------------------------------------------------------------------------
DEBUG_ROWS = [("hrnet_32", 64, 64, "fp32", 24), ("hrnet_32", 64, 64, "bf16", 53)]


@pytest.mark.parametrize("backbone,H,W,dtype,B", DEBUG_ROWS, ids=[f"{c[0]}-{c[1]}x{c[2]}-{c[3]}-B{c[4]}" for c in DEBUG_ROWS])
def test_debug_prefix_and_profile_runs(backbone, H, W, dtype, B):
    """capf_set_debug(1) (the tap buffers join the arena: the workspace is sized after it), capf_forward_prefix at the end of the backbone
    and at one mid-region checkpoint of capf_op_describe, capf_forward_profile: bands intact; outputs / context maps bit-identical across fills"""
    model, _ = _model(backbone, dtype, 21)
    host = _inputs(B, H, W)
    try:
        with torch.no_grad():
            eng = model.engine_for(host[0].cuda())
            plain = eng.workspace_bytes(B)
            eng.set_debug(True)
            assert eng.workspace_bytes(B) >= plain
            ws = wg.install(eng, B, FILLS[0])
            res = [_call(eng, ws, f, host, _forward) for f in FILLS]
            _same_bits(res, "capf_set_debug(1)")
            taps = [eng.tensor(f"cidx{i}") for i in range(4)]                      # (under the last fill, 0x7F: NW corners inside the maps)
            assert all(int(t.min()) >= -1 and int(t.max()) < max(H, W) for t in taps)
            prof = lambda e, i, k, c, o: e.forward_profile(i, k, c, o, _stream())
            _same_bits([_call(eng, ws, f, host, prof) for f in FILLS], "capf_forward_profile")

            descs = [eng.op_describe(i) for i in range(eng.lib.capf_num_ops(eng.h))]
            n_backbone = sum(1 for d in descs if d.backbone)
            assert all(d.backbone for d in descs[:n_backbone]) and 0 < n_backbone < len(descs)
            # a prefix length after which the outputs of the ops that name it are still intact (a fork / join region keeps its buffers)
            cps = sorted({d.checkpoint for d in descs[:n_backbone] if d.kind in (0, 1) and 0 < d.checkpoint < n_backbone})
            for n_ops in (n_backbone, cps[len(cps) // 2]):
                last = max(i for i in range(n_backbone) if descs[i].kind in (0, 1) and descs[i].checkpoint == n_ops)
                d = descs[last]
                kept = []
                for fill in FILLS:
                    ws.refill(fill)
                    img = wg.flush(host[0].cuda(), fill)
                    eng.forward_prefix(img, n_ops, _stream())
                    ws.check(f"capf_forward_prefix({n_ops}) under 0x{fill:02X}")
                    wg.guard_of(img).check("images")
                    if n_ops == n_backbone:
                        kept.append([eng.tensor(f"feat{l}") for l in range(4)])
                    else:
                        kept.append([eng.op_tensor(last, 5, (B, d.Ho, d.Wo, d.Cout), d.out_dtype).clone()])
                for other in kept[1:]:
                    assert all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(kept[0], other)), f"capf_forward_prefix({n_ops})"
                if n_ops == n_backbone:
                    assert all(bool(torch.isfinite(t.float()).all()) for t in kept[0])
    finally:
        _release(model)
    COVERED.update({("debug", dtype), ("prefix", dtype), ("profile", dtype)})


# ---- what ran ------------------------------------------------------------------------------------------------------------------------------------
WANTED = ({(p, w) for p in ("default fp32 plan", "CAPF_PLAN_F32X3_EXACT", "fp32 matrix pipe", "bf16", "fp16", "BF16_F32_STREAM", "CPN fp32", "CPN bf16")
           for w in ("forward", "two calls")} |
          {("lanes", "fp32"), ("lanes", "bf16"), ("maps", "ordered"), ("maps", "atomic"), ("train", "MPI-INF-3DHP"),
           ("train", "CAPF_PLAN_NO_BATCHED_REDUCE"), ("train", "droppath"), ("train", "no droppath"), ("train", "32x64"), ("train", "64x64")} |
          {("train", f"E{e}") for e in (32, 96, 288)} | {("train", f"B{b}") for b in (2, 5, 13, 100)} |
          {(k, d) for k in ("debug", "prefix", "profile") for d in ("fp32", "bf16")})


def test_coverage():
    """the list of the module docstring, from the rows that actually ran (this test runs last: the whole module in one session)"""
    assert (32, (32, 64), 100, 0.0) in TRAIN                      # width 32 at batch 100: the tA / tB case
    assert any(r.backbone == "cpn" and r.dtype == "bf16" and any(p.startswith("bneck0_bf16") for p in r.expected_kernel_prefixes) for r in ROWS)
    missing = sorted(WANTED - COVERED)
    assert not missing, missing
