"""GPU: gradients w.r.t. the keypoints -- dL/d(k2d) and dL/d(ref) from capf_backward_points, and CA_PF's keypoint arguments under autograd.

Yardstick (points_grad_cases.points64): train_yardstick.lifter64's recipe -- capf_oracle.lifter_forward in float64, MPJPE, autograd, the
deformable samplers in the engine's cidx cells and on engine_clip_sides -- with k2d and ref as leaves; test_points_grad_api.py checks it
against central differences.  The context maps are feature_cases.synth_maps (white noise), handed over with capf_set_features.

Bounds: GRAD_L2_BOUND / GRAD_MAX_BOUND (2e-5 relative L2, 2e-5 of the float64 gradient's largest entry) for dk2d and dref wherever the
comparison is well conditioned: every case whose sampling_offsets parameters are scaled by 0.05 ("tame": the module initialises them near
zero).  There the same oracle evaluated in float32 sits 1.4e-6 .. 2.3e-6 from float64, fixed cells or free.
The UNSCALED synthetic weights ("wild": 19 % of the sampling coordinates clipped, |tanh| up to 0.99) on white-noise maps are a badly
conditioned function: the float32 oracle IN THE SAME CELLS AND ON THE SAME CLIP SIDES as the float64 one is 6.7e-4 (dk2d) / 2.2e-3 (dref)
away at B = 2, 7.1e-4 / 9.8e-4 at B = 6, its prediction 2.6e-4, its parameter gradients 1.5e-3 (measured on the CPU; fixing the cells
changes none of these, so it is roundoff amplified by the forward, not a one-sided derivative).  For that case the bound is therefore
4 x the floor, and the floor is computed here, per tensor and per measure, from the oracle alone: float32 against float64 in the engine's
cells and sides.  Nothing of the engine's result enters a bound."""
import pytest
import torch

import workspace_guard as wg
from conftest import make_model
from points_grad_cases import (HRNET32_32x32, MARGIN_PX, OFF_MAP_REF, WHOLLY_OUTSIDE_128x96, WHOLLY_OUTSIDE_32x32, case_inputs,
                               margin_px, normalise, off_map_, points64, rel_errors, small_inputs, tame_)
from train_yardstick import GRAD_L2_BOUND, GRAD_MAX_BOUND, engine_cells, engine_clip_sides

pytestmark = pytest.mark.gpu

FLOOR_LIMIT = 5e-6       # above this float32-vs-float64 distance of the oracle itself the bound is 4 x that distance
J = 17


def _dev():
    return torch.zeros(1, device="cuda").device


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _train_mode(model, drop=0.0):
    model.train(); model.backbone.eval(); model.volume_net.train()
    model.drop_path_rate = drop
    return model


def _model(wseed, tame=True, drop=0.0):
    model, _ = make_model("hrnet_32", device="cuda", wseed=wseed, bn="random")
    if tame:
        tame_(dict(model.volume_net.named_parameters()))
    return _train_mode(model, drop)


def _release(*models):
    for m in models:
        for e in m._engines.values():
            e.close()
        m._engines.clear()


def _params(model):
    return {"volume_net." + n: p for n, p in model.volume_net.named_parameters()}


def _masks(model, B, seed):
    torch.manual_seed(seed)
    masks = model._drop_masks(B, torch.device("cuda"))
    assert masks is not None and (masks == 0).any()
    return masks


def _mpjpe_grad(out, gt):
    from mvn.models.loss import MPJPE
    p = out.detach().clone().requires_grad_(True)
    loss = MPJPE()(p, gt.cuda())
    loss.backward()
    return loss.item(), p.grad.contiguous()


def _nhwc(maps):
    return [m.permute(0, 2, 3, 1).contiguous().cuda() for m in maps]


def _forward(eng, maps, k2d, kc, masks):
    """capf_set_features + capf_lifter_forward_train; returns (prediction, the normalised reference points, k2d) on the device.  The
    backward re-reads both keypoint buffers: the caller keeps them alive until its last backward of this step."""
    B = k2d.shape[0]
    k2d_dev, kc_dev, out = k2d.cuda(), kc.clone().cuda(), torch.empty(B, 1, J, 3, device="cuda")
    eng.set_features(_nhwc(maps), _stream())
    eng.lifter_forward_train(k2d_dev, kc_dev, out, _stream(), masks)
    return out, kc_dev, k2d_dev


def _step(eng, maps, k2d, kc, gt, masks, with_maps=False):
    """One training forward on `maps` and capf_backward_points; NaN-filled outputs, so an element the call did not write shows."""
    B = k2d.shape[0]
    out, ref, k2d_dev = _forward(eng, maps, k2d, kc, masks)
    loss, dout = _mpjpe_grad(out, gt)
    _, total = eng.grad_layout_cached()
    flat = torch.full((total,), float("nan"), device="cuda")
    dk2d, dref = torch.full((B, J, 2), float("nan"), device="cuda"), torch.full((B, J, 2), float("nan"), device="cuda")
    dfeat = [torch.full((B, h, w, c), float("nan"), device="cuda") for h, w, c in eng.feature_shapes()] if with_maps else None
    eng.backward_points(dout, flat, _stream(), masks, dfeat, dk2d, dref)
    torch.cuda.synchronize()
    for t in (out, flat, dk2d, dref) + tuple(dfeat or ()):
        assert torch.isfinite(t).all()
    return {"out": out, "loss": loss, "ref": ref.cpu(), "dout": dout, "flat": flat, "dk2d": dk2d, "dref": dref, "dfeat": dfeat,
            "keep": (ref, k2d_dev)}


def _hold(tag, got, want, l2_bound=GRAD_L2_BOUND, max_bound=GRAD_MAX_BOUND):
    """Print, then assert, the two measures of every lifter gradient test (train_yardstick.check_gradients)."""
    assert want.abs().max() > 0, tag
    l2, mx = rel_errors(got, want)
    print(f"    {tag}: relative L2 {l2:9.2e} (bound {l2_bound:.1e}) | max entry / max {mx:9.2e} (bound {max_bound:.1e})   "
          f"largest entry {want.abs().max().item():.3e}")
    assert l2 <= l2_bound and mx <= max_bound, (tag, l2, mx, l2_bound, max_bound)
    return l2, mx


def _yardstick(model, eng, got, maps, k2d, gt, masks, dtype=torch.float64):
    B = k2d.shape[0]
    return points64(_params(model), k2d, got["ref"], gt, maps, engine_cells(eng, B), masks, engine_clip_sides(eng, B), dtype=dtype)


def _engine(model, H=128, W=96):
    eng = model._engine_at(_dev(), H, W)
    eng.set_debug(True)                                       # cidx / cpos taps of the deformable samplers
    return eng


# ---- 1. tame weights: both sides of the batch-5 switch to the two-piece GEMM, with and without DropPath ----------------------------------
@pytest.mark.parametrize("B,drop", [(2, 0.0), (2, 0.2), (6, 0.0), (6, 0.2)], ids=["B2", "B2-droppath", "B6", "B6-droppath"])
def test_keypoint_gradients_vs_fp64_tame_weights(B, drop):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = _model(41 + B, tame=True, drop=drop)
    try:
        maps, k2d, kc, ref, gt = case_inputs(B)
        eng = _engine(model)
        masks = _masks(model, B, 7) if drop else None
        got = _step(eng, maps, k2d, kc, gt, masks)
        assert torch.equal(got["ref"], ref) and margin_px(got["ref"]) >= MARGIN_PX
        _, dk2d, dref, w64, l64 = _yardstick(model, eng, got, maps, k2d, gt, masks)
        perr = (got["out"].cpu().double() - w64).abs().max().item()
        print(f"  tame B={B} DropPath {drop}: prediction max|hip - fp64| {perr:.2e}, loss {got['loss']:.6f} vs {l64:.6f}")
        assert perr <= 1e-5 and abs(got["loss"] - l64) <= 1e-6 * abs(l64)
        _hold("dk2d", got["dk2d"], dk2d)
        _hold("dref", got["dref"], dref)
    finally:
        _release(model)


# ---- 2. wild weights: the border-clip mask at work; bound from the oracle's own float32 floor ------------------------------------------------
@pytest.mark.parametrize("B,drop", [(2, 0.0), (2, 0.2), (6, 0.0), (6, 0.2)], ids=["B2", "B2-droppath", "B6", "B6-droppath"])
def test_keypoint_gradients_vs_fp64_wild_weights(B, drop):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = _model(41 + B, tame=False, drop=drop)
    try:
        maps, k2d, kc, ref, gt = case_inputs(B)
        eng = _engine(model)
        masks = _masks(model, B, 7) if drop else None
        got = _step(eng, maps, k2d, kc, gt, masks)
        sides = engine_clip_sides(eng, B)
        clipped = 1.0 - sum(s.sum().item() for s in sides) / sum(s.numel() for s in sides)
        print(f"  wild B={B} DropPath {drop}: {100 * clipped:.1f} % of the sampling coordinates clipped to the border")
        assert clipped > 0.05
        _, dk64, dr64, w64, _ = _yardstick(model, eng, got, maps, k2d, gt, masks)
        _, dk32, dr32, w32, _ = _yardstick(model, eng, got, maps, k2d, gt, masks, dtype=torch.float32)
        print(f"    prediction: oracle fp32 vs fp64 {(w32.double() - w64).abs().max().item():.2e}, hip vs fp64 "
              f"{(got['out'].cpu().double() - w64).abs().max().item():.2e}")
        for name, g, t32, t64 in (("dk2d", got["dk2d"], dk32, dk64), ("dref", got["dref"], dr32, dr64)):
            fl2, fmx = rel_errors(t32, t64)
            b2 = GRAD_L2_BOUND if fl2 <= FLOOR_LIMIT else 4 * fl2
            bm = GRAD_MAX_BOUND if fmx <= FLOOR_LIMIT else 4 * fmx
            print(f"    {name}: floor (oracle fp32 vs fp64, the engine's cells and sides) {fl2:.2e} | {fmx:.2e}")
            _hold(name, g, t64, b2, bm)
    finally:
        _release(model)


# ---- 3. reference points off the map ---------------------------------------------------------------------------------------------------------
def test_reference_points_partly_and_wholly_outside_the_maps():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = _model(51, tame=True)
    try:
        maps, k2d, kc, _, gt = case_inputs(1)
        kc = off_map_(kc.clone())
        eng = _engine(model)
        got = _step(eng, maps, k2d, kc, gt, None)
        want = torch.tensor(OFF_MAP_REF)
        assert (got["ref"][0, :len(OFF_MAP_REF)] - want).abs().max() <= 1e-6 and margin_px(got["ref"]) >= MARGIN_PX
        _, dk2d, dref, _, _ = _yardstick(model, eng, got, maps, k2d, gt, None)
        _hold("dk2d", got["dk2d"], dk2d)
        _hold("dref", got["dref"], dref)
        # outside every map: no corner at the reference site, every deformable coordinate clipped -- exactly 0 on both sides
        for p in WHOLLY_OUTSIDE_128x96:
            axes = [a for a in (0, 1) if abs(OFF_MAP_REF[p][a]) > 2.4]            # (tanh moves a position by less than 1: still outside)
            for a in axes:
                assert dref[0, p, a] == 0 and got["dref"][0, p, a] == 0, (p, a, got["dref"][0, p])
    finally:
        _release(model)


# ---- 4. the smallest geometry: maps 8 x 8 .. 1 x 1 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
def test_smallest_geometry_with_a_1x1_map(B):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = _model(61 + B, tame=True)
    try:
        maps, k2d, kc, ref, gt = small_inputs(B)
        eng = _engine(model, 32, 32)
        assert eng.feature_shapes() == [(h, w, c) for c, h, w in HRNET32_32x32]
        got = _step(eng, maps, k2d, kc, gt, None, with_maps=True)             # (_step asserts that every output is finite)
        assert margin_px(got["ref"], HRNET32_32x32) >= MARGIN_PX
        _, dk2d, dref, _, _ = _yardstick(model, eng, got, maps, k2d, gt, None)
        _hold("dk2d", got["dk2d"], dk2d)
        _hold("dref", got["dref"], dref)
        # a point outside the 8 x 8, 4 x 4 and 2 x 2 maps: the 1 x 1 level is all that is left of it, and that contributes exactly 0 at
        # both sites (factor (size - 1) / 2 = 0, coordinate 0 <= 0 clipped)
        for p in WHOLLY_OUTSIDE_32x32:
            assert (dref[0, p] == 0).all() and (got["dref"][0, p] == 0).all(), got["dref"][0, p]
        assert got["dfeat"][3].abs().max() > 0                                # (the 1 x 1 map itself is sampled and has a gradient)
    finally:
        _release(model)


# ---- 5. the variant without context blocks: dref is the reference-site term alone ---------------------------------------------------------------
def test_variant_without_context_blocks():
    from test_gpu_features import _mpi
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B = 3
    m = _mpi(71, 2)
    try:
        assert m.volume_net.Spatial_pos_embed.shape[-1] == 64
        maps, k2d, kc, _, gt = case_inputs(B)
        kc = off_map_(kc.clone())
        eng = m._engine_at(_dev(), 128, 96)
        got = _step(eng, maps, k2d, kc, gt, None)
        assert margin_px(got["ref"]) >= MARGIN_PX
        _, dk2d, dref, w64, _ = points64(_params(m), k2d, got["ref"], gt, maps, context_blocks=False, depth=2)
        assert (got["out"].cpu().double() - w64).abs().max() <= 1e-5
        _hold("dk2d", got["dk2d"], dk2d)
        _hold("dref", got["dref"], dref)
        for p in WHOLLY_OUTSIDE_128x96:                                       # no corner inside any map: exactly 0 from the reference site
            assert (dref[0, p] == 0).all() and (got["dref"][0, p] == 0).all(), (p, got["dref"][0, p])
        assert (got["dref"][0, :8].abs().max(-1).values > 0).all()            # (partly outside points do have a gradient)
    finally:
        _release(m)


# ---- 6. bits ----------------------------------------------------------------------------------------------------------------------------------
def test_bits_against_the_sibling_entries_and_from_run_to_run():
    B = 6
    models = [_model(81, tame=False, drop=0.2), _model(81, tame=False, drop=0.2)]
    try:
        maps, k2d, kc, _, gt = case_inputs(B)
        masks = _masks(models[0], B, 9)
        s = _stream()
        results = []
        for model in models:
            eng = model._engine_at(_dev(), 128, 96)
            eng.set_map_grad_mode(1)
            _, total = eng.grad_layout_cached()
            out, ref_dev, k2d_dev = _forward(eng, maps, k2d, kc, masks)
            dout = _mpjpe_grad(out, gt)[1]
            new = lambda n=total: torch.full((n,), float("nan"), device="cuda")
            like_maps = lambda: [torch.full((B, h, w, c), float("nan"), device="cuda") for h, w, c in eng.feature_shapes()]
            kp = lambda: torch.full((B, J, 2), float("nan"), device="cuda")
            flat0, flat1, flat2, flat3, flat4 = new(), new(), new(), new(), new()
            dfeat1, dfeat2, dk_a, dr_a, dk_b, dr_b = like_maps(), like_maps(), kp(), kp(), kp(), kp()
            eng.backward(dout, flat0, s, masks)
            eng.backward_maps(dout, flat1, dfeat1, s, masks)
            eng.backward_points(dout, flat2, s, masks, dfeat2, dk_a, dr_a)
            eng.backward_points(dout, flat3, s, masks, None, dk_b, dr_b)      # (no maps: feat_embed's input gradient runs for dref alone)
            eng.backward_points(dout, flat4, s, masks, None, None, None)
            torch.cuda.synchronize()
            assert torch.isfinite(flat0).all()
            for name, f in (("capf_backward_maps", flat1), ("all three outputs", flat2), ("dk2d and dref", flat3), ("all NULL", flat4)):
                assert torch.equal(flat0, f), (name, (f - flat0).abs().max().item(), int((f != flat0).sum()))
            assert all(torch.equal(a, b) for a, b in zip(dfeat1, dfeat2))
            assert torch.isfinite(dk_a).all() and torch.isfinite(dr_a).all() and dk_a.abs().max() > 0 and dr_a.abs().max() > 0
            assert torch.equal(dk_a, dk_b) and torch.equal(dr_a, dr_b)
            only_k, only_r = kp(), kp()
            eng.backward_points(dout, new(), s, masks, None, only_k, None)
            eng.backward_points(dout, new(), s, masks, None, None, only_r)
            torch.cuda.synchronize()
            assert torch.equal(only_k, dk_a) and torch.equal(only_r, dr_a)
            assert torch.isfinite(ref_dev).all() and torch.isfinite(k2d_dev).all()      # (alive, and untouched by any backward)
            results.append((out, flat0, dk_a, dr_a))
        for a, b in zip(*results):                                            # a fresh handle: the same bits
            assert torch.equal(a, b)
    finally:
        _release(*models)


# ---- 7. stray accesses: an exact-size, NaN-filled workspace; every operand flush against a guard band ------------------------------------------------
def test_backward_points_on_a_poisoned_exact_size_workspace():
    B = 2
    model = _model(91, tame=True)
    try:
        maps, k2d, kc, _, gt = case_inputs(B)
        eng = model._engine_at(_dev(), 128, 96)
        eng.set_map_grad_mode(1)
        plain = _step(eng, maps, k2d, kc, gt, None, with_maps=True)
        _, total = eng.grad_layout_cached()
        fill = 0xFF
        ws = wg.install(eng, B, fill)
        k, c, d = (wg.flush(t.cuda(), fill) for t in (k2d, kc, plain["dout"]))
        fm = [wg.flush(m, fill) for m in _nhwc(maps)]
        out = wg.filled((B, 1, J, 3), torch.float32, "cuda", fill)
        flat = wg.filled((total,), torch.float32, "cuda", fill)
        dk2d, dref = wg.filled((B, J, 2), torch.float32, "cuda", fill), wg.filled((B, J, 2), torch.float32, "cuda", fill)
        dfeat = [wg.filled(t.shape, torch.float32, "cuda", fill) for t in fm]
        eng.set_features(fm, _stream())
        eng.lifter_forward_train(k, c, out, _stream(), None)
        eng.backward_points(d, flat, _stream(), None, dfeat, dk2d, dref)
        ws.check("capf_backward_points")
        wg.check_all([k, c, d, out, flat, dk2d, dref] + fm + dfeat, "capf_backward_points")
        assert torch.equal(out, plain["out"]) and torch.equal(flat, plain["flat"])
        assert torch.equal(dk2d, plain["dk2d"]) and torch.equal(dref, plain["dref"])
        assert all(torch.equal(a, b) for a, b in zip(dfeat, plain["dfeat"]))
    finally:
        _release(model)


# ---- 8. host: autograd end to end ----------------------------------------------------------------------------------------------------------------
class _KeypointHead(torch.nn.Module):
    """Two parameters in front of the lifter: a per-joint scale of the 2-D keypoints and a per-joint shift (pixels) of the crop keypoints.
    Scale 1 and shifts that are multiples of 1/4 keep the fp32 products and sums exact, so the GPU chain and the float64 chain
    differentiate the lifter at the same point."""

    def __init__(self, dtype=torch.float32):
        super().__init__()
        self.scale = torch.nn.Parameter(torch.ones(J, 2, dtype=dtype))
        g = torch.Generator().manual_seed(5)
        self.shift = torch.nn.Parameter((torch.randint(-8, 9, (J, 2), generator=g) / 4).to(dtype))

    def forward(self, k2d, kc):
        return k2d * self.scale, kc + self.shift


def _round_to(t, steps):
    return torch.round(t * steps) / steps


def _head_step(model, head, call, k2d, kc, gt):
    from mvn.models.loss import MPJPE
    a, b = head(k2d.cuda(), kc.cuda())
    assert not a.is_leaf and not b.is_leaf
    before = b.detach().clone()
    loss = MPJPE()(call(a, b), gt.cuda())
    loss.backward()
    torch.cuda.synchronize()
    assert torch.equal(b.detach(), before)                    # a crop-keypoint tensor in the graph is not mutated
    return loss.item(), normalise(before.cpu())


@pytest.mark.parametrize("route", ["forward_features", "forward"])
def test_a_keypoint_head_trains_through_the_lifter(route):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B = 2
    model = _model(101, tame=True)
    try:
        maps, k2d, kc, _, gt = case_inputs(B)
        kc = _round_to(kc, 4)                                 # (kc + shift exact in fp32)
        head = _KeypointHead().cuda()
        head64 = _KeypointHead(torch.float64)
        if route == "forward_features":
            eng = _engine(model)
            call = lambda a, b: model.forward_features([m.cuda() for m in maps], a, b)
        else:
            from capf import synth
            img = synth.synth_inputs(B, 128, 96, seed=103)[0].cuda()
            eng = model.engine_for(img)
            eng.set_debug(True)
            call = lambda a, b: model(img, a, b)
        loss, ref = _head_step(model, head, call, k2d, kc, gt)
        assert margin_px(ref) >= MARGIN_PX
        assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in model.volume_net.parameters())
        feats = [eng.tensor(f"feat{l}")[:B].cpu().permute(0, 3, 1, 2).contiguous() for l in range(4)]
        if route == "forward_features":
            assert all(torch.equal(f, m) for f, m in zip(feats, maps))
        # the float64 chain: head64 -> conpose.py:34-35 -> the oracle lifter in the engine's cells and on its clip sides
        a64, b64 = head64(k2d.double(), kc.double())
        assert torch.equal(normalise(b64.detach().float()), ref)
        r64 = b64 / torch.tensor([96.0, 128.0], dtype=torch.float64) - 1
        import capf_oracle as oracle
        P = {k: v.detach().cpu().double() for k, v in _params(model).items()}
        w = oracle.lifter_forward(P, a64, r64, [f.double() for f in feats], cells=engine_cells(eng, B), unclipped=engine_clip_sides(eng, B))
        l64 = oracle.mpjpe(w, gt.double())
        l64.backward()
        assert abs(loss - l64.item()) <= 1e-6 * abs(l64.item())
        print(f"  a keypoint head in front of {route}: loss {loss:.6f}")
        _hold("head.scale.grad", head.scale.grad, head64.scale.grad)
        _hold("head.shift.grad", head.shift.grad, head64.shift.grad)
    finally:
        _release(model)


def test_leaf_keypoints_and_the_unchanged_step_without_them():
    from mvn.models.loss import MPJPE
    B = 2
    model = _model(111, tame=True)
    try:
        maps, k2d, kc, _, gt = case_inputs(B)
        feats = [m.cuda() for m in maps]

        def step(mark):
            model.zero_grad(set_to_none=True)
            a, b = k2d.clone().cuda().requires_grad_(mark), kc.clone().cuda().requires_grad_(mark)
            out = model.forward_features(feats, a, b)
            MPJPE()(out, gt.cuda()).backward()
            torch.cuda.synchronize()
            return out.detach().clone(), model.last_flat_grad.clone(), a, b

        out1, flat1, a1, b1 = step(False)
        out2, flat2, a2, b2 = step(True)
        out3, flat3, a3, b3 = step(False)
        # unmarked: normalised in place, no keypoint gradient; the same bits before and after the marked step
        assert torch.equal(b1.cpu(), normalise(kc)) and a1.grad is None and b1.grad is None
        assert torch.equal(out1, out3) and torch.equal(flat1, flat3) and torch.equal(b1, b3)
        # marked: the leaf is untouched and both leaves receive .grad; output and parameter gradients have the unmarked step's bits
        assert torch.equal(b2.detach().cpu(), kc) and torch.equal(a2.detach().cpu(), k2d)
        assert torch.equal(out1, out2) and torch.equal(flat1, flat2)
        for g in (a2.grad, b2.grad):
            assert g is not None and tuple(g.shape) == (B, J, 2) and torch.isfinite(g).all() and g.abs().max() > 0
        # the crop-keypoint gradient is dref / (96, 128): the engine's dref through the C entry on the same step
        eng = model._engine_at(_dev(), 128, 96)
        got = _step(eng, maps, k2d, kc, gt, None)
        assert torch.equal(a2.grad, got["dk2d"])
        assert torch.equal(b2.grad, got["dref"] / torch.tensor([96.0, 128.0], device="cuda"))
        # only one of the two marked
        model.zero_grad(set_to_none=True)
        a, b = k2d.clone().cuda(), kc.clone().cuda().requires_grad_(True)
        MPJPE()(model.forward_features(feats, a, b), gt.cuda()).backward()
        assert torch.equal(b.grad, b2.grad) and torch.equal(b.detach().cpu(), kc)
        # under no_grad a tensor that requires grad is still left alone
        with torch.no_grad():
            out5 = model.forward_features(feats, k2d.clone().cuda(), b)
        assert torch.equal(b.detach().cpu(), kc) and (out5 - out1).abs().max() <= 1e-4      # (the inference plan's kernels: other bits)
    finally:
        _release(model)
