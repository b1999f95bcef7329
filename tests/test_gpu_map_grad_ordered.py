"""GPU: the ordered, atomic-free sum of the gradient w.r.t. the context maps (capf_set_map_grad_mode 1, CA_PF.map_grad_mode).

Inputs are test_gpu_features.py's (_inputs): frame 0 has all 17 joints on ONE pixel -- all 1088 items of a deformable pass fall into a
handful of pixels, the longest segments and the most ties the sort can see; frame 1 has reference points outside the crop box, keypoints
on exact integer pixels, the last pixel's +1 corner outside the map and a corner of weight exactly 0.  Bounds: GRAD_L2_BOUND /
GRAD_MAX_BOUND of train_yardstick.py, the project's bounds for an fp32 sum of at most a few thousand products; the ordered sum is such a
sum (at most 1088 + 4 products per element and pass, five passes).

Nothing here asserts that the atomic route's bits DIFFER from run to run: that cannot be shown by a test."""
import pytest
import torch

import capf_oracle as oracle
from train_yardstick import engine_cells, lifter64
from test_gpu_features import (CASES, _empty_like_maps, _engine_step, _hrnet, _inputs, _map_errors, _maps, _masks, _mpi, _mpjpe_grad,
                               _stream)

pytestmark = pytest.mark.gpu

ATOMIC, ORDERED = 0, 1


def _as_reference(maps_nhwc):
    return [m.cpu().permute(0, 3, 1, 2).double() for m in maps_nhwc]


# ---- 1. bit-reproducible -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,drop", [(2, 0.0), (6, 0.2)], ids=["B2-fp32-pipe", "B6-two-piece-droppath"])
def test_ordered_map_gradient_is_bit_reproducible(B, drop):
    img, k2d, kc, gt = _inputs(B, 128, 96, 112 + B, (32, 24))
    img, k2d = img.cuda(), k2d.cuda()

    def engine():
        model = _hrnet("hrnet_32", 111 + B, drop)
        eng = model.engine_for(img)
        eng.set_map_grad_mode(ORDERED)
        assert eng.map_grad_mode() == ORDERED
        return model, eng

    model, eng = engine()
    masks = _masks(model, B, 9) if drop else None
    runs = []
    for fill in (0.0, float("nan"), 1e30):                     # whatever dfeat held is overwritten
        dfeat = _empty_like_maps(eng, B, fill)
        _, _, _, flat = _engine_step(model, eng, img, k2d, kc, gt, masks, dfeat)
        runs.append((dfeat, flat))
    for l in range(4):
        assert torch.isfinite(runs[0][0][l]).all() and runs[0][0][l].abs().max() > 0, l
    for dfeat, flat in runs[1:]:
        assert torch.equal(flat, runs[0][1])
        for l in range(4):
            assert torch.equal(dfeat[l], runs[0][0][l]), l
    for l in range(4):
        assert torch.equal(runs[1][0][l], runs[2][0][l]), l

    # a second model and engine from the same seeds (other addresses, another allocation order): the same bits
    pad = torch.empty(12345, device="cuda")
    model2, eng2 = engine()
    assert eng2 is not eng
    dfeat2 = _empty_like_maps(eng2, B, float("nan"))
    _, _, _, flat2 = _engine_step(model2, eng2, img, k2d, kc, gt, masks, dfeat2)
    assert torch.equal(flat2, runs[0][1])
    for l in range(4):
        assert torch.equal(dfeat2[l], runs[0][0][l]), l
    del pad


# ---- 2. correct against float64 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("backbone,hw,B,drop,depth", CASES,
                         ids=["hrnet_32-B2", "hrnet_32-B6-droppath", "hrnet_48-B5-Kpad", "cpn-B2", "mpi-hrnet_32-d2-B3"])
def test_ordered_map_gradients_vs_fp64(backbone, hw, B, drop, depth):
    """test_gpu_features.py::test_map_gradients_vs_fp64 in ordered mode: the same cases, float64 oracle and bounds."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    H, W = hw
    model = _mpi(51 + B, depth) if depth else _hrnet(backbone, 51 + B, drop)
    map_hw = (64, 48) if backbone == "cpn" else (H // 4, W // 4)
    img, k2d, kc, gt = _inputs(B, H, W, 52 + B, map_hw)
    img, k2d = img.cuda(), k2d.cuda()
    eng = model.engine_for(img)
    eng.set_debug(True)                                        # cidx taps of the deformable samplers
    eng.set_map_grad_mode(ORDERED)
    masks = _masks(model, B, 7) if drop else None
    dfeat = _empty_like_maps(eng, B, float("nan"))
    pred, loss, ref, _ = _engine_step(model, eng, img, k2d, kc, gt, masks, dfeat)
    assert eng.map_grad_mode() == ORDERED
    assert (ref[1, :6].abs().max(-1).values > 1).all()         # frame 1's first keypoints are outside the crop box

    feats = [m.cpu().double().permute(0, 3, 1, 2).contiguous().requires_grad_(True) for m in _maps(eng, B)]
    params = {"volume_net." + n: p for n, p in model.volume_net.named_parameters()}
    tag = f"ordered {'mpi ' if depth else ''}{backbone} {H}x{W} B={B} DropPath {drop}"
    if depth:
        Q = {k: v.detach().cpu().double() for k, v in params.items()}
        w64 = oracle.lifter_forward(Q, k2d.cpu().double(), ref.double(), feats, context_blocks=False, depth=depth)
        l64 = oracle.mpjpe(w64, gt.double())
        l64.backward()
        w64, l64 = w64.detach(), l64.item()
    else:
        _, w64, l64 = lifter64(params, k2d, ref, gt, feats, engine_cells(eng, B), masks)
    perr, lerr = (pred.double() - w64).abs().max().item(), abs(loss - l64) / abs(l64)
    print(f"  {tag}: prediction max|hip - fp64| {perr:.2e}, loss {loss:.6f} (relative error {lerr:.2e})")
    assert perr <= 1e-5 and lerr <= 1e-6, (perr, lerr)
    print(f"  {tag}: map gradients vs fp64 (relative L2 | max entry / max):")
    l2, mx = _map_errors(tag, dfeat, [f.grad for f in feats])
    print(f"  {tag}: worst map gradient {l2:.2e} relative L2, {mx:.2e} of max")


# ---- 3. one step, two routes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [2, 6], ids=["B2-fp32-pipe", "B6-two-piece"])
def test_both_routes_on_one_saved_step(B):
    model = _hrnet("hrnet_32", 121 + B)
    img, k2d, kc, gt = _inputs(B, 128, 96, 122 + B, (32, 24))
    img, k2d = img.cuda(), k2d.cuda()
    eng = model.engine_for(img)
    s = _stream()
    _, total = eng.grad_layout_cached()
    kc_dev, out = kc.clone().cuda(), torch.empty(B, 1, 17, 3, device="cuda")
    eng.forward_train(img, k2d, kc_dev, out, s, None)
    _, dout = _mpjpe_grad(out, gt)
    got = []
    for mode in (ATOMIC, ORDERED, ATOMIC):                     # a backward only reads the saved activations
        eng.set_map_grad_mode(mode)
        flat, dfeat = torch.full((total,), float("nan"), device="cuda"), _empty_like_maps(eng, B, float("nan"))
        eng.backward_maps(dout, flat, dfeat, s, None)
        torch.cuda.synchronize()
        got.append((flat, dfeat))
    assert eng.map_grad_mode() == ATOMIC
    assert torch.isfinite(got[0][0]).all()
    assert torch.equal(got[0][0], got[1][0]) and torch.equal(got[0][0], got[2][0])      # flat_grad keeps its bits in both modes
    first = _as_reference(got[0][1])
    _map_errors(f"B={B} ordered vs atomic", got[1][1], first)
    _map_errors(f"B={B} atomic again vs atomic", got[2][1], first)


# ---- 4. through autograd ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("train_lifter", [False, True], ids=["lifter-frozen", "lifter-trained"])
def test_forward_features_map_gradients_are_reproducible(train_lifter):
    """No torch matmul or convolution below: the maps are leaves, the loss is the library's MPJPE -- torch's own deterministic-mode
    rules are not what is tested."""
    from mvn.models.loss import MPJPE
    B = 2
    model = _hrnet("hrnet_32", 131)
    img, k2d, kc, gt = _inputs(B, 128, 96, 132, (32, 24))
    img, k2d, gt = img.cuda(), k2d.cuda(), gt.cuda()
    eng = model.engine_for(img)
    eng.backbone_forward(img, _stream())                       # the native backbone's own maps: the conditioning the bounds were set under
    maps = [m.permute(0, 3, 1, 2).contiguous().requires_grad_(True) for m in _maps(eng, B)]
    for p in model.volume_net.parameters():
        p.requires_grad_(train_lifter)

    def round_():
        for m in maps:
            m.grad = None
        model.volume_net.zero_grad(set_to_none=True)
        MPJPE()(model.forward_features(maps, k2d, kc.clone().cuda()), gt).backward()
        torch.cuda.synchronize()
        assert all(m.grad is not None and torch.isfinite(m.grad).all() and m.grad.abs().max() > 0 for m in maps)
        assert all((p.grad is not None) == train_lifter for p in model.volume_net.parameters())
        return [m.grad.clone() for m in maps]

    assert model.map_grad_mode is None and eng.map_grad_mode() == ATOMIC
    model.map_grad_mode = "ordered"
    a, b = round_(), round_()
    assert eng.map_grad_mode() == ORDERED
    assert all(torch.equal(x, y) for x, y in zip(a, b))

    model.map_grad_mode = None
    before = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        round_()
        assert eng.map_grad_mode() == ATOMIC                   # the switch is off: the default route
        torch.use_deterministic_algorithms(True)
        c, d = round_(), round_()
        assert eng.map_grad_mode() == ORDERED                  # the torch switch selected the deterministic form
        assert all(torch.equal(x, y) for x, y in zip(c, d))
        assert all(torch.equal(x, y) for x, y in zip(a, c))    # ... which is the explicit "ordered" one
        torch.use_deterministic_algorithms(False)
        round_()
        assert eng.map_grad_mode() == ATOMIC
    finally:
        torch.use_deterministic_algorithms(before)
