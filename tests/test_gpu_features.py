"""GPU: the lifter on caller-supplied context maps and the gradient w.r.t. the maps (capf_set_features, capf_lifter_forward_train,
capf_backward_maps, CA_PF.forward_features).

The yardstick is train_yardstick.py's: capf_oracle.lifter_forward in float64 on the engine's own maps (now with requires_grad) and in
the engine's own bilinear cells, MPJPE, autograd; test_features_api.py pins that oracle's map gradients to the reference's.  Bounds:
GRAD_L2_BOUND / GRAD_MAX_BOUND (2e-5 relative L2, 2e-5 of the fp64 gradient's largest entry) per map -- a map-gradient element is an
fp32 sum of at most a few thousand products, the arithmetic class those bounds were set for.

Crop keypoints of every case (_inputs): frame 0 has all 17 on ONE pixel (every sample of every joint adds into the same few map pixels:
the most atomic collisions the kernels can see); frame 1 mixes keypoints outside the crop box (ref outside [-1, 1]: the zero-padded
sampler drops corners, the border sampler clamps), keypoints on exact integer map pixels (a +1 corner of weight 0, the last pixel's +1
corner outside the map) and uniform ones; further frames are uniform."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import capf_oracle as oracle
from capf import synth
from conftest import make_model
from lifter_models import lifter_model
from train_yardstick import GRAD_L2_BOUND, GRAD_MAX_BOUND, check_gradients, engine_cells, engine_clip_sides, lifter64

pytestmark = pytest.mark.gpu

H2G_MIN_BATCH = 5        # csrc/engine.h: the first batch whose step runs on the two-piece GEMM


def _on_pixel(size, half, k):
    """A crop coordinate x whose map coordinate ((x / half - 1 + 1) / 2) * (size - 1) is EXACTLY k in the kernels' fp32 arithmetic."""
    f = np.float32
    for kk in list(range(k, size - 1)) + list(range(1, k)):
        x = f(f(2 * half) * f(kk) / f(size - 1))
        u = f(f(f(f(x / f(half)) - f(1)) + f(1)) / f(2)) * f(size - 1)
        if f(u) == f(kk):
            return float(x)
    raise AssertionError("no exact pixel")


def _inputs(B, H, W, seed, map_hw):
    """images, k2d, crop keypoints (pixels of the 192 x 256 box conpose.py:34-35 normalises by), gt -- with the layout of the docstring."""
    img, k2d, kc, gt = synth.synth_inputs(B, H, W, seed=seed, crop_range=(192, 256), with_gt=True)
    kc = kc.clone()
    kc[0] = torch.tensor([50.3, 70.7])
    if B > 1:
        h0, w0 = map_hw
        kc[1, 0:6] = torch.tensor([[-30.0, 100.0], [230.0, 40.0], [60.0, -25.0], [100.0, 300.0], [-5.0, -5.0], [200.0, 260.0]])
        kc[1, 6:12] = torch.tensor([[0.0, 0.0], [192.0, 256.0], [96.0, 0.0], [0.0, 256.0],
                                    [_on_pixel(w0, 96, 3), _on_pixel(h0, 128, 4)], [_on_pixel(w0, 96, w0 // 2), 128.0]])
    return img, k2d, kc, gt


def _train_mode(model, drop):
    model.train(); model.backbone.eval(); model.volume_net.train()
    model.drop_path_rate = drop
    return model


def _hrnet(backbone, wseed, drop=0.0, dtype=None):
    model, _ = make_model(backbone, device="cuda", wseed=wseed, bn="random", compute_dtype=dtype)
    return _train_mode(model, drop)


def _mpi(wseed, depth):
    from model.conpose import VolumetricTriangulationNet, mpi_preset
    from mvn.utils.cfg import config
    cfg = mpi_preset(copy.deepcopy(config), "hrnet_32")
    cfg.model.poseformer.depth = depth
    with contextlib.redirect_stdout(io.StringIO()):
        m = VolumetricTriangulationNet(cfg)
    synth.load_synthetic(m, seed=wseed, bn_mode="random")
    return _train_mode(m.cuda(), 0.0)


def _masks(model, B, seed):
    torch.manual_seed(seed)
    masks = model._drop_masks(B, torch.device("cuda"))
    assert masks is not None and (masks == 0).any()
    return masks


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _maps(eng, B):
    return [eng.tensor(f"feat{l}")[:B].contiguous() for l in range(4)]


def _empty_like_maps(eng, B, fill=None):
    out = [torch.empty(B, h, w, c, device="cuda") for h, w, c in eng.feature_shapes()]
    if fill is not None:
        for t in out:
            t.fill_(fill)
    return out


def _mpjpe_grad(out, gt):
    """MPJPE (loss.py:16-22) of the prediction and its gradient w.r.t. the prediction, by torch."""
    from mvn.models.loss import MPJPE
    p = out.detach().clone().requires_grad_(True)
    loss = MPJPE()(p, gt.cuda())
    loss.backward()
    return loss.item(), p.grad.contiguous()


def _flat_to_named(model, eng, flat):
    layout, _ = eng.grad_layout_cached()
    flat = flat.detach().cpu()
    return {"volume_net." + n: flat[layout["volume_net." + n][0]:][:p.numel()].view(p.shape).clone() for n, p in model.volume_net.named_parameters()}


def _map_errors(tag, got_nhwc, want_nchw):
    """Per map: relative L2 and max-entry error (of the fp64 gradient's largest entry); asserts the yardstick's bounds; returns the worst pair."""
    worst = (0.0, 0.0)
    for l, (g, t) in enumerate(zip(got_nhwc, want_nchw)):
        g = g.detach().cpu().permute(0, 3, 1, 2).double()
        assert torch.isfinite(g).all(), (tag, l)
        assert t.abs().max() > 0, (tag, l)
        d = g - t
        l2, mx = (d.norm() / t.norm()).item(), (d.abs().max() / t.abs().max()).item()
        print(f"    {tag} dfeat{l} {tuple(t.shape)}: {l2:9.2e} | {mx:9.2e}   (norm {t.norm().item():.3e})")
        worst = (max(worst[0], l2), max(worst[1], mx))
        assert l2 <= GRAD_L2_BOUND and mx <= GRAD_MAX_BOUND, (tag, l, l2, mx)
    return worst


# ---- 1. the split forward is the fused forward -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,drop", [(2, 0.0), (6, 0.2)], ids=["B2-fp32-pipe", "B6-two-piece-droppath"])
def test_split_training_forward_equals_the_fused_one_bit_for_bit(B, drop):
    model = _hrnet("hrnet_32", 31 + B, drop)
    img, k2d, kc, gt = _inputs(B, 128, 96, 32 + B, (32, 24))
    img, k2d = img.cuda(), k2d.cuda()
    eng = model.engine_for(img)
    assert (eng.lib.capf_train_h2_matrices(eng.h) > 0) and (B >= H2G_MIN_BATCH) == (B == 6)
    masks = _masks(model, B, 5) if drop else None
    _, total = eng.grad_layout_cached()
    dout = torch.randn(B, 1, 17, 3, generator=torch.Generator().manual_seed(3)).cuda()
    s = _stream()

    kc1, out1, flat1 = kc.clone().cuda(), torch.empty(B, 1, 17, 3, device="cuda"), torch.empty(total, device="cuda")
    eng.forward_train(img, k2d, kc1, out1, s, masks)
    eng.backward(dout, flat1, s, masks)

    kc2, out2, flat2 = kc.clone().cuda(), torch.full((B, 1, 17, 3), float("nan"), device="cuda"), torch.empty(total, device="cuda")
    eng.backbone_forward(img, s)
    eng.lifter_forward_train(k2d, kc2, out2, s, masks)
    dfeat = _empty_like_maps(eng, B)
    eng.backward_maps(dout, flat2, dfeat, s, masks)
    torch.cuda.synchronize()
    assert torch.isfinite(out1).all() and torch.equal(out1, out2)
    assert torch.equal(kc1, kc2)
    assert torch.equal(flat1, flat2)
    assert all(torch.isfinite(d).all() and d.abs().max() > 0 for d in dfeat)
    # no maps of this batch in the workspace: the lifter-only training forward refuses
    from capf.lib import CapfError
    eng.backbone_forward(img[:1].contiguous(), s)
    with pytest.raises(CapfError, match="context maps"):
        eng.lifter_forward_train(k2d, kc.clone().cuda(), out2, s, masks)


# ---- 2. maps round trip ----------------------------------------------------------------------------------------------------------------
def test_maps_set_into_a_second_engine_give_the_first_engines_output():
    B = 3
    img, k2d, kc, _ = _inputs(B, 128, 96, 41, (32, 24))
    img, k2d = img.cuda(), k2d.cuda()
    a, _ = make_model("hrnet_32", device="cuda", wseed=40, bn="random")
    b, _ = make_model("hrnet_32", device="cuda", wseed=40, bn="random")
    s = _stream()
    ea, eb = a.engine_for(img), b.engine_for(img)
    assert ea is not eb
    kca, outa = kc.clone().cuda(), torch.empty(B, 1, 17, 3, device="cuda")
    ea.forward(img, k2d, kca, outa, s)
    ea.backbone_forward(img, s)
    maps = _maps(ea, B)
    assert [tuple(m.shape[1:]) for m in maps] == eb.feature_shapes() == [(32, 24, 32), (16, 12, 64), (8, 6, 128), (4, 3, 256)]
    kcb, outb = kc.clone().cuda(), torch.full((B, 1, 17, 3), float("nan"), device="cuda")
    eb.set_features(maps, s)
    eb.lifter_forward(k2d, kcb, outb, s)
    torch.cuda.synchronize()
    assert torch.isfinite(outa).all() and torch.equal(outa, outb) and torch.equal(kca, kcb)
    for l in range(4):
        assert torch.equal(eb.tensor(f"feat{l}")[:B], maps[l])


# ---- 3. map gradients against float64 --------------------------------------------------------------------------------------------------
def _engine_step(model, eng, img, k2d, kc, gt, masks, dfeat):
    """backbone + lifter-only training forward + MPJPE + capf_backward_maps through the engine; returns prediction, loss, the normalised
    crop keypoints and the flat parameter gradient (all on the host)."""
    B = img.shape[0]
    s = _stream()
    _, total = eng.grad_layout_cached()
    kc_dev, out, flat = kc.clone().cuda(), torch.empty(B, 1, 17, 3, device="cuda"), torch.empty(total, device="cuda")
    eng.backbone_forward(img, s)
    eng.lifter_forward_train(k2d, kc_dev, out, s, masks)
    loss, dout = _mpjpe_grad(out, gt)
    eng.backward_maps(dout, flat, dfeat, s, masks)
    torch.cuda.synchronize()
    return out.cpu(), loss, kc_dev.cpu(), flat


CASES = [
    # backbone, (H, W), B, DropPath rate, depth (None: the H36M model with context blocks)
    ("hrnet_32", (128, 96), 2, 0.0, None),
    ("hrnet_32", (128, 96), 6, 0.2, None),
    ("hrnet_48", (128, 96), 5, 0.0, None),
    ("cpn", (256, 192), 2, 0.0, None),
    ("hrnet_32", (128, 96), 3, 0.0, 2),
]
# the two ends of the widths a plan accepts (tests/test_gpu_train_widths.py holds the parameter step there): feat_embed's input gradient is a
# dX GEMM with N = embed_dim_ratio that no parameter step runs (csrc/train.cpp backward, "embeddings").  At 32 the matrix is in no two-piece
# table (N < 64), at 288 it is no multiple of 64 columns; the narrow one sums the maps in the ordered mode
WIDTH_CASES = [
    # ... embed_dim_ratio (None: the preset's 128), capf_set_map_grad_mode (None: as the engine comes, atomic)
    ("hrnet_32", (128, 96), 6, 0.0, None, 32, 1),
    ("hrnet_32", (128, 96), 6, 0.0, None, 288, 0),
]


@pytest.mark.parametrize("backbone,hw,B,drop,depth,embed,mode", [c + (None, None) for c in CASES] + WIDTH_CASES,
                         ids=["hrnet_32-B2", "hrnet_32-B6-droppath", "hrnet_48-B5-Kpad", "cpn-B2", "mpi-hrnet_32-d2-B3",
                              "hrnet_32-E32-B6-ordered", "hrnet_32-E288-B6"])
def test_map_gradients_vs_fp64(backbone, hw, B, drop, depth, embed, mode):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    H, W = hw
    if embed:
        model = _train_mode(lifter_model(backbone, embed=embed, wseed=51 + B + embed)[0], drop)
    else:
        model = _mpi(51 + B, depth) if depth else _hrnet(backbone, 51 + B, drop)
    map_hw = (64, 48) if backbone == "cpn" else (H // 4, W // 4)
    img, k2d, kc, gt = _inputs(B, H, W, 52 + B, map_hw)
    img, k2d = img.cuda(), k2d.cuda()
    eng = model.engine_for(img)
    eng.set_debug(True)                                        # cidx taps of the deformable samplers
    if mode is not None:
        eng.set_map_grad_mode(mode)
        assert eng.map_grad_mode() == mode
    masks = _masks(model, B, 7) if drop else None
    dfeat = _empty_like_maps(eng, B)
    pred, loss, ref, flat = _engine_step(model, eng, img, k2d, kc, gt, masks, dfeat)
    assert (ref[1, :6].abs().max(-1).values > 1).all()         # frame 1's first keypoints are outside the crop box

    feats = [m.cpu().double().permute(0, 3, 1, 2).contiguous().requires_grad_(True) for m in _maps(eng, B)]
    assert [tuple(f.shape[1:]) for f in feats] == [(c, h, w) for h, w, c in eng.feature_shapes()]
    params = {"volume_net." + n: p for n, p in model.volume_net.named_parameters()}
    tag = f"{'mpi ' if depth else ''}{backbone} {H}x{W} B={B} DropPath {drop}" + (f" E={embed} map_grad_mode {mode}" if embed else "")
    if depth:
        Q = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in params.items()}
        w64 = oracle.lifter_forward(Q, k2d.cpu().double(), ref.double(), feats, context_blocks=False, depth=depth)
        l64 = oracle.mpjpe(w64, gt.double())
        l64.backward()
        g64, w64, l64 = {k: q.grad for k, q in Q.items()}, w64.detach(), l64.item()
    else:
        g64, w64, l64 = lifter64(params, k2d, ref, gt, feats, engine_cells(eng, B), masks, engine_clip_sides(eng, B))
    perr, lerr = (pred.double() - w64).abs().max().item(), abs(loss - l64) / abs(l64)
    print(f"  {tag}: prediction max|hip - fp64| {perr:.2e}, loss {loss:.6f} (relative error {lerr:.2e})")
    assert perr <= 1e-5 and lerr <= 1e-6, (perr, lerr)
    print(f"  {tag}: map gradients vs fp64 (relative L2 | max entry / max):")
    l2, mx = _map_errors(tag, dfeat, [f.grad for f in feats])
    got = _flat_to_named(model, eng, flat)
    if depth:
        assert set(got) == set(g64)
        pl2 = pmx = 0.0
        for k, t in g64.items():
            d = got[k].double() - t
            pl2 = max(pl2, (d.norm() / t.norm().clamp_min(1e-30)).item())
            pmx = max(pmx, (d.abs().max() / t.abs().max().clamp_min(1e-30)).item())
        assert pl2 <= GRAD_L2_BOUND and pmx <= GRAD_MAX_BOUND, (pl2, pmx)
    else:
        pl2, pmx = check_gradients(tag, got, g64)
    print(f"  {tag}: worst map gradient {l2:.2e} relative L2, {mx:.2e} of max; worst parameter gradient {pl2:.2e}, {pmx:.2e}")
    if embed:                                                  # (the training workspace grows with the width squared: 3.7 GB at 288)
        for e in model._engines.values():
            e.close()
        model._engines.clear()


# ---- 4. dfeat is overwritten, not accumulated into -------------------------------------------------------------------------------------
def test_backward_maps_overwrites_whatever_dfeat_held():
    B = 2
    model = _hrnet("hrnet_32", 61)
    img, k2d, kc, gt = _inputs(B, 128, 96, 62, (32, 24))
    img, k2d = img.cuda(), k2d.cuda()
    eng = model.engine_for(img)
    first, second = _empty_like_maps(eng, B, 0.0), _empty_like_maps(eng, B, float("nan"))
    _, _, _, flat1 = _engine_step(model, eng, img, k2d, kc, gt, None, first)
    _, _, _, flat2 = _engine_step(model, eng, img, k2d, kc, gt, None, second)
    assert torch.equal(flat1, flat2)                           # (the parameter gradient is reproducible; the atomic map sums need not be)
    _map_errors("second run vs first", second, [f.cpu().permute(0, 3, 1, 2).double() for f in first])


# ---- 5. host autograd end to end --------------------------------------------------------------------------------------------------------
class _ToyBackbone(torch.nn.Module):
    """Four convolutions of one [B,3,32,24] input, one per level: strides 1, 2, 4, 8 give the HRNet-32 maps of a 128 x 96 crop.
    Two choices, both made from float64 measurements of the oracle alone (no code under test involved):
    * weights and biases are multiples of 1/512 (and the test's input of 1/16): every product and every 27-term sum is exact in fp32 in
      any order, so the GPU's fp32 maps ARE the float64 chain's maps and both chains differentiate the lifter at the same point;
    * their scale is 1/8 of nn.Conv2d's default: maps of rms 0.07.  White-noise maps of rms 0.6 are so rough in space that this
      synthetic lifter's map gradient moves by 1.4e-4 (level 0) for a 1e-7 relative change of the maps, against 4.6e-7 on the native
      backbone's own maps; at 1/8 it moves by 1e-7 -- the conditioning the 2e-5 bound was set under (train_yardstick.py)."""

    def __init__(self):
        super().__init__()
        self.convs = torch.nn.ModuleList(torch.nn.Conv2d(3, c, 3, stride=2 ** l, padding=1) for l, c in enumerate((32, 64, 128, 256)))
        with torch.no_grad():
            for p in self.parameters():
                p.copy_(torch.round(p * 64) / 512)

    def forward(self, x):
        return [conv(x) for conv in self.convs]


def _rel(a, b):
    return ((a.double().cpu() - b.double().cpu()).norm() / b.double().cpu().norm()).item()


def test_a_torch_backbone_trains_through_forward_features():
    from capf.lib import CapfError
    from mvn.models.loss import MPJPE
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B = 3
    model = _hrnet("hrnet_32", 71)
    torch.manual_seed(72)
    toy = _ToyBackbone()
    toy64 = copy.deepcopy(toy).double()
    toy = toy.cuda()
    img, k2d, kc, gt = _inputs(B, 128, 96, 73, (32, 24))
    x = torch.round(torch.randn(B, 3, 32, 24, generator=torch.Generator().manual_seed(74)) * 16) / 16
    eng = model.engine_for(img.cuda())
    eng.set_debug(True)
    kept = []

    def step():
        kc_dev = kc.clone().cuda()
        maps = toy(x.cuda())
        for m in maps:
            m.retain_grad()
        kept[:] = maps
        loss = MPJPE()(model.forward_features(maps, k2d.cuda(), kc_dev), gt.cuda())
        loss.backward()
        torch.cuda.synchronize()
        return loss.item(), kc_dev

    loss1, kc_a = step()
    g1 = [p.grad.detach().clone() for p in toy.parameters()]
    maps1 = [m.detach().cpu() for m in kept]
    dmaps1 = [m.grad.detach().cpu() for m in kept]
    assert all(p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0 for p in model.volume_net.parameters())
    assert all(p.grad is None for p in model.backbone.parameters())

    # the float64 chain: the oracle lifter (in the engine's cells) behind the same convolutions
    params = {"volume_net." + n: p for n, p in model.volume_net.named_parameters()}
    maps64 = toy64(x.double())
    for m in maps64:
        m.retain_grad()
    assert all(torch.equal(a.double(), b.detach()) for a, b in zip(maps1, maps64)), "the toy maps are not exact in fp32"
    _, w64, l64 = lifter64(params, k2d, kc_a.cpu(), gt, maps64, engine_cells(eng, B))
    assert abs(loss1 - l64) / abs(l64) <= 1e-6
    for l in range(4):
        print(f"    dL/dmap{l} (NCHW, as torch receives it) {_rel(dmaps1[l], maps64[l].grad):9.2e}")
    for (n, p), g in zip(toy64.named_parameters(), g1):
        err = _rel(g, p.grad)
        print(f"    {n:16s} {err:9.2e}")
        assert err <= GRAD_L2_BOUND, (n, err)

    # the third argument is normalised in place exactly as forward does
    kc_b = kc.clone().cuda()
    with torch.no_grad():
        model(img.cuda(), k2d.cuda(), kc_b)
    assert torch.equal(kc_a, kc_b)
    # under no_grad: capf_set_features + capf_lifter_forward, no graph
    with torch.no_grad():
        plain = model.forward_features(toy(x.cuda()), k2d.cuda(), kc.clone().cuda())
    assert not plain.requires_grad and torch.isfinite(plain).all()

    # the lifter frozen, only the maps require grad: the same convolution gradients
    for p in model.volume_net.parameters():
        p.requires_grad_(False)
    toy.zero_grad(set_to_none=True)
    loss_f, _ = step()
    assert abs(loss_f - loss1) <= 1e-6 * abs(loss1)
    for (n, p), g in zip(toy.named_parameters(), g1):
        assert _rel(p.grad, g) <= GRAD_L2_BOUND, n
    for (n, p), q in zip(toy.named_parameters(), toy64.parameters()):
        assert _rel(p.grad, q.grad) <= GRAD_L2_BOUND, n
    for p in model.volume_net.parameters():
        p.requires_grad_(True)

    # a second step after an SGD update of both halves
    opt = torch.optim.SGD(list(toy.parameters()) + list(model.volume_net.parameters()), lr=1e-3)
    opt.step()
    opt.zero_grad(set_to_none=True)
    loss2, _ = step()
    print(f"  loss {loss1:.6f} -> {loss2:.6f} after one SGD step")
    assert np.isfinite(loss2) and abs(loss2 - loss1) > 1e-5 * abs(loss1)

    # one set of saved activations: backward of an overwritten forward raises
    out_a = model.forward_features(toy(x.cuda()), k2d.cuda(), kc.clone().cuda())
    model.forward_features(toy(x.cuda()), k2d.cuda(), kc.clone().cuda())
    with pytest.raises(CapfError, match="overwritten by a later forward"):
        MPJPE()(out_a, gt.cuda()).backward()


def test_the_variant_returns_its_own_layout():
    m = _mpi(81, 2)
    B = 2
    _, k2d, kc, _ = _inputs(B, 128, 96, 82, (32, 24))
    from feature_cases import HRNET32_128x96, synth_maps
    maps = [t.cuda().requires_grad_(True) for t in synth_maps(B, HRNET32_128x96, 83)]
    out, aux = m.forward_features(maps, k2d.cuda(), kc.clone().cuda())
    assert aux is None and tuple(out.shape) == (B, 3, 1, 17, 1)
    out.square().sum().backward()
    torch.cuda.synchronize()
    assert all(t.grad is not None and tuple(t.grad.shape) == tuple(t.shape) and torch.isfinite(t.grad).all() and t.grad.abs().max() > 0
               for t in maps)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------------------
def test_forward_features_refuses_a_bf16_model_with_the_librarys_reason():
    from capf.lib import CapfError
    from feature_cases import HRNET32_128x96, synth_maps
    model, _ = make_model("hrnet_32", device="cuda", wseed=91, bn="random", compute_dtype="bf16")
    _, k2d, kc, _ = _inputs(2, 128, 96, 92, (32, 24))
    with pytest.raises(CapfError, match="fp32 only.*bf16"):
        model.forward_features([t.cuda() for t in synth_maps(2, HRNET32_128x96, 93)], k2d.cuda(), kc.clone().cuda())
