"""GPU: the keypoint head inside the model -- CA_PF(keypoint_head=...).detect / forward_detect, the head under autograd through the lifter,
and the head as a free function in front of forward_features.  HRNet-32 at 64x64 and 128x96, batch 2-3.

Bit equalities are exact.  Gradients of the head go against float64: the head (kp_head_cases) on the engine's own feat0, then
capf_oracle.lifter_forward in the engine's cells and on its clip sides, then MPJPE -- test_gpu_points_grad.py's recipe with final_layer's
weight as the leaf.  The bound is that file's: 2e-5 (relative L2 | largest entry) where the same evaluation in float32 sits within 5e-6 of
float64, else 4 x that distance; nothing of the engine's result enters it.  The reference points are the head's own output, so the test
asserts their distance from a cell boundary (points_grad_cases.margin_px) instead of choosing it."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import capf_oracle as oracle
import kp_head_cases as K
from capf import lib as capf
from capf import synth
from points_grad_cases import MARGIN_PX, margin_px, rel_errors, tame_
from train_yardstick import GRAD_L2_BOUND, GRAD_MAX_BOUND, engine_cells, engine_clip_sides

pytestmark = pytest.mark.gpu
FLOOR_LIMIT = 5e-6
J = 17


def _model(head, dtype="fp32", wseed=3, beta=1.0, tame=False, **kw):
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), "hrnet_32")
    cfg.model.backbone.fix_weights = True
    with contextlib.redirect_stdout(io.StringIO()):
        m = CA_PF(cfg, compute_dtype=dtype, keypoint_head=head, keypoint_beta=beta, **kw).eval()
    synth.load_synthetic(m, seed=wseed, bn_mode="random")
    if tame:
        tame_(dict(m.volume_net.named_parameters()))
    return m.cuda()


def _release(*models):
    for m in models:
        for e in m._engines.values():
            e.close()
        m._engines.clear()


def _inputs(B, H, W, seed=9, u8=False):
    g = torch.Generator().manual_seed(seed)
    if u8:
        images = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    else:
        images = torch.randn(B, H, W, 3, generator=g)
    A = torch.from_numpy(np.stack([capf.crop_to_image_matrix((480.0 + 20 * b, 510.0 - 10 * b), (1.2 + 0.1 * b, 1.6 + 0.1 * b), (W, H), 1000, 1002)
                                   for b in range(B)]).astype(np.float32))
    gt = 0.3 * torch.randn(B, 1, J, 3, generator=g)
    gt[:, :, 0] = 0
    return images.cuda(), A.cuda(), gt.cuda()


# ---- 1. forward_detect == forward on detect's keypoints -------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,u8,head,H,W", [("fp32", False, "argmax", 64, 64), ("fp32", True, "integral", 128, 96), ("fp16", False, "integral", 128, 96),
                                              ("fp16", True, "argmax", 64, 64)],
                         ids=["fp32-float-argmax-64x64", "fp32-u8-integral-128x96", "fp16-float-integral-128x96", "fp16-u8-argmax-64x64"])
def test_forward_detect_equals_forward_on_detected_keypoints(dtype, u8, head, H, W):
    B = 3
    m, fresh = _model(head, dtype, beta=2.0), _model(head, dtype, beta=2.0)
    try:
        images, A, _ = _inputs(B, H, W, u8=u8)
        with torch.no_grad():
            kcrop, score, k2d = m.detect(images, A)
            assert kcrop.shape == (B, J, 2) and score.shape == (B, J) and k2d.shape == (B, J, 2)
            assert torch.isfinite(kcrop).all() and torch.isfinite(score).all() and torch.isfinite(k2d).all()
            assert (kcrop[..., 0] >= 0).all() and (kcrop[..., 0] <= W).all() and (kcrop[..., 1] >= 0).all() and (kcrop[..., 1] <= H).all()
            k_only, s_only, none = m.detect(images)
            assert none is None and torch.equal(k_only, kcrop) and torch.equal(s_only, score)
            out, kc2, sc2 = m.forward_detect(images, A)
            assert torch.equal(kc2, kcrop) and torch.equal(sc2, score)                       # still pixels: the lifter normalised a copy
            fwd = m.forward_u8 if u8 else m.forward
            want = fwd(images, k2d, kcrop.clone())
            assert out.shape == (B, 1, J, 3) and torch.equal(out, want)
            # detect leaves the engine usable: a plain forward right after it has a fresh engine's bits
            m.detect(images, A)
            g = torch.Generator().manual_seed(1)
            k2d_given, kc_given = torch.rand(B, J, 2, generator=g).cuda() * 2 - 1, (torch.rand(B, J, 2, generator=g) * 190).cuda()
            assert torch.equal(fwd(images, k2d_given, kc_given.clone()), getattr(fresh, fwd.__name__)(images, k2d_given, kc_given.clone()))
            if u8:       # the uint8 crops and their normalised float image: the same keypoints, bit for bit
                imgf = capf.preprocess(images, None, k2d_given, kc_given, "hrnet_32", 0)[0]
                kf, sf, k2f = m.detect(imgf, A)
                assert torch.equal(kf, kcrop) and torch.equal(sf, score) and torch.equal(k2f, k2d)
    finally:
        _release(m, fresh)


def test_forward_detect_with_batch_statistics_backbone():
    B, H, W = 3, 64, 64
    m = _model("integral", backbone_bn="batch")
    twin = _model("integral", backbone_bn="batch")
    try:
        m.train(); twin.train()
        assert m._bn_batch_active()
        images, A, _ = _inputs(B, H, W)
        with torch.no_grad():
            out, kcrop, score = m.forward_detect(images, A)
            kc_t, sc_t, k2d_t = twin.detect(images, A)            # the twin's statistics move by the same step: its detect sees the same maps
            assert torch.equal(kc_t, kcrop) and torch.equal(sc_t, score)
            twin2 = _model("integral", backbone_bn="batch").train()
            try:
                assert torch.equal(out, twin2(images, k2d_t, kcrop.clone()))
            finally:
                _release(twin2)
    finally:
        _release(m, twin)


# ---- 2. the integral head under grad, through the lifter --------------------------------------------------------------------------------
def _head64(weight, bias, feat0_nhwc, A, beta, H, W, dtype):
    """the head of kp_head_cases in `dtype` with weight [J, C] / bias as leaves: (kcrop pixels, k2d)"""
    z = F.conv2d(feat0_nhwc.to(dtype).permute(0, 3, 1, 2), weight[:, :, None, None], bias)
    xy, _ = K.decode_integral(z, beta)
    decode = (W / feat0_nhwc.shape[2], 0.0, H / feat0_nhwc.shape[1], 0.0)
    return K.to_outputs(xy, decode, A.cpu().numpy())


def _through_lifter(model, eng, B, A, gt, beta, H, W, dtype, feat_leaf=False):
    feats = [eng.tensor(f"feat{l}")[:B].cpu() for l in range(4)]                                # NHWC fp32
    fl = model.keypoint_head.final_layer
    w = fl.weight.detach().cpu().to(dtype).reshape(J, -1).clone().requires_grad_(True)
    b = fl.bias.detach().cpu().to(dtype).clone().requires_grad_(True)
    f0 = feats[0].to(dtype).clone().requires_grad_(feat_leaf)
    kcrop, k2d = _head64(w, b, f0, A, beta, H, W, dtype)
    ref = torch.stack([kcrop[..., 0] / 96.0 - 1.0, kcrop[..., 1] / 128.0 - 1.0], -1)           # conpose.py:34-35
    Q = {"volume_net." + n: p.detach().cpu().to(dtype).clone().requires_grad_(True) for n, p in model.volume_net.named_parameters()}
    maps = [f0.permute(0, 3, 1, 2)] + [f.to(dtype).permute(0, 3, 1, 2) for f in feats[1:]]
    pred = oracle.lifter_forward(Q, k2d, ref, maps, cells=engine_cells(eng, B), unclipped=engine_clip_sides(eng, B))
    loss = oracle.mpjpe(pred, gt.cpu().to(dtype))
    loss.backward()
    return {"w": w.grad, "b": b.grad, "ref": ref.detach(), "loss": loss.item(), "f0": f0.grad}


def _hold(tag, got, t64, t32):
    fl2, fmx = rel_errors(t32, t64)
    b2 = GRAD_L2_BOUND if fl2 <= FLOOR_LIMIT else 4 * fl2
    bm = GRAD_MAX_BOUND if fmx <= FLOOR_LIMIT else 4 * fmx
    l2, mx = rel_errors(got, t64)
    print(f"    {tag}: relative L2 {l2:.2e} (bound {b2:.1e}, floor {fl2:.1e}) | max entry / max {mx:.2e} (bound {bm:.1e}, floor {fmx:.1e})   "
          f"largest entry {t64.abs().max().item():.3e}")
    assert t64.abs().max() > 0 and l2 <= b2 and mx <= bm, (tag, l2, mx, b2, bm)


def test_integral_head_trains_through_the_lifter_vs_fp64():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B, H, W, beta = 2, 128, 96, 3.0
    m = _model("integral", beta=beta, wseed=43, tame=True)
    try:
        m.train(); m.backbone.eval(); m.drop_path_rate = 0.0                                   # DropPath off
        from mvn.models.loss import MPJPE
        images, A, gt = _inputs(B, H, W)
        eng = m._engine_at(images.device, H, W)
        eng.set_debug(True)
        out, kcrop, score = m.forward_detect(images, A)
        assert kcrop.requires_grad and out.requires_grad and not score.requires_grad
        MPJPE()(out, gt).backward()
        torch.cuda.synchronize()
        fl = m.keypoint_head.final_layer
        assert fl.weight.grad is not None and torch.isfinite(fl.weight.grad).all()
        assert (fl.bias.grad == 0).all()                                                       # exactly: softmax ignores a shift
        lifter = {n: p.grad.clone() for n, p in m.volume_net.named_parameters()}
        y64 = _through_lifter(m, eng, B, A, gt, beta, H, W, torch.float64)
        y32 = _through_lifter(m, eng, B, A, gt, beta, H, W, torch.float32)
        margin = margin_px(y64["ref"], [(c, h, w) for h, w, c in eng.feature_shapes()])
        print(f"  head through lifter: reference points {margin:.2e} px from the nearest cell boundary, |dbias64| {y64['b'].abs().max().item():.1e}")
        assert margin >= MARGIN_PX
        assert (kcrop.detach().cpu().double() - (y64["ref"] + 1) * torch.tensor([96.0, 128.0], dtype=torch.float64)).abs().max() <= 1e-4
        _hold("final_layer.weight.grad", fl.weight.grad.reshape(J, -1), y64["w"], y32["w"])
        # the lifter's gradients: the same step through forward() on the detached keypoints, bit for bit
        with torch.no_grad():
            kc_d, _, k2d_d = m.detect(images, A)
        assert torch.equal(kc_d, kcrop.detach())
        for p in m.parameters():
            p.grad = None
        MPJPE()(m(images, k2d_d, kc_d.clone()), gt).backward()
        for n, p in m.volume_net.named_parameters():
            assert torch.equal(p.grad, lifter[n]), n
        assert fl.weight.grad is None
    finally:
        _release(m)


def test_two_adamw_steps_on_the_head_lower_a_keypoint_loss():
    from mvn.models.loss import KeypointsMSELoss
    B, H, W = 3, 64, 64
    m = _model("integral", beta=2.0)
    try:
        m.volume_net.requires_grad_(False)
        images, A, _ = _inputs(B, H, W)
        g = torch.Generator().manual_seed(5)
        target = (torch.rand(B, J, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])).cuda()
        valid = torch.ones(B, J, 1).cuda()
        opt = torch.optim.AdamW(m.keypoint_head.parameters(), lr=0.01, weight_decay=0.0)
        losses = []
        for _ in range(3):
            opt.zero_grad()
            _, kcrop, _ = m.forward_detect(images, A)
            loss = KeypointsMSELoss()(kcrop, target, valid)
            losses.append(loss.item())
            loss.backward()
            opt.step()
        print(f"  KeypointsMSELoss over two AdamW steps on the head: {losses}")
        assert losses[2] < losses[1] < losses[0]
    finally:
        _release(m)


# ---- 3. the head as a free function in front of forward_features ----------------------------------------------------------------------------
def test_head_function_hands_the_map_its_gradient():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    from mvn.models.conpose import keypoint_head
    from mvn.models.loss import MPJPE
    B, H, W, beta = 2, 128, 96, 3.0
    m = _model("integral", beta=beta, wseed=43, tame=True)
    try:
        m.train(); m.backbone.eval(); m.drop_path_rate = 0.0
        images, A, gt = _inputs(B, H, W)
        eng = m._engine_at(images.device, H, W)
        eng.set_debug(True)
        with torch.no_grad():
            m.detect(images, A)                                                               # fills the workspace's maps
        maps = [eng.tensor(f"feat{l}")[:B].permute(0, 3, 1, 2).contiguous().requires_grad_(l == 0) for l in range(4)]       # NCHW, a torch backbone's output
        fl = m.keypoint_head.final_layer
        decode = (W / maps[0].shape[3], 0.0, H / maps[0].shape[2], 0.0)
        kcrop, score, k2d = keypoint_head(maps[0].permute(0, 2, 3, 1).contiguous(), fl.weight, fl.bias, A, "integral", beta, decode)
        out = m.forward_features(maps, k2d, kcrop)
        MPJPE()(out, gt).backward()
        torch.cuda.synchronize()
        assert maps[0].grad is not None and maps[0].grad.shape == maps[0].shape
        y64 = _through_lifter(m, eng, B, A, gt, beta, H, W, torch.float64, feat_leaf=True)
        y32 = _through_lifter(m, eng, B, A, gt, beta, H, W, torch.float32, feat_leaf=True)
        assert margin_px(y64["ref"], [(c, h, w) for h, w, c in eng.feature_shapes()]) >= MARGIN_PX
        _hold("d(feat0): head + lifter", maps[0].grad.permute(0, 2, 3, 1), y64["f0"], y32["f0"])
        _hold("final_layer.weight.grad", fl.weight.grad.reshape(J, -1), y64["w"], y32["w"])
        assert (fl.bias.grad == 0).all()
    finally:
        _release(m)
