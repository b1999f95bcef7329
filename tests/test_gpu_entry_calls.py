"""GPU: which engine entries every host entry point of CA_PF reaches, in which order.

The bit-parity tests cannot tell an entry that reaches the same bits through other engine calls (forward_detect == forward bit for bit is by
design).  Here the run entries of capf.lib.Engine are patched with recorders that note their name and call through, and every row of the
table "(image source, grad mode, BatchNorm mode) -> engine calls" is held to its sequence, forward and backward apart.  backward_points
also notes which of its optional outputs (dfeat, dk2d, dref) were asked for.

HRNet-32, fp32, 64x64 crops, batch 2 (a uint8 pair: one source crop): the smallest geometry test_gpu_sessions.py uses; batch 2 leaves
2 x 2 x 2 = 8 values per channel on the smallest branch, which capf_backbone_forward_bn accepts.  Nothing here looks at a kernel's result
beyond what a row of the table says about tensors of the caller's."""
import pytest
import torch

import test_gpu_cpn_flip as cpn
from capf import synth
from capf.lib import Engine
from feature_cases import synth_maps
from test_gpu_kp_head_model import _inputs, _model, _release

pytestmark = pytest.mark.gpu

J, B, H, W = 17, 2, 64, 64
RECORDED = ("forward", "forward_u8", "forward_train", "forward_train_u8", "backbone_forward", "backbone_forward_u8", "backbone_forward_bn",
            "lifter_forward", "lifter_forward_train", "set_features", "backward", "backward_maps", "params_changed", "lifter_params_changed",
            "set_map_grad_mode")
STEP = ["set_features", "lifter_forward_train"]


@pytest.fixture
def log(monkeypatch):
    """The names of the Engine run entries called since the last clear(), in order."""
    calls = []

    def recorder(name, real):
        def run(self, *args, **kwargs):
            calls.append(name)
            return real(self, *args, **kwargs)
        return run

    for name in RECORDED:
        monkeypatch.setattr(Engine, name, recorder(name, getattr(Engine, name)))
    real_points = Engine.backward_points

    def backward_points(self, grad_out, flat_grad, stream, masks=None, dfeat_nhwc=None, dk2d=None, dref=None):
        asked = [n for n, t in (("dfeat", dfeat_nhwc), ("dk2d", dk2d), ("dref", dref)) if t is not None]
        calls.append("backward_points({})".format(", ".join(asked)))
        return real_points(self, grad_out, flat_grad, stream, masks, dfeat_nhwc, dk2d, dref)

    monkeypatch.setattr(Engine, "backward_points", backward_points)
    return calls


def _keypoints(batch=B, seed=5):
    _, k2d, kc, _ = synth.synth_inputs(batch, H, W, seed=seed, crop_range=(W, H), with_gt=True)
    return k2d.cuda(), kc.cuda()


@pytest.fixture(scope="module")
def head_model():
    """keypoint_head="integral", warmed up: its 64x64 engine exists and is bound"""
    m = _model("integral")
    images, _, _ = _inputs(B, H, W)
    k2d, kc = _keypoints()
    with torch.no_grad():
        m(images, k2d, kc.clone())
    yield m
    _release(m)


@pytest.fixture(scope="module")
def bn_model():
    """backbone_bn="batch", warmed up in eval mode"""
    m = _model(None, backbone_bn="batch")
    images, _, _ = _inputs(B, H, W)
    k2d, kc = _keypoints()
    with torch.no_grad():
        m(images, k2d, kc.clone())
    yield m
    _release(m)


def _step(log, call):
    """One forward under grad and its backward: (the forward's calls, the backward's calls, the forward's result)."""
    del log[:]
    with torch.enable_grad():
        out = call()
        out = out[0] if isinstance(out, tuple) else out
        fwd = list(log)
        del log[:]
        out.square().sum().backward()
    return fwd, list(log), out


def _plain(log, call):
    del log[:]
    with torch.no_grad():
        out = call()
    return list(log), out


@pytest.fixture
def frozen_lifter(head_model):
    head_model.zero_grad(set_to_none=True)
    head_model.volume_net.requires_grad_(False)
    yield head_model
    head_model.volume_net.requires_grad_(True)
    head_model.zero_grad(set_to_none=True)


# ---- forward ---------------------------------------------------------------------------------------------------------------------------------
def test_forward(head_model, log):
    m = head_model
    images, _, _ = _inputs(B, H, W)
    k2d, kc = _keypoints()
    assert _plain(log, lambda: m(images, k2d, kc.clone()))[0] == ["forward"]
    fwd, bwd, _ = _step(log, lambda: m(images, k2d, kc.clone()))
    assert (fwd, bwd) == (["forward_train"], ["backward"])
    k2d_leaf = k2d.clone().requires_grad_(True)
    fwd, bwd, _ = _step(log, lambda: m(images, k2d_leaf, kc.clone()))
    assert (fwd, bwd) == (["forward_train"], ["backward_points(dk2d)"])
    assert k2d_leaf.grad is not None and k2d_leaf.grad.shape == k2d.shape


def test_forward_frozen_lifter_crop_keypoints_in_the_graph(frozen_lifter, log):
    m = frozen_lifter
    images, _, _ = _inputs(B, H, W)
    k2d, kc = _keypoints()
    kc_leaf = kc.clone().requires_grad_(True)
    fwd, bwd, _ = _step(log, lambda: m(images, k2d, kc_leaf))
    assert (fwd, bwd) == (["forward_train"], ["backward_points(dref)"])
    assert all(p.grad is None for p in m.parameters())
    assert torch.equal(kc_leaf.detach(), kc) and kc_leaf.grad is not None          # a tensor in the graph is never normalised in place


def test_forward_writes_back_into_a_non_contiguous_view(head_model, log):
    m = head_model
    images, _, _ = _inputs(B, H, W)
    k2d, kc = _keypoints()
    wide = torch.zeros(B, J, 4, device="cuda")
    view = wide[..., 1:3]
    view.copy_(kc)
    assert not view.is_contiguous()
    contiguous = kc.clone()
    with torch.no_grad():
        want = m(images, k2d, contiguous)
    calls, out = _plain(log, lambda: m(images, k2d, view))
    assert calls == ["forward"] and torch.equal(out, want)
    assert torch.equal(view, contiguous) and not torch.equal(view, kc)
    ref = torch.stack([kc[..., 0] / 96.0 - 1.0, kc[..., 1] / 128.0 - 1.0], -1)      # conpose.py:34-35
    assert torch.allclose(view, ref, rtol=0, atol=1e-6)
    assert (wide[..., 0] == 0).all() and (wide[..., 3] == 0).all()


def test_forward_after_an_in_place_parameter_update(head_model, log):
    m = head_model
    images, _, _ = _inputs(B, H, W)
    k2d, kc = _keypoints()
    with torch.no_grad():
        next(m.volume_net.parameters()).add_(0)
    assert _plain(log, lambda: m(images, k2d, kc.clone()))[0] == ["lifter_params_changed", "forward"]
    assert _plain(log, lambda: m(images, k2d, kc.clone()))[0] == ["forward"]


# ---- forward_u8 ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mirror", ["none", "all", "pair"])
def test_forward_u8(head_model, log, mirror):
    m = head_model
    crops, _, _ = _inputs(1 if mirror == "pair" else B, H, W, u8=True)
    k2d, kc = _keypoints()
    calls, out = _plain(log, lambda: m.forward_u8(crops, k2d, kc.clone(), mirror=mirror))
    assert calls == ["forward_u8"] and out.shape == (B, 1, J, 3)


def test_forward_u8_under_grad(head_model, log):
    m = head_model
    crops, _, _ = _inputs(B, H, W, u8=True)
    k2d, kc = _keypoints()
    fwd, bwd, _ = _step(log, lambda: m.forward_u8(crops, k2d, kc.clone()))
    assert (fwd, bwd) == (["forward_train_u8"], ["backward"])


# ---- backbone_bn="batch" ---------------------------------------------------------------------------------------------------------------------
def test_batch_statistics_route(bn_model, log):
    m = bn_model
    images, _, _ = _inputs(B, H, W)
    k2d, kc = _keypoints()
    try:
        m.backbone.train()
        for _ in range(2):
            assert _plain(log, lambda: m(images, k2d, kc.clone()))[0] == ["backbone_forward_bn", "lifter_forward"]
        fwd, bwd, _ = _step(log, lambda: m(images, k2d, kc.clone()))
        assert (fwd, bwd) == (["backbone_forward_bn", "lifter_forward_train"], ["backward"])
    finally:
        m.backbone.eval()
    # the running statistics moved: the folded packs are rebuilt once, on the first running-statistics forward
    assert _plain(log, lambda: m(images, k2d, kc.clone()))[0] == ["params_changed", "forward"]
    assert _plain(log, lambda: m(images, k2d, kc.clone()))[0] == ["forward"]


# ---- detect / forward_detect -----------------------------------------------------------------------------------------------------------------
def test_detect(head_model, log):
    m = head_model
    images, A, _ = _inputs(B, H, W)
    crops, _, _ = _inputs(B, H, W, u8=True)
    assert _plain(log, lambda: m.detect(images, A))[0] == ["backbone_forward"]
    assert _plain(log, lambda: m.detect(crops, A))[0] == ["backbone_forward_u8"]


def test_forward_detect(head_model, log):
    m = head_model
    images, A, _ = _inputs(B, H, W)
    assert _plain(log, lambda: m.forward_detect(images, A))[0] == ["backbone_forward", "lifter_forward"]
    m.zero_grad(set_to_none=True)
    fwd, bwd, _ = _step(log, lambda: m.forward_detect(images, A))
    assert (fwd, bwd) == (["backbone_forward", "lifter_forward_train"], ["backward_points(dk2d, dref)"])
    assert m.keypoint_head.final_layer.weight.grad is not None
    m.zero_grad(set_to_none=True)


# ---- forward_features ------------------------------------------------------------------------------------------------------------------------
def _maps(m):
    eng = m._engine_at(torch.device("cuda", torch.cuda.current_device()), H, W)
    return [f.cuda() for f in synth_maps(B, [(c, h, w) for h, w, c in eng.feature_shapes()], 17)]


def test_forward_features(head_model, log):
    m = head_model
    maps = _maps(m)
    k2d, kc = _keypoints()
    assert _plain(log, lambda: m.forward_features(maps, k2d, kc.clone()))[0] == ["set_features", "lifter_forward"]
    fwd, bwd, _ = _step(log, lambda: m.forward_features(maps, k2d, kc.clone()))
    assert (fwd, bwd) == (STEP, ["backward_maps"])
    k2d_leaf = k2d.clone().requires_grad_(True)
    fwd, bwd, _ = _step(log, lambda: m.forward_features(maps, k2d_leaf, kc.clone()))
    assert (fwd, bwd) == (STEP, ["backward_points(dfeat, dk2d)"])
    assert k2d_leaf.grad is not None
    m.zero_grad(set_to_none=True)


def test_forward_features_frozen_lifter_one_map_in_the_graph(frozen_lifter, log):
    m = frozen_lifter
    maps = _maps(m)
    maps[1].requires_grad_(True)
    k2d, kc = _keypoints()
    fwd, bwd, _ = _step(log, lambda: m.forward_features(maps, k2d, kc.clone()))
    assert (fwd, bwd) == (STEP, ["backward_maps"])
    assert [f.grad is not None for f in maps] == [False, True, False, False] and maps[1].grad.shape == maps[1].shape
    assert all(p.grad is None for p in m.parameters())


def test_forward_features_sets_the_map_gradient_mode_once(head_model, log):
    m = head_model
    maps = _maps(m)
    k2d, kc = _keypoints()
    eng = m._engine_at(maps[0].device, H, W)
    assert eng.map_grad_mode() == 0
    try:
        m.map_grad_mode = "ordered"
        fwd, bwd, _ = _step(log, lambda: m.forward_features(maps, k2d, kc.clone()))
        assert (fwd, bwd) == (STEP, ["set_map_grad_mode", "backward_maps"])
        for _ in range(2):
            fwd, bwd, _ = _step(log, lambda: m.forward_features(maps, k2d, kc.clone()))
            assert (fwd, bwd) == (STEP, ["backward_maps"])
    finally:
        m.map_grad_mode = None
        eng.set_map_grad_mode(0)
        m.zero_grad(set_to_none=True)


# ---- the flip entries: one backbone pass over the 2B engine frames, whatever the image form ----------------------------------------------------
def _pair_forms(images, crops):
    """(image form, the backbone entry it reaches): float crops, the [2,B,H,W,3] stack of preprocess(mode=2), uint8 crops"""
    return ((images, "backbone_forward"), (torch.stack([images, torch.flip(images, [2])]), "backbone_forward"), (crops, "backbone_forward_u8"))


def test_detect_flip_test(head_model, log):
    m = head_model
    images, A, _ = _inputs(B, H, W)
    crops, _, _ = _inputs(B, H, W, u8=True)
    for form, backbone in _pair_forms(images, crops):
        calls, (kcrop, score, k2d) = _plain(log, lambda: m.detect_flip_test(form, A))
        assert calls == [backbone] and kcrop.shape == (B, J, 2) and score.shape == (B, J) and k2d.shape == (B, J, 2)


def test_forward_detect_flip_test(head_model, log):
    m = head_model
    images, A, _ = _inputs(B, H, W)
    crops, _, _ = _inputs(B, H, W, u8=True)
    for form, backbone in _pair_forms(images, crops):
        calls, (out, kcrop, _) = _plain(log, lambda: m.forward_detect_flip_test(form, A))
        assert calls == [backbone, "lifter_forward"] and out.shape == (B, 1, J, 3) and kcrop.shape == (B, J, 2)


# ---- keypoint_head="cpn": bf16, 256x192 (the smallest crop the CPN module tests use), one source crop ---------------------------------------
CPN_H, CPN_W = 256, 192


@pytest.fixture(scope="module")
def cpn_model():
    """keypoint_head="cpn", warmed up: its 256x192 engine exists and is bound"""
    m = cpn._model("bf16")
    images, A = cpn._inputs(1, CPN_H, CPN_W)
    m.detect(images, A)
    yield m
    cpn._release(m)


def _cpn_inputs(u8=False):
    return cpn._inputs(1, CPN_H, CPN_W, u8=u8)


def test_cpn_detect_and_forward_detect(cpn_model, log):
    m = cpn_model
    images, A = _cpn_inputs()
    assert _plain(log, lambda: m.detect(images, A))[0] == ["backbone_forward"]
    calls, (out, kcrop, score) = _plain(log, lambda: m.forward_detect(images, A))
    assert calls == ["backbone_forward", "lifter_forward"] and out.shape == (1, 1, J, 3) and kcrop.shape == (1, J, 2) and score.shape == (1, J)
    assert any(p.requires_grad for p in m.volume_net.parameters())          # the lifter trains: the native step, the head outside the graph
    m.zero_grad(set_to_none=True)
    fwd, bwd, _ = _step(log, lambda: m.forward_detect(images, A))
    assert (fwd, bwd) == (["backbone_forward", "lifter_forward_train"], ["backward"])
    assert all(p.grad is not None for p in m.volume_net.parameters())
    m.zero_grad(set_to_none=True)


@pytest.mark.parametrize("u8", [False, True], ids=["float", "u8"])
def test_cpn_flip_entries(cpn_model, log, u8):
    m = cpn_model
    images, A = _cpn_inputs(u8)
    backbone = "backbone_forward_u8" if u8 else "backbone_forward"
    calls, (kcrop, score, k2d) = _plain(log, lambda: m.detect_cpn_flip(images, A))
    assert calls == [backbone] and kcrop.shape == (1, J, 2) and score.shape == (1, J) and k2d.shape == (1, J, 2)
    calls, (out, kcrop, _) = _plain(log, lambda: m.forward_detect_cpn_flip(images, A))
    assert calls == [backbone, "lifter_forward"] and out.shape == (1, 1, J, 3) and kcrop.shape == (1, J, 2)
