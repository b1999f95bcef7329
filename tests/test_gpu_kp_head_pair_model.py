"""GPU: the flip test with the native head inside the model -- CA_PF(keypoint_head=...).detect_flip_test / forward_detect_flip_test and
VolumetricTriangulationNet's pass-throughs.  HRNet-32 at 64x64 and 128x96, batch 2-3, synthetic weights as in test_gpu_kp_head_model.py.
Every comparison is a bit equality between two routes of the library; the paired head itself is held to its yardstick in
test_gpu_kp_head_pair.py."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import kp_head_cases as K  # noqa: F401  (the head's yardstick: the stand-alone tests of this entry use it)
from capf import lib as capf
from capf import synth

pytestmark = pytest.mark.gpu
J = 17


def _model(head, dtype="fp32", wseed=3, beta=2.0, mpi=False, **kw):
    from mvn.utils.cfg import backbone_preset, config
    with contextlib.redirect_stdout(io.StringIO()):
        if mpi:
            from model.conpose import VolumetricTriangulationNet, mpi_preset
            cfg = mpi_preset(copy.deepcopy(config), "hrnet_32")
            m = VolumetricTriangulationNet(cfg, compute_dtype=dtype, keypoint_head=head, keypoint_beta=beta, **kw).eval()
        else:
            from mvn.models.conpose import CA_PF
            cfg = backbone_preset(copy.deepcopy(config), "hrnet_32")
            cfg.model.backbone.fix_weights = True
            m = CA_PF(cfg, compute_dtype=dtype, keypoint_head=head, keypoint_beta=beta, **kw).eval()
    synth.load_synthetic(m, seed=wseed, bn_mode="random")
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
    return images.cuda(), A.cuda()


def _given(B, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(B, J, 2, generator=g).cuda() * 2 - 1, (torch.rand(B, J, 2, generator=g) * 190).cuda()


# ---- 1. forward_detect_flip_test == forward_flip_test on detect_flip_test's keypoints ------------------------------------------------------
@pytest.mark.parametrize("dtype,u8,head,H,W", [("fp32", False, "argmax", 64, 64), ("fp32", True, "integral", 128, 96), ("fp16", False, "integral", 128, 96)],
                         ids=["fp32-float-argmax-64x64", "fp32-u8-integral-128x96", "fp16-float-integral-128x96"])
def test_forward_detect_flip_test_equals_forward_flip_test_on_detected_keypoints(dtype, u8, head, H, W):
    B = 3
    m, fresh = _model(head, dtype), _model(head, dtype)
    try:
        images, A = _inputs(B, H, W, u8=u8)
        kcrop, score, k2d = m.detect_flip_test(images, A)
        assert kcrop.shape == (B, J, 2) and score.shape == (B, J) and k2d.shape == (B, J, 2)
        assert not (kcrop.requires_grad or score.requires_grad or k2d.requires_grad)           # under grad mode, trainable head: detached all the same
        assert torch.isfinite(kcrop).all() and torch.isfinite(score).all() and torch.isfinite(k2d).all()
        k_only, s_only, none = m.detect_flip_test(images)
        assert none is None and torch.equal(k_only, kcrop) and torch.equal(s_only, score)
        # the flag reaches the kernel: some keypoint moves without the one-column shift
        assert not torch.equal(m.detect_flip_test(images, A, shift=False)[0], kcrop)
        out, kc2, sc2 = m.forward_detect_flip_test(images, A)
        assert out.shape == (B, 1, J, 3) and not out.requires_grad
        assert torch.equal(kc2, kcrop) and torch.equal(sc2, score)                             # still pixels: the lifter normalised a copy
        _, k2d2, kcrop2 = capf.preprocess_points(None, k2d, kcrop, mode=2)
        with torch.no_grad():
            if u8:
                pred = m.forward_u8(images, k2d2.view(2 * B, J, 2), kcrop2.clone().view(2 * B, J, 2), mirror="pair")
                want = capf.fliptest_fuse(pred.view(2, B, 1, J, 3))
            else:
                want = m.forward_flip_test(torch.stack([images, torch.flip(images, [2])]), k2d2, kcrop2.clone())
            assert torch.equal(out, want)
            # the H36M table given by name: the same bits as the default
            o2, k3, s3 = m.forward_detect_flip_test(images, A, flip_pairs=capf.H36M_SWAP)
            assert torch.equal(o2, out) and torch.equal(k3, kcrop) and torch.equal(s3, score)
            # the engine stays usable: a plain forward right after either method has a fresh engine's bits
            fwd = m.forward_u8 if u8 else m.forward
            k2d_given, kc_given = _given(B)
            for call in (lambda: m.detect_flip_test(images, A), lambda: m.forward_detect_flip_test(images, A)):
                call()
                assert torch.equal(fwd(images, k2d_given, kc_given.clone()), getattr(fresh, fwd.__name__)(images, k2d_given, kc_given.clone()))
    finally:
        _release(m, fresh)


# ---- 2. the three forms of `images`; the head on the engine's own map ------------------------------------------------------------------------
@pytest.mark.parametrize("head,H,W", [("argmax", 128, 96), ("integral", 64, 64)])
def test_uint8_float_and_stack_give_the_same_bits_and_the_entry_s_on_feat0(head, H, W):
    B = 2
    m = _model(head)
    try:
        images_u8, A = _inputs(B, H, W, u8=True)
        k2d_given, kc_given = _given(B)
        imgf = capf.preprocess(images_u8, None, k2d_given, kc_given, "hrnet_32", 0)[0]
        stack = capf.preprocess(images_u8, None, k2d_given, kc_given, "hrnet_32", 2)[0]
        assert imgf.shape == (B, H, W, 3) and stack.shape == (2, B, H, W, 3)
        ref = m.forward_detect_flip_test(images_u8, A)
        det = m.detect_flip_test(images_u8, A)
        assert torch.equal(det[0], ref[1]) and torch.equal(det[1], ref[2])
        for images in (imgf, stack):
            got = m.forward_detect_flip_test(images, A)
            assert all(torch.equal(g, r) for g, r in zip(got, ref))
            assert all(torch.equal(g, r) for g, r in zip(m.detect_flip_test(images, A), det))
        # detect_flip_test = capf_kp_head_forward_pair on feat0 of a mode-2 backbone pass
        eng = m.engine_for(images_u8)
        mean, std = capf.input_constants("hrnet_32")
        with torch.no_grad():
            eng.backbone_forward_u8(images_u8, mean, std, 2, torch.cuda.current_stream().cuda_stream)
            feat0 = eng.tensor_view("feat0", 2 * B)
            fl = m.keypoint_head.final_layer
            decode = (float(W) / feat0.shape[2], 0.0, float(H) / feat0.shape[1], 0.0)
            for shift in (True, False):
                kcrop2, score, k2d2, _ = capf.kp_head_forward_pair(feat0, fl.weight.detach(), fl.bias.detach(), capf.KP_MODES[head], m.keypoint_beta,
                                                                   None, shift, decode, A)
                kc, sc, kd = m.detect_flip_test(images_u8, A, shift=shift)          # (leaves the same feat0 behind for the next round)
                assert torch.equal(kcrop2[0], kc) and torch.equal(score, sc) and torch.equal(k2d2[0], kd)
    finally:
        _release(m)


def test_symmetric_head_without_shift_stays_inside_the_crop():
    """With W[swap[j]] = W[j] and no shift the fused logits equal the single ones up to the backbone's own left / right asymmetry: no
    equality with detect() holds, only that the outputs are finite and inside the crop."""
    B, H, W = 2, 64, 64
    m = _model("argmax")
    try:
        with torch.no_grad():
            w = m.keypoint_head.final_layer.weight
            w.copy_(0.5 * (w + w[list(capf.H36M_SWAP)]))
            b = m.keypoint_head.final_layer.bias
            b.copy_(0.5 * (b + b[list(capf.H36M_SWAP)]))
        images, A = _inputs(B, H, W)
        for head in ("argmax", "integral"):
            m.keypoint_head_mode = head
            kcrop, score, k2d = m.detect_flip_test(images, A, shift=False)
            assert torch.isfinite(kcrop).all() and torch.isfinite(score).all() and torch.isfinite(k2d).all()
            assert (kcrop[..., 0] >= 0).all() and (kcrop[..., 0] <= W).all() and (kcrop[..., 1] >= 0).all() and (kcrop[..., 1] <= H).all()
    finally:
        _release(m)


# ---- 3. the variant without context blocks ------------------------------------------------------------------------------------------------
def test_mpi_variant_passes_through_with_its_own_skeleton():
    B, H, W = 2, 64, 64
    m = _model("integral", mpi=True)
    try:
        images, A = _inputs(B, H, W)
        kcrop, score, k2d = m.detect_flip_test(images, A)
        x, kc, sc = m.forward_detect_flip_test(images, A)
        assert x.shape == (B, 3, 1, J, 1) and torch.equal(kc, kcrop) and torch.equal(sc, score)
        # the same through today's route: the stacks by hand with the 3DHP table, then forward_flip_test (capf_fliptest_fuse_swap with it)
        idx = list(capf.MPI_SWAP)
        kcrop2 = torch.stack([kcrop, torch.stack([(192.0 - kcrop[:, idx, 0]) - 1.0, kcrop[:, idx, 1]], -1)]).contiguous()
        k2d2 = torch.stack([k2d, torch.stack([-k2d[:, idx, 0], k2d[:, idx, 1]], -1)]).contiguous()
        with torch.no_grad():
            want, none = m.forward_flip_test(torch.stack([images, torch.flip(images, [2])]), k2d2, kcrop2.clone())
        assert none is None and torch.equal(x, want)
        # the H36M table is another skeleton: asking for it by name changes the result
        assert not torch.equal(m.detect_flip_test(images, A, flip_pairs=capf.H36M_SWAP)[0], kcrop)
    finally:
        _release(m)


# ---- 4. refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals_raise_with_their_reason():
    B, H, W = 2, 64, 64
    images, A = _inputs(B, H, W)
    m = _model("argmax")
    none = _model(None)
    bn = _model("integral", backbone_bn="batch")
    try:
        for call in (m.detect_flip_test, m.forward_detect_flip_test):
            with pytest.raises(ValueError, match="NHWC"):
                call(torch.zeros(B, 3, H, W, device="cuda"), A)
            with pytest.raises(ValueError, match="to_image must be a float32 tensor \\[2, 2, 3\\]"):
                call(images, torch.zeros(2 * B, 2, 3, device="cuda"))                # one matrix per SOURCE frame
            with pytest.raises(ValueError, match="to_image must be a float32 tensor \\[2, 2, 3\\]"):
                call(torch.stack([images, images]), torch.zeros(2 * B, 2, 3, device="cuda"))
            with pytest.raises(ValueError, match="to_image is on cpu"):
                call(images, A.cpu())
            with pytest.raises(TypeError, match="float32 or uint8"):
                call(images.half(), A)
            with pytest.raises(TypeError, match="stack"):
                call(torch.stack([images, images, images]), A)
            with pytest.raises(ValueError, match="flip_pairs"):
                call(images, A, flip_pairs=(1, 0))
        with pytest.raises(ValueError, match="needs to_image"):
            m.forward_detect_flip_test(images, None)
        with pytest.raises(capf.CapfError, match="no keypoint head"):
            none.detect_flip_test(images, A)
        with pytest.raises(capf.CapfError, match="no keypoint head"):
            none.forward_detect_flip_test(images, A)
        bn.train()
        with pytest.raises(NotImplementedError, match="backbone.eval\\(\\)"):
            bn.forward_detect_flip_test(images, A)
        bn.backbone.eval()                                                           # the way out the message names
        out, _, _ = bn.forward_detect_flip_test(images, A)
        assert torch.isfinite(out).all()
    finally:
        _release(m, none, bn)
