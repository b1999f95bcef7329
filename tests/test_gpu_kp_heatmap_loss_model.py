"""GPU: CA_PF.keypoint_loss -- one backbone pass, then capf_kp_heatmap_loss on feat0 with detect()'s heatmap <-> crop convention: its gradients
on final_layer are the binding's on the engine's own feat0 bit for bit, nothing else receives a gradient, the state dicts are the parent's,
and 30 plain-SGD steps on the head learn."""
import contextlib
import copy
import io
import json
import os

import numpy as np
import pytest
import torch

import kp_heatmap_oracle as O
from capf import lib as capf
from capf import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
J = 17
SMALLEST = (32, 32)        # the smallest crop a plan accepts (tests/small_geometry_cases.py: feat0 is 8 x 8)


def _model(head, dtype="fp32", wseed=3, backbone="hrnet_32"):
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), backbone)
    cfg.model.backbone.fix_weights = True
    with contextlib.redirect_stdout(io.StringIO()):
        m = CA_PF(cfg, compute_dtype=dtype, keypoint_head=head).eval()
    synth.load_synthetic(m, seed=wseed, bn_mode="random")
    return m


def _release(*models):
    for m in models:
        for e in m._engines.values():
            e.close()
        m._engines.clear()


def _inputs(B, H, W, u8, seed=9):
    g = torch.Generator().manual_seed(seed)
    images = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8) if u8 else torch.randn(B, H, W, 3, generator=g)
    gt = torch.rand(B, J, 2, generator=g) * torch.tensor([W + 8.0, H + 8.0]) - 4.0       # crop pixels, some a little outside the crop
    tw = torch.tensor([1.0, 1.0, 0.5, 0.0])[torch.randint(0, 4, (B, J), generator=g)]
    return images.cuda(), gt.cuda(), tw.cuda()


CASES = [("argmax", "fp32", False, SMALLEST, 3, "mean"), ("integral", "fp32", True, SMALLEST, 3, "ohkm"), ("argmax", "bf16", True, SMALLEST, 3, "mean"),
         ("integral", "bf16", False, SMALLEST, 3, "ohkm"), ("argmax", "fp32", True, (256, 192), 2, "ohkm"), ("integral", "bf16", False, (256, 192), 2, "mean")]


@pytest.mark.parametrize("head,dtype,u8,hw,B,reduction", CASES, ids=[f"{h}-{d}-{'u8' if u else 'float'}-{s[0]}x{s[1]}-{r}" for h, d, u, s, _, r in CASES])
def test_keypoint_loss_gradients_are_the_binding_s_on_feat0(head, dtype, u8, hw, B, reduction):
    H, W = hw
    m = _model(head, dtype).cuda()
    try:
        images, gt, tw = _inputs(B, H, W, u8)
        sigma, topk = (1.0 if hw == SMALLEST else 2.0), 5
        fl = m.keypoint_head.final_layer
        loss = m.keypoint_loss(images, gt, tw, sigma=sigma, reduction=reduction, topk=topk)
        assert loss.dim() == 0 and loss.requires_grad and torch.isfinite(loss)
        loss.backward()
        eng = m._engine_at(images.device, H, W)
        feat0 = eng.tensor_view("feat0", B)
        assert feat0.dtype == {"fp32": torch.float32, "bf16": torch.bfloat16}[dtype]
        h, w = feat0.shape[1], feat0.shape[2]
        want = capf.kp_heatmap_loss(feat0, fl.weight.detach(), fl.bias.detach(), gt, tw, (W / w, 0.0, H / h, 0.0), sigma, reduction, topk, 0.5)
        bits = lambda t: t.contiguous().view(torch.int32)
        assert torch.equal(bits(loss.detach().view(1)), bits(want[0]))
        assert torch.equal(bits(fl.weight.grad.view(J, -1)), bits(want[2])) and torch.equal(bits(fl.bias.grad), bits(want[3]))
        assert fl.weight.grad.abs().max() > 0 and fl.bias.grad.abs().max() > 0                 # the bias gets a real gradient
        # nothing else receives a gradient
        assert all(p.grad is None for p in m.volume_net.parameters()) and all(p.grad is None for p in m.backbone.parameters())
        # a second loss * 3 scales them by 3 (a fresh backbone pass: the same bits)
        g_w, g_b = fl.weight.grad.clone(), fl.bias.grad.clone()
        fl.weight.grad = fl.bias.grad = None
        (m.keypoint_loss(images, gt, tw, sigma=sigma, reduction=reduction, topk=topk) * 3).backward()
        assert torch.equal(bits(fl.weight.grad), bits(g_w * 3)) and torch.equal(bits(fl.bias.grad), bits(g_b * 3))
        # without grad: the same loss, no graph
        with torch.no_grad():
            plain = m.keypoint_loss(images, gt, tw, sigma=sigma, reduction=reduction, topk=topk)
        assert not plain.requires_grad and torch.equal(bits(plain.view(1)), bits(want[0]))
    finally:
        _release(m)


def test_state_dict_keys_are_the_parent_s_for_every_head():
    schema = lambda bb: set(json.load(open(os.path.join(ROOT, "tests", "golden", f"schema_{bb}.json"))))
    head_keys = {"keypoint_head.final_layer.weight", "keypoint_head.final_layer.bias"}
    assert set(_model(None).state_dict()) == schema("hrnet_32")
    for head in ("argmax", "integral"):
        assert set(_model(head).state_dict()) == schema("hrnet_32") | head_keys
    assert set(_model("cpn", backbone="cpn").state_dict()) == schema("cpn")


def test_mpi_variant_and_the_free_function():
    from model.conpose import VolumetricTriangulationNet, mpi_preset
    from mvn.models.conpose import keypoint_heatmap_loss
    from mvn.utils.cfg import config
    with contextlib.redirect_stdout(io.StringIO()):
        m = VolumetricTriangulationNet(mpi_preset(copy.deepcopy(config), "hrnet_32"), keypoint_head="argmax").eval()
    synth.load_synthetic(m, seed=3, bn_mode="random")
    m = m.cuda()
    try:
        H, W = SMALLEST
        images, gt, tw = _inputs(2, H, W, False)
        loss = m.keypoint_loss(images, gt, tw, sigma=1.0)
        loss.backward()
        fl = m.keypoint_head.final_layer
        assert loss.dim() == 0 and fl.weight.grad.abs().max() > 0 and fl.bias.grad.abs().max() > 0
        # the free function on a map of the caller's: gradients to weight, bias and an fp32 map; a 16-bit map that requires grad raises
        feat = torch.randn(2, 8, 8, 32, device="cuda", generator=torch.Generator("cuda").manual_seed(4)).requires_grad_(True)
        w, b = fl.weight.detach().clone().requires_grad_(True), fl.bias.detach().clone().requires_grad_(True)
        out = keypoint_heatmap_loss(feat, w, b, gt, tw, decode=(4.0, 0.0, 4.0, 0.0), sigma=1.0, reduction="ohkm", topk=3)
        (out * 2).backward()
        ref = capf.kp_heatmap_loss(feat.detach(), w.detach(), b.detach(), gt, tw, (4.0, 0.0, 4.0, 0.0), 1.0, "ohkm", 3, want_dmap=True)
        for got, want in ((feat.grad, ref[4]), (w.grad.view(J, -1), ref[2]), (b.grad, ref[3])):
            assert torch.equal(got, want * 2)
        with pytest.raises(NotImplementedError, match="fp32 map"):
            keypoint_heatmap_loss(feat.detach().to(torch.bfloat16).requires_grad_(True), w, b, gt, tw, decode=(4.0, 0.0, 4.0, 0.0), sigma=1.0)
    finally:
        _release(m)


def test_thirty_sgd_steps_on_the_head_learn():
    """One fixed seed, three frames at the smallest crop, ground truth at cell centres: for joint j the cell where the j-th most active
    channel of feat0 peaks (something a 1x1 conv on feat0 can point at), never cell (0, 0), where the decode parks a joint without a
    positive logit.  The head starts from the checkpoint's random final_layer scaled to 1 %: 30 steps cannot undo a random start's weight
    in the directions feat0 barely spans (the Hessian's eigenvalues fall by 80 x after the first), and those decide an argmax.
    The loss is a convex quadratic in (weight, bias) with Hessian (2 scale / (H W B J)) sum [x; 1][x; 1]^T per joint, so plain gradient
    descent with step 1 / lambda_max decreases it at every step: the float64 oracle on the same feat0 does (asserted), by more than 0.1 % a
    step, far above fp32 rounding -- and so must the GPU loss.  Afterwards the argmax decode hits the ground-truth cell on strictly more
    (frame, joint) items than before training (on the CPU oracle's feat0: 0 -> 23 of 51)."""
    H, W = SMALLEST
    B, steps, sigma = 3, 30, 1.0
    m = _model("argmax").cuda()
    try:
        images = _inputs(B, H, W, False)[0]
        fl = m.keypoint_head.final_layer
        with torch.no_grad():
            m.detect(images)
            x = m._engine_at(images.device, H, W).tensor_view("feat0", B).clone()
        h, w, C = x.shape[1:]
        x64 = x.cpu().to(torch.float64).numpy()
        with torch.no_grad():
            fl.weight *= 0.01
            fl.bias *= 0.01
        peaks = x64.reshape(B, -1, C).argmax(1)                                              # [B, C]
        chans = [c for c in np.argsort(-x64.reshape(-1, C).std(0), kind="stable") if (peaks[:, c] != 0).all()][:J]
        assert len(chans) == J
        peak = peaks[:, chans]                                                               # [B, J]
        cells = np.stack([peak % w, peak // w], -1)
        decode = (W / w, 0.0, H / h, 0.0)
        gt = torch.tensor(cells * np.array([decode[0], decode[2]]), dtype=torch.float32).cuda()
        xt = np.concatenate([x64.reshape(-1, C), np.ones((B * h * w, 1))], 1)
        lr = 1.0 / np.linalg.eigvalsh(2 * 0.5 / (h * w * B * J) * xt.T @ xt)[-1]

        def hits(kcrop):
            cell = torch.round(kcrop.cpu().to(torch.float64) / torch.tensor([decode[0], decode[2]])).numpy()
            return int((cell == cells).all(-1).sum())

        # the oracle side: float64 gradient descent on the same data
        W64, b64 = fl.weight.detach().cpu().to(torch.float64).numpy().reshape(J, C).copy(), fl.bias.detach().cpu().to(torch.float64).numpy().copy()
        ref = []
        for _ in range(steps):
            z = np.einsum("byxc,jc->bjyx", x64, W64) + b64[None, :, None, None]
            r = O.evaluate(z, x64, None, gt.cpu().numpy(), None, decode, sigma)
            ref.append(r["loss"])
            W64 -= lr * r["dweight"]
            b64 -= lr * r["dbias"]
        assert all(b < a * (1 - 1e-3) for a, b in zip(ref, ref[1:])), ref

        with torch.no_grad():
            before = hits(m.detect(images)[0])
        losses = []
        for _ in range(steps):
            fl.weight.grad = fl.bias.grad = None
            loss = m.keypoint_loss(images, gt, sigma=sigma)
            loss.backward()
            losses.append(loss.item())
            with torch.no_grad():
                fl.weight -= lr * fl.weight.grad
                fl.bias -= lr * fl.bias.grad
        with torch.no_grad():
            after = hits(m.detect(images)[0])
        print(f"loss {losses[0]:.6f} -> {losses[-1]:.6f} (oracle {ref[0]:.6f} -> {ref[-1]:.6f}); hits {before} -> {after} of {B * J}")
        assert all(b < a for a, b in zip(losses, losses[1:])), losses
        assert abs(losses[-1] - ref[-1]) < 1e-3 * ref[-1]
        assert after > before
    finally:
        _release(m)
