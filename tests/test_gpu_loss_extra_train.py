"""GPU: the new losses as training criteria of the native step.  CA_PF, HRNet-32, fp32, 64x64 crops, batch 2 (the smallest geometry the
session tests use), DropPath off: one forward under grad, backward() through the loss's autograd node and the lifter's, one SGD step.  The
gradients must be finite and the lifter's parameters must move."""
import pytest
import torch

from capf import synth
from conftest import make_model

pytestmark = pytest.mark.gpu
B, H, W = 2, 64, 64


@pytest.fixture(scope="module")
def model():
    m, _ = make_model("hrnet_32", device="cuda", wseed=5)
    m.train()
    m.backbone.eval()
    m.drop_path_rate = 0.0
    yield m
    for e in m._engines.values():
        e.close()
    m._engines.clear()


def _inputs(seed):
    img, k2d, kc, gt = synth.synth_inputs(B, H, W, seed=seed, crop_range=(W, H), with_gt=True)
    return img.cuda(), k2d.cuda(), kc.cuda(), gt.cuda()


def _one_step(model, criterion, seed):
    """-> (loss, whether more than half of the lifter's parameter tensors changed)"""
    params = [p for p in model.volume_net.parameters() if p.requires_grad]
    before = [p.detach().clone() for p in params]
    opt = torch.optim.SGD(params, lr=1e-2)
    opt.zero_grad(set_to_none=True)
    img, k2d, kc, gt = _inputs(seed)
    out = model(img, k2d, kc)
    assert out.shape == (B, 1, 17, 3) and out.requires_grad
    loss = criterion(out, gt)
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    loss.backward()
    grads = [p.grad for p in params]
    assert all(g is not None and bool(torch.isfinite(g).all()) for g in grads)
    assert any(bool((g != 0).any()) for g in grads)
    opt.step()
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(p).all()) for p in params)
    moved = sum(int(not torch.equal(a, p.detach())) for a, p in zip(before, params))
    return loss.item(), moved > len(params) // 2


def test_one_step_on_mpjpe_plus_limb_length_loss(model):
    from mvn.models.loss import MPJPE, limb_length_loss
    mpjpe = MPJPE()
    seen = {}

    def criterion(out, gt):
        seen["mpjpe"], seen["limb"] = mpjpe(out, gt), limb_length_loss(out, gt)
        return seen["mpjpe"] + 0.1 * seen["limb"]

    loss, moved = _one_step(model, criterion, seed=21)
    assert seen["limb"].item() > 0 and abs(loss - (seen["mpjpe"].item() + 0.1 * seen["limb"].item())) <= 1e-6 * loss
    assert moved


def test_one_step_on_keypoints_l2_loss_under_a_mask_with_zeros(model):
    from mvn.models.loss import KeypointsL2Loss
    validity = torch.ones(B, 17, 1, device="cuda")
    validity[0, 3] = validity[1, 0] = validity[1, 16] = 0.0
    l2 = KeypointsL2Loss()
    # the reference's own expression on the same tensors: its gradient is NaN as soon as the mask holds a zero
    img, k2d, kc, gt = _inputs(22)
    with torch.no_grad():
        out = model(img, k2d, kc)[:, 0]
    probe = out.clone().requires_grad_(True)
    torch.sum(torch.sqrt(torch.sum((gt[:, 0] - probe) ** 2 * validity, dim=2))).backward()
    assert bool(torch.isnan(probe.grad).any())
    loss, moved = _one_step(model, lambda out, gt: l2(out[:, 0], gt[:, 0], validity), seed=22)
    assert loss > 0 and moved
