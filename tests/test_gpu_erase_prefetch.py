"""GPU: data_prefetcher(erase=...) -- the occlusion in front of the prefetcher's native launch pair.

erase=None is today's prefetcher bit for bit; with a seeded generator the image slot is preprocess(erase_patches(images, kcrop, mask), ...)
for the mask the same seed draws, the labels are the no-erase labels, fused_input hands out the erased uint8 batch, and forward_u8 on that
batch equals forward on its preprocessed form."""
import random

import pytest
import torch

import erase_oracle
from capf import lib as capf

pytestmark = pytest.mark.gpu

J = 17
MODES = [(0, False, False, 0.0), (1, True, False, 0.25), (2, False, True, 0.0)]          # capf_preprocess mode, is_train, flip_test, the coin


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t.contiguous()


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _batch(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8), torch.randn(B, 1, J, 3, generator=g),
            torch.rand(B, J, 2, generator=g) * 2 - 1, torch.rand(B, J, 2, generator=g) * torch.tensor([W + 3.0, H + 3.0]) - 1.5)


def _device():
    return torch.device("cuda", torch.cuda.current_device())


def _direct(batch, mode, images=None):
    """capf.preprocess called directly, in the layout the prefetcher hands out"""
    img, gt, k2d, kc = (t.cuda() for t in batch)
    x, g, a, b = capf.preprocess(img if images is None else images, gt, k2d, kc, "hrnet_32", mode)
    if mode == 2:
        x, a, b = x.transpose(0, 1), a.transpose(0, 1), b.transpose(0, 1)
    return x, g, a, b


def _generator(seed):
    return torch.Generator(device=_device()).manual_seed(seed)


@pytest.mark.parametrize("mode,is_train,flip_test,coin", MODES)
@pytest.mark.parametrize("erase", [None, False])
def test_without_erase_the_prefetcher_is_preprocess(monkeypatch, mode, is_train, flip_test, coin, erase):
    from mvn.datasets.utils import data_prefetcher
    monkeypatch.setattr(random, "random", lambda: coin)
    called = []
    monkeypatch.setattr(capf, "erase_patches", lambda *a, **k: called.append(a))
    batch = _batch(3, 64, 48, seed=31)
    pf = data_prefetcher([batch], _device(), is_train, flip_test, "hrnet_32", erase=erase)
    got = pf.next()
    assert pf.next() is None and pf.erase is None and pf.erase_mask is None and not called
    for g, w in zip(got, _direct(batch, mode)):
        assert _same(g, w)


@pytest.mark.parametrize("mode,is_train,flip_test,coin", MODES)
@pytest.mark.parametrize("options", [True, {"size": 15, "use_mean": False, "prob": 0.3}], ids=["defaults", "size15-zero-p0.3"])
def test_seeded_erase_is_erase_patches_then_preprocess(monkeypatch, mode, is_train, flip_test, coin, options):
    from mvn.datasets.utils import data_prefetcher
    monkeypatch.setattr(random, "random", lambda: coin)
    B, H, W, seed = 3, 64, 48, 77
    batch = _batch(B, H, W, seed=32)
    opts = dict({} if options is True else options, generator=_generator(seed))
    size, use_mean, prob = opts.get("size", 70), opts.get("use_mean", True), opts.get("prob", 0.5)
    mask = (torch.rand(B, J, device=_device(), generator=_generator(seed)) < prob).to(torch.uint8)          # what the same seed draws
    assert 0 < int(mask.sum()) < B * J
    erased = capf.erase_patches(batch[0].cuda(), batch[3].cuda(), mask, size, use_mean)
    assert not torch.equal(erased.cpu(), batch[0])
    assert torch.equal(erased.cpu(), torch.from_numpy(erase_oracle.erase_batch(batch[0].numpy(), batch[3].numpy(), mask.cpu().numpy(), size, use_mean)))
    want = _direct(batch, mode, erased)
    plain = _direct(batch, mode)

    pf = data_prefetcher([batch], _device(), is_train, flip_test, "hrnet_32", erase=opts)
    got = pf.next()
    assert torch.equal(pf.erase_mask, mask) and pf.next() is None
    assert _same(got[0], want[0]) and not _same(got[0], plain[0])
    for g, w in zip(got[1:], plain[1:]):                                   # the labels: untouched
        assert _same(g, w)

    opts["generator"] = _generator(seed)
    fused = data_prefetcher([batch], _device(), is_train, flip_test, "hrnet_32", fused_input=True, erase=opts)
    crops, gt8, k2d8, kc8 = fused.next()
    assert fused.mirror == ("none", "all", "pair")[mode] and torch.equal(fused.erase_mask, mask)
    assert crops.dtype == torch.uint8 and torch.equal(crops, erased)
    assert _same(gt8, plain[1]) and _same(k2d8, plain[2].transpose(0, 1).reshape(-1, J, 2) if mode == 2 else plain[2])
    assert _same(kc8, plain[3].transpose(0, 1).reshape(-1, J, 2) if mode == 2 else plain[3])


def test_listed_joints_are_erased_in_every_frame():
    from mvn.datasets.utils import data_prefetcher
    B, H, W = 2, 64, 48
    batch = _batch(B, H, W, seed=33)
    pf = data_prefetcher([batch], _device(), False, False, "hrnet_32", fused_input=True, erase={"joints": [16, 0, 9], "size": 11})
    crops = pf.next()[0]
    mask = torch.zeros(B, J, dtype=torch.uint8)
    mask[:, [0, 9, 16]] = 1
    assert torch.equal(pf.erase_mask.cpu(), mask)
    assert torch.equal(crops.cpu(), torch.from_numpy(erase_oracle.erase_batch(batch[0].numpy(), batch[3].numpy(), mask.numpy(), 11, True)))


@pytest.fixture(scope="module")
def host_model():
    from conftest import make_model
    return make_model("hrnet_32", device="cuda", wseed=9)[0]


@pytest.mark.parametrize("mirror,mode", [("none", 0), ("all", 1), ("pair", 2)])
def test_forward_u8_on_the_erased_batch_equals_forward_on_its_preprocessed_form(host_model, mirror, mode):
    """hrnet_32 at a 32 x 32 crop (tests/small_geometry_cases.py), batch 2"""
    model = host_model
    B, H, W = 2, 32, 32
    img, gt, k2d, kc = (t.cuda() for t in _batch(B, H, W, seed=34))
    kc = kc.clamp(0.0, W - 1.0)
    erased = capf.erase_patches(img, kc, None, 9, True)
    assert not torch.equal(erased, img)
    frames = 2 * B if mode == 2 else B
    with torch.no_grad():
        x, _, a, b = capf.preprocess(erased, gt, k2d, kc, "hrnet_32", mode)
        want = model(x.view(frames, H, W, 3), a.view(frames, J, 2), b.view(frames, J, 2).clone())
        got = model.forward_u8(erased, a.view(frames, J, 2), b.view(frames, J, 2).clone(), mirror=mirror)
        other = model.forward_u8(img, a.view(frames, J, 2), b.view(frames, J, 2).clone(), mirror=mirror)
    assert got.shape == (frames, 1, J, 3) and _same(got, want) and not _same(other, want)

