"""GPU: capf_erase_patches (csrc/erase.hip) against the integer restatement of the reference's erase_image (tests/erase_oracle.py), bit for bit.

No tolerance anywhere: the operation is integer.  Shapes: 1 x 1 and 5 x 7 (a frame that is no multiple of 16 bytes: the pixel-per-thread paint
kernel), 16 x 12, 64 x 48 and 256 x 192 (the 16-bytes-per-thread one, more than one block a frame from 64 x 48 on); P = 1, 17 (the skeleton)
and 32 (the cap); B = 1 and 3."""
import ctypes

import numpy as np
import pytest
import torch

import erase_oracle
from capf import lib as capf
from test_erase_api import golden_cases

pytestmark = pytest.mark.gpu

NAN, INF = float("nan"), float("inf")
BAND = 0xA5


def _images(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)


def _specials(H, W):
    """the centres of the rule's edges: (x, y) with one coordinate on an edge value and the other inside, the non-finite ones, 1e30"""
    xin, yin = (W - 1) * 0.5, (H - 1) * 0.5
    return [(-0.5, yin), (-1.0, yin), (W - 0.25, yin), (float(W), yin), (xin, -0.5), (xin, -1.0), (xin, H - 0.25), (xin, float(H)),
            (NAN, yin), (xin, INF), (-INF, yin), (1e30, yin), (xin, -1e30), (W - 0.25, H - 0.25)]


def _centre_sets(B, H, W, P, seed):
    """fp32 [B, P, 2] tensors that between them hold every special centre, random ones inside and just outside the image, and repeats"""
    rng = np.random.RandomState(seed)
    sp = _specials(H, W)
    rand = lambda n: np.stack([rng.uniform(-2.0, W + 2.0, n), rng.uniform(-2.0, H + 2.0, n)], axis=1)
    inside = lambda n: np.stack([rng.uniform(0.0, W, n), rng.uniform(0.0, H, n)], axis=1)
    sets = []
    if P == 1:
        for k in range(0, len(sp), B):
            sets.append(np.array([[sp[(k + b) % len(sp)]] for b in range(B)]))
        sets.append(inside(B).reshape(B, 1, 2))
    else:
        c = np.empty((B, P, 2))
        repeats = 1 if P < 32 else 3
        for b in range(B):
            base = np.concatenate([np.array(sp), inside(P - len(sp) - repeats - 1), rand(1)])
            base = base[rng.permutation(len(base))]
            row = np.concatenate([base, base[:repeats]])         # repeated centres: the last one wins
            if repeats > 1:
                row[[10, P - 2]] = row[[P - 2, 10]]              # ... one of them in the middle of the list
            c[b] = row
        sets.append(c)
    return [torch.from_numpy(s.astype(np.float32)) for s in sets]


SHAPES = [(1, 1), (5, 7), (16, 12), (64, 48), (256, 192)]


@pytest.mark.parametrize("P", [1, 17, 32])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_kernel_equals_the_restatement(H, W, B, P):
    images = _images(B, H, W, seed=1000 * H + 10 * B + P)
    img_np, dev = images.numpy(), images.cuda()
    rng = np.random.RandomState(H + P)
    checked = 0
    for centres in _centre_sets(B, H, W, P, seed=7 * H + B + P):
        cen_dev, cen_np = centres.cuda(), centres.numpy()
        if P > 1:       # every special centre is there, and so are repeats
            assert np.isnan(cen_np).any() and np.isinf(cen_np).any() and (cen_np == 1e30).any() and (cen_np[:, :, 0] == -0.5).any()
            assert (cen_np[:, :, 0] == -1.0).any() and (cen_np[:, :, 0] == W - 0.25).any() and (cen_np[:, :, 0] == W).any()
            assert all(len({tuple(p) for p in f.tolist() if p[0] == p[0]}) < P - 1 for f in cen_np)
        masks = [None, np.zeros((B, P), np.uint8), (rng.rand(B, P) < 0.6).astype(np.uint8) * rng.randint(1, 256, (B, P)).astype(np.uint8)]
        for size in (0, 1, 2, 3, 7, 70, 71, 2 * max(H, W) + 3):
            for use_mean in (True, False):
                for mask in masks:
                    got = capf.erase_patches(dev, cen_dev, None if mask is None else torch.from_numpy(mask).cuda(), size, use_mean)
                    want = erase_oracle.erase_batch(img_np, cen_np, mask, size, use_mean)
                    assert got.dtype == torch.uint8 and got.shape == dev.shape
                    assert torch.equal(got.cpu(), torch.from_numpy(want)), (size, use_mean, None if mask is None else mask.tolist())
                    if mask is not None and not mask.any():
                        assert torch.equal(got, dev)
                    checked += 1
    assert torch.equal(dev.cpu(), images) and checked >= 48


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_kernel_equals_the_reference_on_the_golden(case):
    name, image, centres, size, use_mean, want = case
    dev = torch.from_numpy(image).cuda()[None]
    cen = torch.from_numpy(centres.astype(np.float32)).cuda().view(1, -1, 2)
    got = capf.erase_patches(dev, cen, None, size, use_mean)
    assert torch.equal(got[0].cpu(), torch.from_numpy(want))


def _banded(nbytes, front):
    """a uint8 buffer of BAND bytes with a view of nbytes starting `front` bytes in: (buffer, view)"""
    buf = torch.full((front + nbytes + 64,), BAND, dtype=torch.uint8, device="cuda")
    return buf, buf[front:front + nbytes]


def _bands_intact(buf, front, nbytes):
    return bool((buf[:front] == BAND).all()) and bool((buf[front + nbytes:] == BAND).all())


@pytest.mark.parametrize("H,W,front", [(16, 12, 64), (16, 12, 61), (64, 48, 64), (64, 48, 3), (5, 7, 64), (5, 7, 1), (1, 1, 2)])
def test_in_place_guard_bands_and_repeat(H, W, front):
    """through the C entry with the caller's own buffers: out and scratch sit between guard bands (out at a 16-byte aligned and at a
    misaligned base: both paint kernels at every shape that has both), in place gives the out-of-place bits, a second run the first's"""
    B, P, size = 3, 17, 7
    lib = capf.load_library()
    images = _images(B, H, W, seed=H * W + front)
    centres = _centre_sets(B, H, W, P, seed=front)[0]
    mask = (torch.rand(B, P, generator=torch.Generator().manual_seed(front)) < 0.7).to(torch.uint8)
    n = B * H * W * 3
    need = lib.capf_erase_scratch_bytes(B, P)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    cen_dev, mask_dev = centres.cuda(), mask.cuda()
    for use_mean in (1, 0):
        want = torch.from_numpy(erase_oracle.erase_batch(images.numpy(), centres.numpy(), mask.numpy(), size, bool(use_mean))).view(-1)
        src_buf, src = _banded(n, front)
        src.copy_(images.view(-1))
        outs = []
        for run in range(2):
            out_buf, out = _banded(n, front)
            scr_buf, scr = _banded(need, 64)
            assert lib.capf_erase_patches(stream, p(src), B, H, W, p(cen_dev), p(mask_dev), P, size, use_mean, p(out), p(scr), need) == 0
            torch.cuda.synchronize()
            assert _bands_intact(out_buf, front, n) and _bands_intact(scr_buf, 64, need) and _bands_intact(src_buf, front, n)
            assert torch.equal(src.cpu(), images.view(-1)) and torch.equal(out.cpu(), want)
            outs.append(out.clone())
        assert torch.equal(outs[0], outs[1])
        scr_buf, scr = _banded(need, 64)
        assert lib.capf_erase_patches(stream, p(src), B, H, W, p(cen_dev), p(mask_dev), P, size, use_mean, p(src), p(scr), need) == 0
        torch.cuda.synchronize()
        assert _bands_intact(src_buf, front, n) and _bands_intact(scr_buf, 64, need) and torch.equal(src, outs[0])


def test_binding_in_place_and_out_argument():
    images = _images(3, 64, 48, seed=2).cuda()
    centres = _centre_sets(3, 64, 48, 17, seed=2)[0].cuda()
    want = capf.erase_patches(images, centres, None, 70, True)
    assert not torch.equal(want, images)
    out = torch.empty_like(images)
    assert capf.erase_patches(images, centres, None, 70, True, out=out) is out and torch.equal(out, want)
    work = images.clone()
    assert capf.erase_patches(work, centres, None, 70, True, out=work) is work and torch.equal(work, want)
    bools = torch.ones(3, 17, dtype=torch.bool, device="cuda")
    assert torch.equal(capf.erase_patches(images, centres, bools, 70, True), want)
    empty = capf.erase_patches(images, centres[:, :0], None, 70, True)
    assert torch.equal(empty, images) and empty.data_ptr() != images.data_ptr()


def test_refusals_on_device_buffers():
    B, H, W, P = 2, 16, 12, 17
    n = B * H * W * 3
    buf = torch.zeros(2 * n, dtype=torch.uint8, device="cuda")
    images = buf[:n].view(B, H, W, 3)
    centres = torch.zeros(B, P, 2, device="cuda")
    for shift in (16, 1, n - 1):                                           # partly overlapping buffers
        with pytest.raises(capf.CapfError, match=r"\(-1\)"):
            capf.erase_patches(images, centres, out=buf[shift:shift + n].view(B, H, W, 3))
    with pytest.raises(capf.CapfError, match=r"\(-2\)"):                   # P = 33
        capf.erase_patches(images, torch.zeros(B, 33, 2, device="cuda"))
    assert not buf.any()
    for bad in (dict(images_u8=images.float()), dict(images_u8=images.transpose(1, 2)), dict(centers=centres.double()),
                dict(centers=torch.zeros(B, 2, P, device="cuda").transpose(1, 2)), dict(centers=centres[:1]), dict(centers=centres.cpu()),
                dict(mask=torch.ones(B, P, device="cuda")), dict(mask=torch.ones(B, P + 1, dtype=torch.uint8, device="cuda")),
                dict(mask=torch.ones(P, B, dtype=torch.uint8, device="cuda").t()), dict(out=torch.empty(B, H, W, 3, device="cuda")),
                dict(out=torch.empty(B, H, W + 1, 3, dtype=torch.uint8, device="cuda")), dict(size=-1)):
        args = dict(images_u8=images, centers=centres)
        args.update(bad)
        with pytest.raises(ValueError):
            capf.erase_patches(**args)


def test_sums_beyond_32_bits_are_exact():
    """one patch over a whole 4200 x 4200 image of mostly 255: a channel sum of 4.49e9 > 2^32"""
    H = W = 4200
    images = torch.full((1, H, W, 3), 255, dtype=torch.uint8, device="cuda")
    images[0, ::7, ::5, 1] = 3
    images[0, 5::11, :, 2] = 254
    sums = images.view(-1, 3).sum(dim=0, dtype=torch.int64)
    assert int(sums.max()) > 1 << 32
    mean = (sums // (H * W)).to(torch.uint8)
    assert mean.tolist() != [255, 255, 255]
    got = capf.erase_patches(images, torch.tensor([[[2100.5, 2099.5]]], device="cuda"), None, 2 * H, True)
    assert bool((got.view(-1, 3) == mean).all())


def test_erase_image_on_the_device():
    from mvn.utils.img import erase_image, erase_image_batch
    rng = np.random.RandomState(9)
    image = rng.randint(0, 256, (12, 10, 3)).astype(np.uint8)
    centres = [(4.999999999999, 6.999999999999), (-0.999999999999, 3.0), (9.999999999999, 11.999999999999), (10.0, 3.0), (-1.0, 3.0)]
    for size, use_mean in ((2, True), (3, False), (70, True)):
        want = erase_oracle.erase_image(image, centres, size, use_mean)
        got = erase_image(image, centres, size, use_mean)
        assert isinstance(got, np.ndarray) and (got == want).all()
        dev = erase_image(torch.from_numpy(image).cuda(), centres, size, use_mean)
        assert dev.is_cuda and torch.equal(dev.cpu(), torch.from_numpy(want))
    batch = torch.from_numpy(image).cuda()[None]
    cen = torch.tensor([[[4.0, 6.0], [0.0, 3.0]]], device="cuda")
    assert torch.equal(erase_image_batch(batch, cen)[0].cpu(), torch.from_numpy(erase_oracle.erase_image(image, [(4, 6), (0, 3)])))
