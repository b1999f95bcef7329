"""CPU: erase_image for crop batches (capf_erase_patches) without a device -- the integer restatement against the reference's own outputs,
the symbols, every refusal the entry makes before a launch, and the host function's int() rule.

The GPU half is tests/test_gpu_erase.py (the kernel against the restatement) and tests/test_gpu_erase_prefetch.py (the prefetcher)."""
import ctypes

import numpy as np
import pytest

import erase_oracle
from conftest import load_golden

OK, INVALID, UNSUPPORTED = 0, -1, -2          # include/capf.h :: CAPF_OK, CAPF_ERR_INVALID, CAPF_ERR_UNSUPPORTED


def golden_cases():
    """[(name, image, centres float64 [n, 2], size, use_mean, the reference's output)] of tests/golden/erase_reference.npz"""
    g = load_golden("erase_reference")
    return [(str(n), g[f"image_{i}"], g[f"centers_{i}"], int(g[f"size_{i}"]), bool(g[f"use_mean_{i}"]), g[f"out_{i}"]) for i, n in enumerate(g["names"])]


def test_golden_holds_the_cases_the_rule_needs():
    cases = golden_cases()
    assert 18 <= len(cases) <= 30
    assert {0, 1, 2, 3, 7} <= {c[3] for c in cases} and any(c[3] > max(c[1].shape[:2]) for c in cases)
    assert {c[4] for c in cases} == {True, False}
    assert all(c[1].shape[0] <= 24 and c[1].shape[1] <= 24 and c[1].shape[0] * c[1].shape[1] <= 24 * 20 for c in cases)
    every = np.concatenate([np.concatenate([c[2], np.full((len(c[2]), 1), c[1].shape[1]), np.full((len(c[2]), 1), c[1].shape[0])], axis=1) for c in cases])
    x, y, W, H = every.T
    for want in (x == -0.5, x == -1.0, x == W - 0.25, x == W, y == -0.5, y == -1.0, y == H - 0.25, y == H, x == 1e30):
        assert want.any()
    assert any(len(c[2]) != len({tuple(p) for p in c[2].tolist()}) for c in cases)           # coincident centres
    assert sum(not np.array_equal(c[1], c[5]) for c in cases) >= 12                            # most cases change pixels


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c[0])
def test_restatement_equals_the_reference(case):
    name, image, centres, size, use_mean, want = case
    keep = image.copy()
    got = erase_oracle.erase_image(image, centres, size, use_mean)
    assert got.dtype == np.uint8 and (got == want).all()
    assert (image == keep).all()
    # the batched form on the fp32 centres the native entry takes (every golden centre is an fp32 number or rounds to one on the same side)
    got_b = erase_oracle.erase_batch(image[None], centres.astype(np.float32)[None], None, size, use_mean) if len(centres) else image[None]
    assert (got_b[0] == want).all()


def test_restatement_skips_what_the_mask_and_the_range_rule_exclude():
    rng = np.random.RandomState(3)
    img = rng.randint(0, 256, (2, 6, 5, 3)).astype(np.uint8)
    centres = np.array([[[2, 2], [np.nan, 1], [np.inf, 1], [1, -np.inf], [1e30, 2], [4.75, 5.75]]] * 2, np.float32)
    none = erase_oracle.erase_batch(img, centres, np.zeros((2, 6), np.uint8), 3, False)
    assert (none == img).all()
    some = erase_oracle.erase_batch(img, centres, np.array([[0, 1, 1, 1, 1, 1], [1, 1, 1, 1, 1, 0]], np.uint8), 3, False)
    assert (some[0][4:, 3:] == 0).all() and (some[0][:4] == img[0][:4]).all()
    assert (some[1][1:4, 1:4] == 0).all() and (some[1][4:] == img[1][4:]).all()


def test_symbols_are_exported_and_declared():
    import capf
    from capf.lib import ERASE_MAX_PATCHES, EXPORTS, PROTOTYPES
    lib = capf.load_library()
    for sym in ("capf_erase_scratch_bytes", "capf_erase_patches"):
        assert sym in EXPORTS and hasattr(lib, sym)
    assert PROTOTYPES["capf_erase_scratch_bytes"][0] is ctypes.c_size_t and len(PROTOTYPES["capf_erase_patches"][1]) == 13
    assert ERASE_MAX_PATCHES == 32
    assert lib.capf_erase_scratch_bytes(1, 1) == 32 and lib.capf_erase_scratch_bytes(512, 17) == 512 * 17 * 32
    assert lib.capf_erase_scratch_bytes(3, 32) == 3 * 32 * 32
    for bad in ((0, 1), (1, 0), (-1, 4), (1, 33)):
        assert lib.capf_erase_scratch_bytes(*bad) == 0


def test_every_refusal_comes_before_a_launch():
    """a NULL stream and addresses that are never read: each call returns its code from the host-side judgement"""
    import capf
    lib = capf.load_library()
    IMG, OUT, CEN, MSK, SCR = 1 << 20, 1 << 24, 1 << 28, 1 << 29, 1 << 30            # far apart, 16-byte aligned

    def call(images=IMG, batch=2, height=8, width=6, centers=CEN, mask=MSK, patches=17, size=70, use_mean=1, out=OUT, scratch=SCR, scratch_bytes=None):
        if scratch_bytes is None:
            scratch_bytes = lib.capf_erase_scratch_bytes(batch, patches) or 1 << 20
        return lib.capf_erase_patches(None, images, batch, height, width, centers, mask, patches, size, use_mean, out, scratch, scratch_bytes)

    for null in ("images", "centers", "out", "scratch"):
        assert call(**{null: None}) == INVALID, null
    for name in ("batch", "height", "width", "patches"):
        for v in (0, -3):
            assert call(**{name: v}) == INVALID, (name, v)
    assert call(size=-1) == INVALID
    assert call(patches=33) == UNSUPPORTED and call(patches=1 << 20) == UNSUPPORTED
    assert call(height=1 << 15, width=1 << 15) == UNSUPPORTED                          # a frame of 3 * 2^30 bytes
    assert call(batch=1 << 30, height=16, width=32, patches=1, scratch_bytes=1 << 40) == UNSUPPORTED       # the paint grid: 2^31 blocks
    need = lib.capf_erase_scratch_bytes(2, 17)
    assert call(scratch_bytes=need - 1) == INVALID and call(scratch_bytes=0) == INVALID
    assert call(scratch=SCR + 8) == INVALID                                            # misaligned scratch
    n = 2 * 8 * 6 * 3
    for shift in (1, 16, n - 1):                                                       # partly overlapping buffers, either way round
        assert call(out=IMG + shift) == INVALID and call(images=OUT + shift, out=OUT) == INVALID
    assert call(scratch=IMG + 32) == INVALID and call(scratch=OUT - 16) == INVALID     # scratch inside images / running into out
    assert call(images=SCR + need - 16) == INVALID


def _fake_device(monkeypatch):
    """erase_image's device half replaced by the restatement on CPU tensors; returns the list of calls the binding received"""
    import torch
    from capf import lib as capf_lib
    calls = []

    def erase_patches(images_u8, centers, mask=None, size=70, use_mean=True, out=None):
        assert images_u8.dtype == torch.uint8 and centers.dtype == torch.float32 and mask is None and out is None
        calls.append((centers.clone(), size, use_mean))
        return torch.from_numpy(erase_oracle.erase_batch(images_u8.numpy(), centers.numpy(), None, size, use_mean))

    monkeypatch.setattr(capf_lib, "erase_patches", erase_patches)
    monkeypatch.setattr(torch.Tensor, "cuda", lambda self, *a, **k: self)
    return calls


def test_erase_image_truncates_float64_centres_as_python_does(monkeypatch):
    """4.999999999999 is 5.0 in fp32 and 4 under int(): the host function converts before the device sees the centre"""
    from mvn.utils.img import erase_image
    calls = _fake_device(monkeypatch)
    rng = np.random.RandomState(5)
    image = rng.randint(0, 256, (12, 10, 3)).astype(np.uint8)
    centres = [(4.999999999999, 6.999999999999), (np.float64(-0.999999999999), 3.0), (9.999999999999, 11.999999999999), (10.0, 3.0), (-1.0, 3.0), (3, 1e300)]
    assert np.float32(4.999999999999) == 5.0 and int(4.999999999999) == 4
    for size, use_mean in ((1, False), (2, True), (3, True)):
        keep = image.copy()
        got = erase_image(image, centres, size, use_mean)
        assert isinstance(got, np.ndarray) and got.dtype == np.uint8 and got is not image and (image == keep).all()
        want = erase_oracle.erase_image(image, centres, size, use_mean)
        assert (got == want).all() and not (got == image).all()
        sent, s, m = calls[-1]
        assert sent.tolist() == [[[4.0, 6.0], [0.0, 3.0], [9.0, 11.0]]] and s == size and m == use_mean
    # the reference's defaults, and the reference's errors: int() of a non-finite centre raises
    assert (erase_image(image, [(5, 6)]) == erase_oracle.erase_image(image, [(5, 6)], 70, True)).all() and calls[-1][1:] == (70, True)
    for bad in (float("nan"), float("inf")):
        with pytest.raises((ValueError, OverflowError)):
            erase_image(image, [(bad, 1.0)])
    n = len(calls)
    assert (erase_image(image, []) == image).all() and (erase_image(image, [(-3, 2), (2, 12)]) == image).all() and len(calls) == n
    with pytest.raises(ValueError, match="at most 32"):
        erase_image(image, [(1, 1)] * 33)


def test_erase_image_returns_the_kind_it_was_given(monkeypatch):
    import torch
    from mvn.utils.img import erase_image
    _fake_device(monkeypatch)
    image = torch.arange(5 * 4 * 3, dtype=torch.uint8).view(5, 4, 3)
    got = erase_image(image, [(1.5, 2.5)], 3, True)
    assert torch.is_tensor(got) and got.dtype == torch.uint8 and got.data_ptr() != image.data_ptr()
    assert (got.numpy() == erase_oracle.erase_image(image.numpy(), [(1, 2)], 3, True)).all()


def test_binding_refuses_wrong_inputs_before_the_library_is_called():
    import torch
    from capf import lib as capf_lib
    img, cen = torch.zeros(2, 4, 4, 3, dtype=torch.uint8), torch.zeros(2, 3, 2)
    with pytest.raises(ValueError, match="CUDA"):
        capf_lib.erase_patches(img, cen)


def test_prefetcher_erase_options():
    from mvn.datasets.utils import data_prefetcher
    opt = data_prefetcher._erase_options
    assert opt(None) is None and opt(False) is None
    assert opt(True) == {"size": 70, "use_mean": True, "prob": 0.5, "joints": None, "generator": None}
    assert opt({"size": 31, "joints": (16, 3, 3)}) == {"size": 31, "use_mean": True, "prob": 0.5, "joints": [3, 16], "generator": None}
    for bad in ({"sise": 3}, {"joints": [17]}, {"joints": [-1]}, {"prob": 1.5}, {"size": -2}):
        with pytest.raises(ValueError):
            opt(bad)
