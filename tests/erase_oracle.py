"""The integer restatement of erase_image (ContextPose/mvn/utils/img.py:179-198) that the native entry capf_erase_patches is held to.

numpy only, no float arithmetic on pixels: a patch's value is the integer sum // count per channel -- what the reference's float64
`.mean()` becomes when numpy stores it into the uint8 image (tests/test_erase_api.py holds this file to the reference's own outputs,
tests/golden/erase_reference.npz, with ==).  A centre counts iff x > -1 and x < W and y > -1 and y < H on the given numbers, which is the
reference's int() truncation toward zero followed by its range test; it is False for NaN and +-Inf, which the reference's int() raises on
and the native entry skips (the one divergence)."""
import numpy as np


def counts(x, y, H, W):
    return bool(x > -1 and x < W and y > -1 and y < H)


def erase_image(image, center_list, size=70, use_mean=True):
    """image: uint8 [H, W, C]; center_list: (x, y) pairs, any real numbers -> a new uint8 [H, W, C]"""
    image = np.asarray(image)
    assert image.dtype == np.uint8 and image.ndim == 3
    H, W = image.shape[:2]
    out = image.copy()
    half = int(size) // 2
    for x, y in center_list:
        if not counts(x, y, H, W):
            continue
        xc, yc = int(x), int(y)
        left, right = max(0, xc - half), min(W, xc + half + 1)
        upper, lower = max(0, yc - half), min(H, yc + half + 1)
        if use_mean:
            patch = image[upper:lower, left:right].astype(np.int64)
            out[upper:lower, left:right] = (patch.sum(axis=(0, 1)) // (patch.shape[0] * patch.shape[1])).astype(np.uint8)
        else:
            out[upper:lower, left:right] = 0
    return out


def erase_batch(images, centers, mask=None, size=70, use_mean=True):
    """images: uint8 [B, H, W, 3]; centers: float32 [B, P, 2]; mask: [B, P] (non-zero selects) or None -> uint8 [B, H, W, 3]"""
    images, centers = np.asarray(images), np.asarray(centers, dtype=np.float32)
    out = np.empty_like(images)
    for b in range(images.shape[0]):
        chosen = [(float(x), float(y)) for p, (x, y) in enumerate(centers[b]) if mask is None or mask[b][p] != 0]
        out[b] = erase_image(images[b], chosen, size, use_mean)
    return out
