"""Generate tests/golden/erase_reference.npz: the REAL reference's erase_image on small synthetic images.

Run where the reference exists only (it is read through oracle/_refshim.py, as tools/make_pck2d_golden.py does; never on a GPU box):
    PYTHONDONTWRITEBYTECODE=1 python tools/make_erase_golden.py            # write the fixture
    PYTHONDONTWRITEBYTECODE=1 python tools/make_erase_golden.py --check    # recompute and compare with the committed one

ContextPose/mvn/utils/img.py:179-198: `erase_image(image, center_list, size=70, use_mean=True)`.  The module's file is executed on its own
with `cv2`, `tqdm` and `PIL` stubbed in sys.modules (imported at its top, never called on this path).

The cases (data only: per case the image, the centres as float64 [n, 2], size, use_mean and the reference's output) walk every rule the
native entry restates: centres at -0.5 (truncates to 0: counts), -1.0 (does not), W - 0.25 / H - 0.25 (count), W / H (do not), 1e30; sizes
0, 1, 2, 3, 7 and one larger than the image; both use_mean values; overlapping and coincident centres (the later one wins, and its mean is
the ORIGINAL image's); patches clipped at every border; a 1 x 1 image; an empty centre list.  Images are at most 24 x 20."""
import os
import sys
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in ("oracle", "contextaware-poseformer_amd", "tests"):
    sys.path.insert(0, os.path.join(ROOT, p))
sys.dont_write_bytecode = True

import numpy as np

OUT = os.path.join(ROOT, "tests", "golden", "erase_reference.npz")


def reference_erase_image():
    import importlib.util
    import _refshim

    class _Stub(types.ModuleType):
        def __getattr__(self, name):
            if name.startswith("__"):
                raise AttributeError(name)
            return 0

    added = [m for m in ("cv2", "tqdm", "PIL") if m not in sys.modules]
    for m in added:
        sys.modules[m] = _Stub(m)
    try:
        path = _refshim.REFERENCE_ROOT + "/mvn/utils/img.py"
        spec = importlib.util.spec_from_file_location("reference_img", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        assert mod.__file__.startswith(_refshim.REFERENCE_ROOT + "/")
    finally:
        for m in added:
            del sys.modules[m]
    return mod.erase_image


def cases():
    """[(name, image uint8 [H, W, 3], centres float64 [n, 2], size, use_mean)]"""
    rng = np.random.RandomState(37)
    img = lambda H, W: rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    c = lambda *pts: np.asarray(pts, np.float64).reshape(-1, 2)
    out = []
    H, W = 20, 24
    edge = c((-0.5, 3.0), (-1.0, 10.0), (W - 0.25, 7.5), (W, 12.0), (5.0, -0.5), (9.0, -1.0), (11.0, H - 0.25), (13.0, H), (-0.999, -0.999), (1e30, 4.0),
             (4.0, -1e30), (W - 1, H - 1))
    for size in (0, 1, 2, 3, 7):
        for use_mean in (True, False):
            out.append((f"edges_size{size}_{'mean' if use_mean else 'zero'}", img(H, W), edge, size, use_mean))
    out.append(("larger_than_image_mean", img(H, W), c((12.3, 9.9)), 61, True))
    out.append(("larger_than_image_zero", img(H, W), c((0.0, 0.0), (23.9, 19.9)), 70, False))
    # overlap: partly overlapping patches, then the same centre three times, then a patch inside an earlier one
    out.append(("overlap_mean", img(H, W), c((8.0, 8.0), (10.5, 9.5), (10.5, 9.5), (10.5, 9.5), (3.0, 15.0), (4.0, 16.0), (3.9, 15.2)), 7, True))
    out.append(("overlap_order_mean", img(24, 20), c((10.0, 12.0), (10.0, 12.0), (11.0, 13.0), (2.0, 2.0), (11.0, 13.0), (10.0, 12.0)), 9, True))
    out.append(("overlap_zero", img(24, 20), c((5.0, 5.0), (6.0, 6.0), (19.9, 23.9), (0.2, 0.7)), 6, False))
    out.append(("inside_earlier_mean", img(H, W), c((12.0, 10.0), (12.6, 10.4), (13.0, 9.0)), 15, True))
    out.append(("inside_earlier_small_mean", img(H, W), c((12.0, 10.0), (12.0, 10.0), (13.0, 9.0)), 3, True))
    out.append(("one_pixel_image_mean", img(1, 1), c((0.0, 0.0), (-0.5, 0.9), (1.0, 0.0)), 3, True))
    out.append(("one_pixel_image_zero", img(1, 1), c((0.99, -0.99)), 0, False))
    out.append(("no_centres", img(5, 7), c(), 7, True))
    out.append(("all_outside", img(5, 7), c((-1.0, 2.0), (7.0, 2.0), (3.0, 5.0), (3.0, -1.5)), 7, True))
    out.append(("odd_image_mean", img(5, 7), c((6.75, 4.75), (0.0, 0.0), (3.5, 2.5)), 2, True))
    # means that are no integers and a flat image whose mean is exact
    flat = np.full((9, 11, 3), 255, np.uint8)
    out.append(("flat_255_mean", flat, c((5.0, 4.0), (0.0, 8.0)), 5, True))
    return out


def compute():
    erase_image = reference_erase_image()
    rec = {"names": np.array([n for n, *_ in cases()])}
    for i, (name, image, centres, size, use_mean) in enumerate(cases()):
        keep = image.copy()
        got = erase_image(image, [(float(x), float(y)) for x, y in centres], size, use_mean)
        assert got.dtype == np.uint8 and got.shape == image.shape and np.array_equal(image, keep)
        rec[f"image_{i}"], rec[f"centers_{i}"], rec[f"out_{i}"] = image, centres, got
        rec[f"size_{i}"], rec[f"use_mean_{i}"] = np.int64(size), np.int64(1 if use_mean else 0)
    return rec


if __name__ == "__main__":
    got = compute()
    if "--check" in sys.argv:
        want = np.load(OUT)
        assert sorted(want.files) == sorted(got), "tests/golden/erase_reference.npz holds other cases"
        assert all(np.array_equal(want[k], got[k]) for k in got), "tests/golden/erase_reference.npz differs from what the reference computes now"
        print("ok:", OUT)
    else:
        np.savez_compressed(OUT, **got)
        print("wrote", OUT, os.path.getsize(OUT), "bytes,", len(got["names"]), "cases")
