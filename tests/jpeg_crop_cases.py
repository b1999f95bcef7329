"""Shared by tests/test_jpeg_crop.py (CPU) and tests/test_gpu_jpeg_crop.py: the forward matrices the crop-aware JPEG route is tried with,
and the taps the affine warp reads, restated in numpy from the documented rule (oracle/crop_oracle.py's docstring): inverse map in double,
coordinates rounded to 1/1024, taps at the integer part and the integer part + 1."""
import numpy as np

import crop_oracle

SAMPLING = {"444": (1, 1), "422": (2, 1), "420": (2, 2), "grey": (1, 1)}


def matrices(W, H, out_w, out_h):
    """name -> forward 2x3 matrix (source pixels -> crop pixels) for a W x H image and an out_w x out_h crop"""
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    rot = np.array([[c, -s, 0.0], [s, c, 0.0]])
    rot[:, 2] = np.array([(out_w - 1) / 2, (out_h - 1) / 2]) - rot[:, :2] @ np.array([(W - 1) / 2, (H - 1) / 2])   # about the centres
    box = (0.6 * W / 200.0, 0.6 * W / 200.0 * out_h / out_w)              # get_affine_transform's scale: a box 0.6 W wide
    m = {
        "identity": np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]),
        "shift_int": np.array([[1.0, 0.0, -3.0], [0.0, 1.0, -2.0]]),
        "shift_half": np.array([[1.0, 0.0, -0.5], [0.0, 1.0, 0.5]]),
        "down2": np.array([[0.5, 0.0, 0.0], [0.0, 0.5, 0.0]]),
        "up3": np.array([[3.0, 0.0, -1.0], [0.0, 3.0, -2.0]]),
        "rot30": rot,
        "shear": np.array([[1.0, 0.25, 0.0], [0.1, 1.0, 0.0]]),
        "box_centre": crop_oracle.get_affine_transform((W / 2.0, H / 2.0), box, (out_w, out_h)),
    }
    for name, centre in (("left", (0.0, H / 2.0)), ("right", (float(W), H / 2.0)), ("top", (W / 2.0, 0.0)), ("bottom", (W / 2.0, float(H))),
                         ("top_left", (0.0, 0.0)), ("top_right", (float(W), 0.0)), ("bottom_left", (0.0, float(H))),
                         ("bottom_right", (float(W), float(H)))):
        m["box_" + name] = crop_oracle.get_affine_transform(centre, box, (out_w, out_h))
    return m


def first_taps(m, out_w, out_h):
    """(sx, sy): int64 [out_h, out_w], the first tap of every output pixel; the warp reads columns sx, sx + 1 and rows sy, sy + 1"""
    m = np.asarray(m, np.float64).reshape(2, 3)
    d = m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]
    d = 1.0 / d if d != 0 else 0.0
    a00, a11, a01, a10 = m[1, 1] * d, m[0, 0] * d, m[0, 1] * -d, m[1, 0] * -d
    b0 = -a00 * m[0, 2] - a01 * m[1, 2]
    b1 = -a10 * m[0, 2] - a11 * m[1, 2]
    xs, ys = np.arange(out_w, dtype=np.float64), np.arange(out_h, dtype=np.float64)
    adelta, bdelta = np.rint(a00 * xs * 1024.0).astype(np.int64), np.rint(a10 * xs * 1024.0).astype(np.int64)
    x0 = np.rint((a01 * ys + b0) * 1024.0).astype(np.int64) + 16
    y0 = np.rint((a11 * ys + b1) * 1024.0).astype(np.int64) + 16
    X, Y = (x0[:, None] + adelta[None, :]) >> 5, (y0[:, None] + bdelta[None, :]) >> 5
    return np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)


def tap_bounds(m, W, H, out_w, out_h):
    """brute force over all output pixels: (x0, y0, x1, y1), the bounding box of the tap columns inside [0, W) and the tap rows inside
    [0, H) (end exclusive), or None when an axis has no tap inside the image -- every read then hits the border"""
    sx, sy = first_taps(m, out_w, out_h)
    cols = np.unique(np.concatenate([sx.ravel(), sx.ravel() + 1]))
    rows = np.unique(np.concatenate([sy.ravel(), sy.ravel() + 1]))
    cols, rows = cols[(cols >= 0) & (cols < W)], rows[(rows >= 0) & (rows < H)]
    if not len(cols) or not len(rows):
        return None
    return int(cols.min()), int(rows.min()), int(cols.max()) + 1, int(rows.max()) + 1


def make_image(W, H, seed):
    """smooth colour + noise, uint8 RGB [H, W, 3]"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    return np.clip(np.stack([128 + 100 * np.sin(x / 7.0 + seed) * np.cos(y / 11.0), 128 + 90 * np.cos(x / 5.0 + y / 9.0), (5 * x + 3 * y + 7 * seed) % 256], -1)
                   + rng.normal(0, 8, (H, W, 3)), 0, 255).astype(np.uint8)


def encode(img, quality, subsampling, **kw):
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=subsampling, **kw)
    return buf.getvalue()
