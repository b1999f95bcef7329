"""N3, crop-aware decode, host side (no GPU): capf_jpeg_crop_rect -- which pixels and MCUs of a file an affine crop can read -- against a brute
force over every output pixel of the warp's documented coordinate rule, and capf_jpeg_crop_batch_info's sizes and refusals."""
import ctypes

import numpy as np
import pytest

import crop_oracle
import jpeg_crop_cases as cc

SIZES = [(8, 8), (17, 13), (64, 48), (1000, 1002)]                       # (W, H)
INVALID = -1                                                               # include/capf.h :: CAPF_ERR_INVALID


def _out_size(W, H):
    return (192, 256) if W >= 1000 else (24, 32)                           # (out_w, out_h)


def _expected_mcu(rect, W, H, hs, vs):
    """the MCUs holding rect grown by one pixel along each subsampled axis (the neighbouring chroma sample fancy upsampling reads),
    clamped to the image"""
    x0, y0, x1, y1 = rect
    x0, x1 = max(x0 - (hs == 2), 0), min(x1 + (hs == 2), W)
    y0, y1 = max(y0 - (vs == 2), 0), min(y1 + (vs == 2), H)
    return (x0 // (8 * hs), y0 // (8 * vs), -(-x1 // (8 * hs)), -(-y1 // (8 * vs)))


@pytest.mark.parametrize("sampling", list(cc.SAMPLING))
@pytest.mark.parametrize("W,H", SIZES)
def test_rectangle_holds_every_tap_and_not_a_pixel_more(W, H, sampling):
    from capf import lib as capf
    hs, vs = cc.SAMPLING[sampling]
    out_w, out_h = _out_size(W, H)
    mats = cc.matrices(W, H, out_w, out_h)
    assert len(mats) == 16
    n_inside = 0
    for name, m in mats.items():
        rect, mcu = capf.jpeg_crop_rect(W, H, hs, vs, m, (out_w, out_h))
        want = cc.tap_bounds(m, W, H, out_w, out_h)
        # coverage: every tap column / row inside the image lies in the rectangle; minimality: a side that is not clamped to the image
        # edge lies ON the outermost tap, so taking one pixel off it loses that tap (a clamped side may lie beyond the outermost tap
        # inside the image: a crop that shrinks the image steps over columns)
        assert want is not None, (name, "the case list holds no crop outside the image")
        edge = (0, 0, W, H)
        assert all(r == t if r != e else (r <= t if k < 2 else r >= t) for k, (r, t, e) in enumerate(zip(rect, want, edge))), (name, rect, want)
        sx, sy = cc.first_taps(m, out_w, out_h)
        for t, lo, hi, size in ((sx, rect[0], rect[2], W), (sx + 1, rect[0], rect[2], W), (sy, rect[1], rect[3], H), (sy + 1, rect[1], rect[3], H)):
            inside = (t >= 0) & (t < size)
            assert np.all((t[inside] >= lo) & (t[inside] < hi)), name
        # the MCU rectangle: whole MCUs, holds the pixel rectangle and the chroma margin, and is the smallest that does
        mw, mh = 8 * hs, 8 * vs
        assert mcu[0] * mw <= rect[0] and mcu[1] * mh <= rect[1] and mcu[2] * mw >= rect[2] and mcu[3] * mh >= rect[3], (name, rect, mcu)
        assert 0 <= mcu[0] < mcu[2] <= -(-W // mw) and 0 <= mcu[1] < mcu[3] <= -(-H // mh), (name, mcu)
        assert mcu == _expected_mcu(rect, W, H, hs, vs), (name, rect, mcu)
        n_inside += rect != (0, 0, W, H)
    assert W < 64 or n_inside >= 8                                         # (on the larger images most cases are true sub-rectangles)


def test_shrinking_an_unclamped_side_loses_a_tap():
    """the minimality claim spelled out on one case: a box inside a 1000 x 1002 frame, each side moved in by one pixel"""
    from capf import lib as capf
    W, H, out = 1000, 1002, (192, 256)
    m = cc.matrices(W, H, *out)["box_centre"]
    rect, _ = capf.jpeg_crop_rect(W, H, 2, 2, m, out)
    assert 0 < rect[0] < rect[2] < W and 0 < rect[1] < rect[3] < H
    sx, sy = cc.first_taps(m, *out)
    cols, rows = np.union1d(sx, sx + 1), np.union1d(sy, sy + 1)
    assert rect[0] in cols and rect[2] - 1 in cols and rect[1] in rows and rect[3] - 1 in rows


def test_crop_outside_the_image_and_crop_of_the_whole_image():
    from capf import lib as capf
    for (W, H) in SIZES:
        for hs, vs in cc.SAMPLING.values():
            out = (W, H)
            for shift in ((-(W + 2.0), 0.0), (0.0, H + 5.0), (3.0 * W, -2.0 * H)):        # dst = src + shift: the crop sees nothing of the image
                m = np.array([[1.0, 0.0, shift[0]], [0.0, 1.0, shift[1]]])
                assert cc.tap_bounds(m, W, H, *out) is None
                assert capf.jpeg_crop_rect(W, H, hs, vs, m, out) == ((0, 0, 0, 0), (0, 0, 0, 0))
            rect, mcu = capf.jpeg_crop_rect(W, H, hs, vs, np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]), out)
            assert rect == (0, 0, W, H) and mcu == (0, 0, -(-W // (8 * hs)), -(-H // (8 * vs)))


def test_crop_rect_refuses_bad_arguments():
    from capf import lib as capf
    from capf.lib import CapfError
    eye = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    for args in ((0, 8, 1, 1, eye, (4, 4)), (8, -1, 1, 1, eye, (4, 4)), (8, 8, 1, 2, eye, (4, 4)), (8, 8, 4, 1, eye, (4, 4)),
                 (8, 8, 1, 1, eye, (0, 4)), (8, 8, 1, 1, eye, (4, -3))):
        with pytest.raises(CapfError):
            capf.jpeg_crop_rect(*args)


@pytest.fixture(scope="module")
def frame420():
    return cc.encode(cc.make_image(1000, 1002, 3), 75, 2)


def test_scratch_shrinks_with_the_rectangle(frame420):
    """a crop reading at most a quarter of the frame needs less scratch than the full decode of the same file; a crop of the whole frame
    needs the full decode's plus the BGR patch, to within 1 % (AC storage is proportional to the blocks kept; on top come one DC
    difference per block -- 2 of a block's 128 coefficient bytes -- and the descriptor's few more fields)"""
    from capf import lib as capf
    W, H, out = 1000, 1002, (192, 256)
    _, full = capf.jpeg_batch_info([frame420])
    m = crop_oracle.get_affine_transform((500.0, 500.0), (2.1, 2.8), out)     # a 420 x 560 box: just under a quarter of the frame
    rc, rows, crop = capf.jpeg_crop_batch_info([frame420], [m], out)
    x0, y0, x1, y1 = rows[0]["pixel_rect"]
    assert rc == 0 and 0 < (x1 - x0) * (y1 - y0) <= W * H / 4 and (x1 - x0) * (y1 - y0) > W * H / 8
    assert crop < full, (crop, full)
    assert rows[0]["coef_elems"] < capf.jpeg_batch_info([frame420])[0][0]["coef_elems"] / 3
    rc, rows, whole = capf.jpeg_crop_batch_info([frame420], [np.array([[1.0, 0, 0], [0, 1.0, 0]])], (W, H))
    assert rc == 0 and rows[0]["pixel_rect"] == (0, 0, W, H) and rows[0]["mcu_rect"] == (0, 0, 63, 63)
    patch = W * H * 3
    assert full + patch <= whole <= 1.01 * (full + patch), (whole, full, patch)
    # both files of a batch count
    rc, _, two = capf.jpeg_crop_batch_info([frame420, frame420], [m, m], out)
    assert rc == 0 and crop < two < 2 * full


def test_unsupported_files_and_bad_arguments_are_refused(frame420):
    import io
    from PIL import Image
    from capf import lib as capf
    from capf.lib import CapfError
    lib = capf.load_library()
    buf = io.BytesIO()
    Image.fromarray(cc.make_image(32, 32, 1)).save(buf, "JPEG", quality=80, progressive=True)
    prog = buf.getvalue()
    want = lib.capf_jpeg_info(prog, len(prog), None, None, None, None, None, None)
    assert want != 0
    eye = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    rc, rows, scratch = capf.jpeg_crop_batch_info([frame420, prog, frame420], [eye] * 3, (192, 256))
    assert rc == want and scratch is None and [r["status"] for r in rows] == [0, want, 0]
    with pytest.raises(CapfError, match=r"files \[1\]"):
        capf.jpeg_decode_crop_batch([frame420, prog, frame420], [eye] * 3, (192, 256), device="cpu")     # refused before any GPU work
    # bad n, out_w, out_h
    datas, ptrs, sizes = capf._byte_arrays([frame420])
    m = np.ascontiguousarray(eye.reshape(1, 6))
    for n, out_w, out_h in ((0, 192, 256), (-1, 192, 256), (1, 0, 256), (1, 192, 0), (1, -192, 256), (1, 192, -1)):
        rc, _, _ = capf._crop_batch_info(lib, n, ptrs, sizes, m, out_w, out_h, 0)
        assert rc == INVALID, (n, out_w, out_h, rc)
    mp = m.ctypes.data_as(ctypes.c_void_p)
    for n, out_h, out_w in ((0, 256, 192), (-1, 256, 192), (1, 0, 192), (1, 256, 0)):                    # (checked before any pointer is used)
        assert lib.capf_jpeg_decode_crop_batch(None, n, ptrs, sizes, mp, out_h, out_w, 4096, 4096, 1 << 30, 4096, 0) == INVALID
    assert lib.capf_jpeg_decode_crop_batch(None, 1, ptrs, sizes, mp, 256, 192, 4096, 4096, 1 << 30, 4096, -5) == INVALID
