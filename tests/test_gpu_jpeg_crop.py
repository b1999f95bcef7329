"""N3, crop-aware decode on the MI355X: capf_jpeg_decode_crop_batch (files -> affine crops, only the MCUs a crop reads are transformed) gives,
bit for bit, what capf_warp_affine gives on capf_jpeg_decode_batch's frames -- on the libjpeg goldens, at rectangle edge cases, on
frame-sized files, alone or in a batch, run after run, and next to corrupt files.  Equality is exact everywhere; nothing is excluded."""
import os

import numpy as np
import pytest

from conftest import ROOT

import jpeg_crop_cases as cc

pytestmark = pytest.mark.gpu

CASES = ["rgb444_q90", "rgb420_q75_odd", "rgb422_q50", "rgb420_q95_opt", "rgb420_q85_rst", "rgb444_q30", "grey_q80", "rgb420_q100_sat"]
EYE = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"), allow_pickle=False)


def _crop(datas, mats, out, subseq=0):
    import torch
    from capf import lib as capf
    crops, status = capf.jpeg_decode_crop_batch(datas, mats, out, "cuda", subseq)
    torch.cuda.synchronize()
    return crops.cpu().numpy(), status.cpu().numpy()


def _two_step(datas, mats, out, subseq=0):
    """the route the crop-aware one must equal: full decode of every file, then the warp"""
    import torch
    from capf import lib as capf
    frames, status = capf.jpeg_decode_batch(datas, "cuda", subseq)
    crops = capf.warp_affine(frames, np.stack(mats), out)
    torch.cuda.synchronize()
    return crops.cpu().numpy(), status.cpu().numpy()


def _shift(dx, dy):
    """crop pixel (x, y) = image pixel (x + dx, y + dy)"""
    return np.array([[1.0, 0.0, -float(dx)], [0.0, 1.0, -float(dy)]])


def test_goldens_each_with_its_own_matrix():
    """all eight libjpeg goldens in ONE call (odd sizes, 4:2:2, grey, optimised tables, a restart interval, saturated blocks), file i with
    matrix i of the CPU test's list (and the other half of the list in a second call), at the default subsequence length and at 4 bytes"""
    import torch
    from capf import lib as capf
    g = _golden()
    datas = [g[n + ":jpeg"].tobytes() for n in CASES]
    out = (24, 32)
    for half in (0, 1):
        mats = []
        for i, n in enumerate(CASES):
            W, H = g[n + ":info"].tolist()[:2]
            ms = cc.matrices(W, H, *out)
            mats.append(ms[list(ms)[half * 8 + i]])
        uploaded = capf.warp_affine([torch.from_numpy(np.ascontiguousarray(g[n + ":bgr"])).cuda() for n in CASES], np.stack(mats), out).cpu().numpy()
        for subseq in (0, 4):
            got, status = _crop(datas, mats, out, subseq)
            want, _ = _two_step(datas, mats, out, subseq)
            assert not status.any(), status
            for i, n in enumerate(CASES):
                assert np.array_equal(got[i], want[i]), (n, half, subseq)
                assert np.array_equal(got[i], uploaded[i]), (n, half, subseq)
        assert uploaded.any()


@pytest.mark.parametrize("W,H", [(48, 40), (33, 17)])
def test_rectangle_edge_cases(W, H):
    """4:2:0 files encoded on the spot, without and with a restart interval of one MCU row; the crop's rectangle is exactly one MCU, one MCU
    wide and full height, touches each image edge, spans restart boundaries, is empty, is the whole image"""
    from capf import lib as capf
    img = cc.make_image(W, H, W)
    files = [cc.encode(img, 85, 2), cc.encode(img, 85, 2, restart_marker_rows=1)]
    cases = {                                             # name -> (matrix, (out_w, out_h), expected MCU rectangle or None)
        # taps 18..28 (+ the chroma margin 17..29) inside MCU column 1; rows likewise in MCU row 1, or rows 2..12 (1..13) in row 0
        "one_mcu": (_shift(18, 18 if H > 32 else 2), (10, 10), (1, 1, 2, 2) if H > 32 else (1, 0, 2, 1)),
        "mcu_column": (_shift(18, 0), (10, H), (1, 0, 2, -(-H // 16))),
        "left": (_shift(-5, 3), (12, 9), None), "right": (_shift(W - 7, 2), (12, 9), None),
        "top": (_shift(4, -6), (9, 12), None), "bottom": (_shift(3, H - 6), (9, 12), None),
        "across_restarts": (_shift(2, 9), (8, 20) if H > 32 else (8, 8), None),      # rows 9.. : two (three) MCU rows = restart intervals
        "empty": (_shift(W + 3, 0), (12, 9), (0, 0, 0, 0)),
        "whole": (EYE, (W, H), (0, 0, -(-W // 16), -(-H // 16))),
        "rot30": (cc.matrices(W, H, 24, 32)["rot30"], (24, 32), None),
        "down2": (cc.matrices(W, H, 24, 32)["down2"], (24, 32), None),
    }
    for name, (m, out, mcu) in cases.items():
        rect, got_mcu = capf.jpeg_crop_rect(W, H, 2, 2, m, out)
        if mcu is not None:
            assert got_mcu == mcu, (name, got_mcu)
        if name in ("left", "top"):
            assert rect[0 if name == "left" else 1] == 0
        if name in ("right", "bottom"):
            assert rect[2 if name == "right" else 3] == (W if name == "right" else H)
        if name == "across_restarts":
            assert got_mcu[3] - got_mcu[1] >= 2
        for subseq in (0, 4):
            got, status = _crop(files, [m, m], out, subseq)
            want, _ = _two_step(files, [m, m], out, subseq)
            assert not status.any(), (name, status)
            assert np.array_equal(got, want), (name, subseq)
            assert (not got.any()) if name == "empty" else got.any(), name


@pytest.fixture(scope="module")
def frames():
    """four 1000 x 1002 frames (quality 75 / 90, 4:2:0 / 4:4:4) with Human3.6M-like boxes, one hanging off the frame"""
    W, H = 1000, 1002
    files = [cc.encode(cc.make_image(W, H, 31 + i), (75, 90)[i % 2], (2, 0)[i // 2]) for i in range(4)]
    centers = [(500.0, 480.0), (430.0, 520.0), (610.0, 300.0), (60.0, 950.0)]
    scales = [(1.6, 2.13), (1.2, 1.6), (2.4, 3.2), (1.9, 2.5333)]
    return files, centers, scales


def test_frame_sized_files_match_both_existing_routes(frames):
    from mvn.utils.img import load_and_crop_batch
    files, centers, scales = frames
    got = load_and_crop_batch(files, centers, scales, (192, 256), decoder="device_crop").cpu().numpy()
    dev = load_and_crop_batch(files, centers, scales, (192, 256), decoder="device").cpu().numpy()
    host = load_and_crop_batch(files, centers, scales, (192, 256), decoder="host").cpu().numpy()
    assert got.shape == (4, 256, 192, 3) and got.any()
    assert np.array_equal(got, dev) and np.array_equal(got, host)
    assert not got[3, -1].any() and got[3, 0].any()                          # (the fourth box hangs over the bottom-left corner)


def test_composition_and_determinism(frames):
    from mvn.utils.img import get_affine_transform
    files, centers, scales = frames
    g = _golden()
    datas = list(files) + [g[n + ":jpeg"].tobytes() for n in CASES[:3]]
    out = (192, 256)
    mats = [get_affine_transform(c, s, 0, out) for c, s in zip(centers, scales)]
    mats += [cc.matrices(*g[n + ":info"].tolist()[:2], *out)["up3"] for n in CASES[:3]]
    batch, status = _crop(datas, mats, out)
    again, status2 = _crop(datas, mats, out)
    assert not status.any() and not status2.any()
    assert np.array_equal(batch, again)
    for i in range(len(datas)):
        alone, st = _crop([datas[i]], [mats[i]], out)
        assert st[0] == 0 and np.array_equal(alone[0], batch[i]), i


def test_a_corrupt_file_is_flagged_and_named_and_its_neighbours_stay_exact(frames):
    from capf.lib import CapfError
    from mvn.utils.img import get_affine_transform, load_and_crop_batch
    files, centers, scales = frames
    bad = files[1][:len(files[1]) // 2] + b"\xff\xd9"                        # the entropy data ends half way: too few blocks
    datas = [files[0], bad, files[2]]
    out = (192, 256)
    mats = [get_affine_transform(c, s, 0, out) for c, s in zip(centers[:3], scales[:3])]
    got, status = _crop(datas, mats, out)
    want, _ = _two_step([files[0], files[2]], [mats[0], mats[2]], out)
    assert status[0] == 0 and status[2] == 0 and status[1] != 0, status
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[1])
    with pytest.raises(CapfError, match=r"#1"):
        load_and_crop_batch(datas, centers[:3], scales[:3], out, decoder="device_crop")
