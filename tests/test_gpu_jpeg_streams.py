"""N3 on the MI355X, on the streams of tests/golden/jpeg_streams.npz (oracle/make_jpeg_stream_goldens.py; the CPU half is
tests/test_jpeg_streams.py): images of a few pixels, Huffman codes of every length written from known coefficients, legal marker layouts.
All three routes -- capf_jpeg_decode_batch (device Huffman walk), capf_jpeg_decode (host walk) and capf_jpeg_decode_crop_batch -- are held
bit for bit to Pillow's libjpeg-turbo decode and to the coefficients the writer was given; files the parser must refuse are refused by
the loaders, by index.  Only the fixture is read: Pillow is not needed here.  Every stream is valid; nothing is excluded."""
import os

import numpy as np
import pytest

from conftest import ROOT

import jpeg_crop_cases as cc
import jpeg_writer as jw

pytestmark = pytest.mark.gpu

OUT = (40, 40)


def streams():
    return jw.streams(os.path.join(ROOT, "tests", "golden", "jpeg_streams.npz"))


def _decode(datas, subseq=0, coefficients=False):
    import torch
    from capf import lib as capf
    r = capf.jpeg_decode_batch(datas, "cuda", subseq, coefficients)
    torch.cuda.synchronize()
    outs = [o.cpu().numpy() for o in r[0]]
    status = r[1].cpu().numpy()
    if coefficients:
        return outs, status, [[c.cpu().numpy() for c in cs] for cs in r[2]]
    return outs, status


@pytest.fixture(scope="module")
def host_coefficients():
    """what the coefficient blocks of every decodable file must be: the writer's own where the file is writer-made, the host walk's
    (itself held to Pillow's pixels through the restatement, tests/test_jpeg_streams.py) for the Pillow-made ones"""
    from capf import lib as capf
    s = streams()
    return {n: s.coefficients(n) or capf.jpeg_coefficients(s.data(n)) for n in s.decodable()}


@pytest.mark.parametrize("subseq", [0, 4])
def test_every_decodable_file_in_one_batch_call(subseq, host_coefficients):
    """409 files in ONE call, from 1 x 1 to 400 x 300 (475 restart segments of 12 bits), at the default subsequence length and at 4 bytes:
    status 0, pixels == Pillow's, coefficients == the writer's; a second call gives the same bits"""
    s = streams()
    names = s.decodable()
    assert len(names) == 409
    datas = [s.data(n) for n in names]
    outs, status, coefs = _decode(datas, subseq, coefficients=True)
    assert not status.any(), [(n, int(st)) for n, st in zip(names, status) if st]
    bad_px = [n for n, o in zip(names, outs) if o.shape != s.bgr(n).shape or not np.array_equal(o, s.bgr(n))]
    assert not bad_px, (len(bad_px), bad_px[:12])
    bad_cf = [n for n, c in zip(names, coefs)
              if len(c) != len(host_coefficients[n]) or not all(a.shape == b.shape and np.array_equal(a, b) for a, b in zip(c, host_coefficients[n]))]
    assert not bad_cf, (len(bad_cf), bad_cf[:12])
    outs2, status2, coefs2 = _decode(datas, subseq, coefficients=True)
    assert not status2.any()
    assert all(np.array_equal(a, b) for a, b in zip(outs, outs2))
    assert all(np.array_equal(a, b) for ca, cb in zip(coefs, coefs2) for a, b in zip(ca, cb))


def test_host_walk_route_on_the_tiny_family_and_every_written_variant():
    """capf_jpeg_decode (host Huffman walk + the one-file pixel kernels): the whole tiny family, every long-code family x sampling (at
    restart interval 1, and the 400 x 300 file), every layout and control file == Pillow's pixels"""
    import torch
    from capf import lib as capf
    s = streams()
    names = s.family("tiny", "layout", "control") + [n for n in s.family("long") if "_ri1" in n]
    assert len(names) == 325 + 25 + 10 + 17
    outs = [capf.jpeg_decode(s.data(n)) for n in names]
    torch.cuda.synchronize()
    bad = [n for n, o in zip(names, outs) if tuple(o.shape) != s.bgr(n).shape or not np.array_equal(o.cpu().numpy(), s.bgr(n))]
    assert not bad, (len(bad), bad[:12])


@pytest.fixture(scope="module")
def crop_set():
    """the tiny family and the 4:2:0 long-code files, with Pillow's pixels uploaded once"""
    import torch
    s = streams()
    names = s.family("tiny") + [n for n in s.family("long") if n.startswith("long/420_")]
    assert len(names) == 325 + 13
    return names, [s.data(n) for n in names], [torch.from_numpy(np.ascontiguousarray(s.bgr(n))).cuda() for n in names]


@pytest.mark.parametrize("matrix", ["identity", "shift_int", "shift_half"])
def test_crop_route_equals_the_warp_of_the_stored_pixels(matrix, crop_set):
    """capf_jpeg_decode_crop_batch to 40 x 40 with the identity, an integer shift and a half-pixel shift: the tiny images sit inside a zero
    border, so the image-edge rules and the replicated narrow chroma are met through the patch origin; == capf_warp_affine of Pillow's
    pixels, and of capf_jpeg_decode_batch's frames, at the default subsequence length and at 4 bytes"""
    import torch
    from capf import lib as capf
    names, datas, uploaded = crop_set
    mats = np.stack([cc.matrices(8, 8, *OUT)[matrix]] * len(names))
    assert matrix != "shift_int" or mats[0].tolist() == [[1.0, 0.0, -3.0], [0.0, 1.0, -2.0]]
    want = capf.warp_affine(uploaded, mats, OUT).cpu().numpy()
    assert want.shape == (len(names), 40, 40, 3) and want.any()
    for subseq in (0, 4):
        crops, status = capf.jpeg_decode_crop_batch(datas, mats, OUT, "cuda", subseq)
        frames, status2 = capf.jpeg_decode_batch(datas, "cuda", subseq)
        two_step = capf.warp_affine(frames, mats, OUT)
        torch.cuda.synchronize()
        assert not status.cpu().numpy().any() and not status2.cpu().numpy().any()
        crops, two_step = crops.cpu().numpy(), two_step.cpu().numpy()
        bad = [n for i, n in enumerate(names) if not np.array_equal(crops[i], want[i]) or not np.array_equal(crops[i], two_step[i])]
        assert not bad, (matrix, subseq, len(bad), bad[:12])


def test_refused_files_are_named_by_the_loaders_and_neighbours_stay_exact():
    """a refused file (RGB by Adobe transform 0, RGB by component ids, Pillow's keep_rgb, Tq = 5) between two good ones: imread_batch and
    load_and_crop_batch(decoder="device_crop") raise CapfError naming index 1 and enqueue nothing; the two good files, in a batch of their
    own, equal the fixture"""
    from capf.lib import CapfError
    from mvn.utils.img import imread_batch, load_and_crop_batch
    s = streams()
    good = ["tiny/420_w4_h7", "long/422_dense_ri3"]
    for name in ("refused/444_adobe0_nojfif", "refused/420_idsRGB_nojfif", "refused/pillow_keep_rgb", "refused/420_tq5"):
        assert s.status(name) != 0
        datas = [s.data(good[0]), s.data(name), s.data(good[1])]
        with pytest.raises(CapfError, match=r"\[1\]"):
            imread_batch(datas)
        with pytest.raises(CapfError, match=r"\[1\]"):
            load_and_crop_batch(datas, [(4.0, 4.0)] * 3, [(0.2, 0.2)] * 3, OUT, decoder="device_crop")
    outs, status = _decode([s.data(n) for n in good])
    assert not status.any()
    for n, o in zip(good, outs):
        assert np.array_equal(o, s.bgr(n)), n
