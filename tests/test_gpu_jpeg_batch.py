"""N3, batched decode on the MI355X: capf_jpeg_decode_batch (device entropy decode + batched IDCT / colour) is bit-identical to the
libjpeg goldens, to capf_jpeg_decode (host Huffman walk) and to Pillow, composes across a batch, is deterministic, and flags corrupt files
without disturbing their neighbours."""
import io
import os

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = ["rgb444_q90", "rgb420_q75_odd", "rgb422_q50", "rgb420_q95_opt", "rgb420_q85_rst", "rgb444_q30", "grey_q80", "rgb420_q100_sat"]


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"), allow_pickle=False)


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


def _frames(n, seed=21):
    from PIL import Image
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        H, W = (1002, 1000) if i % 3 else (640, 480)
        y, x = np.mgrid[0:H, 0:W]
        img = np.clip(np.stack([128 + 100 * np.sin(x / (30.0 + i)) * np.cos(y / 51.0), 128 + 90 * np.cos(x / 25.0 + y / (19.0 + i)),
                                (x + 2 * y + 7 * i) % 256], -1) + rng.normal(0, 6, (H, W, 3)), 0, 255).astype(np.uint8)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "JPEG", quality=(75, 90)[i % 2], subsampling=(2, 0)[(i // 2) % 2])
        out.append(buf.getvalue())
    return out


def test_all_goldens_in_one_call():
    """eight files of mixed size, sampling and restart interval in ONE call: each BGR output equals its libjpeg golden, each coefficient
    block equals the host decoder's"""
    from capf import lib as capf
    g = _golden()
    datas = [g[n + ":jpeg"].tobytes() for n in CASES]
    for subseq in (0, 4):
        outs, status, coefs = _decode(datas, subseq, coefficients=True)
        assert not status.any(), status
        for n, d, o, c in zip(CASES, datas, outs, coefs):
            assert np.array_equal(o, g[n + ":bgr"]), (n, subseq)
            assert all(np.array_equal(a, b) for a, b in zip(c, capf.jpeg_coefficients(d))), (n, subseq)


def test_frame_sized_batch_matches_the_host_path_and_pillow():
    pytest.importorskip("PIL")
    from PIL import Image
    from capf import lib as capf
    datas = _frames(16)
    host = [capf.jpeg_decode(d).cpu().numpy() for d in datas]
    for subseq in (0, 4):
        outs, status = _decode(datas, subseq)
        assert not status.any(), (subseq, status)
        for i, (o, h, d) in enumerate(zip(outs, host, datas)):
            assert np.array_equal(o, h), (i, subseq)
            if subseq == 0:
                assert np.array_equal(o, np.asarray(Image.open(io.BytesIO(d)).convert("RGB"))[..., ::-1]), i


def test_composition_and_determinism():
    g = _golden()
    datas = [g[n + ":jpeg"].tobytes() for n in CASES]
    alone, st = _decode([datas[4]])
    assert not st.any()
    first, st1 = _decode(datas)
    second, st2 = _decode(datas)
    assert np.array_equal(alone[0], first[4])
    assert not st1.any() and not st2.any()
    assert all(np.array_equal(a, b) for a, b in zip(first, second))


def test_corrupt_files_are_flagged_and_neighbours_stay_exact():
    """byte flips in the entropy data of some files of a batch: each flagged file has a status bit or the host path's exact output; the
    intact files in the same batch stay bit-exact"""
    from capf import lib as capf
    from capf.lib import CapfError
    g = _golden()
    good = [g[n + ":jpeg"].tobytes() for n in CASES]
    rng = np.random.default_rng(7)
    corrupt = []
    while len(corrupt) < 24:
        src = good[int(rng.integers(0, len(good)))]
        bad = bytearray(src)
        sos = bytes(src).find(b"\xff\xda")
        for pos in rng.integers(sos + 20, len(bad) - 2, size=int(rng.integers(1, 4))):
            bad[pos] = int(rng.integers(0, 256))
        try:
            capf.jpeg_coefficients(bytes(bad))                         # headers intact and the host path takes it
        except CapfError:
            continue
        corrupt.append(bytes(bad))
    batch = [x for pair in zip(good * 3, corrupt) for x in pair]
    outs, status = _decode(batch, 8)
    flagged = 0
    for i, (d, o, s) in enumerate(zip(batch, outs, status)):
        if i % 2 == 0:
            assert s == 0 and np.array_equal(o, g[CASES[(i // 2) % 8] + ":bgr"]), i
        elif s:
            flagged += 1
        else:
            assert np.array_equal(o, capf.jpeg_decode(d).cpu().numpy()), i
    assert flagged > 0


def test_load_and_crop_batch_device_decoder_matches_the_default():
    pytest.importorskip("PIL")
    from mvn.utils.img import imread_batch, load_and_crop_batch
    from capf.lib import CapfError
    base = _frames(8, seed=5)
    files = [base[i % 8] for i in range(64)]
    rng = np.random.default_rng(3)
    centers = [(float(rng.uniform(300, 700)), float(rng.uniform(300, 700))) for _ in files]
    scales = [(float(rng.uniform(1.0, 2.0)),) * 2 for _ in files]
    want = load_and_crop_batch(files, centers, scales, (192, 256)).cpu().numpy()
    got = load_and_crop_batch(files, centers, scales, (192, 256), decoder="device").cpu().numpy()
    assert np.array_equal(got, want)
    rst = _golden()["rgb420_q85_rst:jpeg"].tobytes()
    m = rst.index(b"\xff\xd0", rst.index(b"\xff\xda"))
    with pytest.raises(CapfError, match="#1"):
        imread_batch([rst, rst[:m] + rst[m + 2:]])                     # a restart marker removed
