"""N3, batched decode (capf_jpeg_decode_batch): its entropy stage -- device unstuffing, subsequence lanes, sync rounds and the serial
fallback of csrc/jpeg_sync.h -- run serially on the CPU by capf_jpeg_coefficients_subseq, held to the host decoder's coefficients
(capf_jpeg_coefficients, the independent oracle) on the committed goldens, on Pillow-made frame-sized files and on corrupt streams."""
import io
import os

import numpy as np
import pytest

from conftest import ROOT

CASES = ["rgb444_q90", "rgb420_q75_odd", "rgb422_q50", "rgb420_q95_opt", "rgb420_q85_rst", "rgb444_q30", "grey_q80", "rgb420_q100_sat"]
SUBSEQ = [4, 8, 64, 1024, 0]          # 4 bytes: a sync at nearly every boundary and the serial fallback; 0: the default


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"), allow_pickle=False)


def _same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def _frame(H=1002, W=1000, seed=11, sigma=6.0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    return np.clip(np.stack([128 + 100 * np.sin(x / 37.0) * np.cos(y / 51.0), 128 + 90 * np.cos(x / 25.0 + y / 19.0), (x + 2 * y) % 256], -1)
                   + rng.normal(0, sigma, (H, W, 3)), 0, 255).astype(np.uint8)


def _encode(img, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def _entropy_range(data):
    """(first byte after SOS, offset of EOI)"""
    p = 2
    while True:
        m, ln = data[p + 1], (data[p + 2] << 8) | data[p + 3]
        if m == 0xDA:
            return p + 2 + ln, data.rindex(b"\xff\xd9")
        p += 2 + ln


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("subseq", SUBSEQ)
def test_subsequence_emulation_equals_the_host_decoder_on_the_goldens(name, subseq):
    from capf import lib as capf
    data = _golden()[name + ":jpeg"].tobytes()
    assert _same(capf.jpeg_coefficients_subseq(data, subseq), capf.jpeg_coefficients(data))


def test_subsequence_emulation_on_frame_sized_files():
    """1000 x 1002 frames (Human3.6M's resolution): every sampling mode, grey, optimised tables, restart markers, qualities 30 - 100, and
    a file whose entropy data is dense in FF 00 stuffing."""
    pytest.importorskip("PIL")
    from capf import lib as capf
    img = _frame()
    files = [("grey", _encode(img[..., 0].copy(), quality=85))]
    files += [(f"sub{s}", _encode(img, quality=88, subsampling=s)) for s in (0, 1, 2)]
    files += [("optimize", _encode(img, quality=75, subsampling=2, optimize=True)),
              ("rst1", _encode(img, quality=80, subsampling=2, restart_marker_blocks=1)),
              ("rst7", _encode(img, quality=90, subsampling=0, restart_marker_blocks=7))]
    files += [(f"q{q}", _encode(img, quality=q, subsampling=2)) for q in (30, 50, 95, 100)]
    checker = ((np.indices((256, 248)).sum(0) % 2) * 255).astype(np.uint8)[..., None].repeat(3, -1)
    dense = _encode(checker, quality=100, subsampling=0)
    a, e = _entropy_range(dense)
    assert dense[a:e].count(b"\xff\x00") > 0.05 * (e - a)
    files.append(("ff00", dense))
    for name, data in files:
        want = capf.jpeg_coefficients(data)
        for subseq in (4, 0) if name in ("sub2", "rst1", "ff00") else (0,):
            assert _same(capf.jpeg_coefficients_subseq(data, subseq), want), (name, subseq)


def _flag_or_equal(capf, data, subseq):
    """the emulation flags the file (CapfError), or returns exactly what the host decoder returns"""
    from capf.lib import CapfError
    try:
        got = capf.jpeg_coefficients_subseq(data, subseq)
    except CapfError:
        return "flagged"
    assert _same(got, capf.jpeg_coefficients(data))
    return "equal"


def test_corrupt_streams_are_flagged_or_decoded_exactly_like_the_host():
    """The byte-flip recipe of test_jpeg.py's corrupt-stream test, truncations, and removed / extra restart markers: never a crash (the
    process survives), and never a result that differs from the host decoder's without a flag."""
    from capf import lib as capf
    from capf.lib import CapfError
    g = _golden()
    good = g["rgb420_q75_odd:jpeg"].tobytes()
    rng = np.random.default_rng(5)
    seen = set()
    for it in range(300):
        bad = bytearray(good)
        for pos in rng.integers(2, len(bad), size=int(rng.integers(1, 6))):
            bad[pos] = int(rng.integers(0, 256))
        try:
            capf.jpeg_info(bytes(bad))
            capf.jpeg_coefficients(bytes(bad))
        except CapfError:
            continue                                                   # refused by the host path: nothing to compare
        seen.add(_flag_or_equal(capf, bytes(bad), (4, 0)[it % 2]))
    a, e = _entropy_range(good)
    for cut in range(a + 1, len(good), 7):                             # truncated inside the entropy data
        try:
            capf.jpeg_coefficients(good[:cut])
        except CapfError:
            continue
        seen.add(_flag_or_equal(capf, good[:cut], 8))
    assert "flagged" in seen and "equal" in seen
    rst = g["rgb420_q85_rst:jpeg"].tobytes()
    a, e = _entropy_range(rst)
    marks = [i for i in range(a, e - 1) if rst[i] == 0xFF and 0xD0 <= rst[i + 1] <= 0xD7]
    assert len(marks) >= 2
    for m in (marks[0], marks[len(marks) // 2], marks[-1]):
        removed = rst[:m] + rst[m + 2:]
        with pytest.raises(CapfError):
            capf.jpeg_coefficients_subseq(removed, 0)                 # restart-marker count off by one
        extra = rst[:m] + bytes([0xFF, rst[m + 1]]) + rst[m:]
        assert _flag_or_equal(capf, extra, 0) == "flagged"
    # an entropy-coded segment cut short of its MCUs decodes zeros on the host; the device path cannot see them and flags the file
    short = rst[:marks[1] - 20] + rst[marks[1]:]
    assert _flag_or_equal(capf, short, 4) in ("flagged", "equal")


def test_batch_info_geometry_and_unsupported_files():
    from capf import lib as capf
    g = _golden()
    datas = [g[n + ":jpeg"].tobytes() for n in CASES]
    rows, scratch = capf.jpeg_batch_info(datas)
    assert scratch and scratch > 0
    for d, r in zip(datas, rows):
        i = capf.jpeg_info(d)
        assert (r["width"], r["height"], r["components"], r["status"]) == (i["width"], i["height"], i["components"], 0)
        assert r["coef_elems"] == sum(c.size for c in capf.jpeg_coefficients(d))
    # a smaller subsequence needs more lanes, so more scratch
    assert capf.jpeg_batch_info(datas, 4)[1] > capf.jpeg_batch_info(datas, 1024)[1]
    extra = [b"\x89PNG\r\n\x1a\n" + bytes(64), datas[0][:40]]
    try:
        from PIL import Image
        buf = io.BytesIO()
        Image.fromarray((np.arange(32 * 32 * 3) % 251).astype(np.uint8).reshape(32, 32, 3)).save(buf, "JPEG", quality=80, progressive=True)
        extra.append(buf.getvalue())
    except ImportError:
        pass
    rows, scratch = capf.jpeg_batch_info([datas[0]] + extra + [datas[1]])
    assert scratch is None
    assert rows[0]["status"] == 0 and rows[-1]["status"] == 0
    assert all(r["status"] != 0 for r in rows[1:-1])
    if len(extra) == 3:
        assert rows[3]["status"] == -2                                 # CAPF_ERR_UNSUPPORTED: progressive
