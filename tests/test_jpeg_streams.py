"""N3, the JPEG front end on streams Pillow's encoder does not make (tests/golden/jpeg_streams.npz, oracle/make_jpeg_stream_goldens.py): images
of a few pixels, Huffman codes of every length written from KNOWN coefficients (tests/jpeg_writer.py), legal marker layouts, and files the
parser has to refuse -- three-component RGB, a quantisation-table selector above 3.  The host half (capf_jpeg_info / capf_jpeg_coefficients),
the subsequence emulation of the device walk and the numpy restatement (oracle/jpeg_oracle.py) are held, bit for bit, to the writer's
coefficients and to Pillow's libjpeg-turbo decode.  The GPU routes run the same fixture in tests/test_gpu_jpeg_streams.py."""
import io
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.join(ROOT, "oracle"))

import jpeg_writer as jw  # noqa: E402


def streams():
    return jw.streams(os.path.join(ROOT, "tests", "golden", "jpeg_streams.npz"))


def test_fixture_holds_the_families_and_stays_small():
    s = streams()
    count = {f: len(s.family(f)) for f in ("tiny", "long", "layout", "refused", "control")}
    assert count == {"tiny": 13 * 8 * 3 + 13, "long": 49, "layout": 25, "refused": 9, "control": 10}, count
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "jpeg_streams.npz")) < 300 * 1000
    assert all(s.coefficients(n) is not None for n in s.family("long", "layout", "control"))
    for n in s.family("refused"):
        assert s.status(n) in (-1, -2) and s._part("bgr", n).size == 0
    big = s.data("long/420_empty_ri1_400x300")
    scan = big[big.index(b"\xff\xda"):]
    assert sum(scan.count(bytes([0xFF, 0xD0 + k])) for k in range(8)) == 474 and len(scan) < 475 * 4 + 16   # 475 segments of 12 bits each


def test_stream_recipe_regenerates_the_committed_fixture():
    """oracle/make_jpeg_stream_goldens.py on this environment's Pillow and numpy reproduces the committed bytes, pixels and coefficients"""
    pytest.importorskip("PIL")
    import make_jpeg_stream_goldens
    rec = make_jpeg_stream_goldens.make()
    old = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_streams.npz"), allow_pickle=False)
    assert set(rec) == set(old.files)
    for k in rec:
        if k not in ("pillow_version", "libjpeg_turbo"):
            assert np.array_equal(rec[k], old[k]), k


def test_writer_tables_hold_every_code_length():
    dc, ac = jw.huffman_codes(*jw.DC_LONG), jw.huffman_codes(*jw.AC_LONG)
    assert sorted(l for _, l in dc.values()) == list(range(1, 12)) + [16] and sorted(dc) == list(range(12))
    assert sorted(l for _, l in ac.values()) == list(range(1, 9)) + [16] * 154 and len(ac) == 162
    assert all(code != (1 << l) - 1 for code, l in list(dc.values()) + list(ac.values()))      # the all-ones code is unused
    # prefix-free: no code is the head of another
    for tab in (dc, ac):
        words = sorted(format(c, "0%db" % l) for c, l in tab.values())
        assert not any(b.startswith(a) for a, b in zip(words, words[1:]))


def test_host_walk_returns_the_coefficients_the_writer_was_given():
    """every writer-made file: capf_jpeg_info reports the geometry written, capf_jpeg_coefficients the coefficients written -- no decoder
    in between, so this pins the host Huffman walk on its own (codes of 1..16 bits, ZRL chains, k = 63, category 11 differences, one-byte
    restart segments, fill bytes, 16-bit tables, odd marker orders)"""
    from capf import lib as capf
    s, n = streams(), 0
    for name in s.family("long", "layout", "control"):
        want = s.coefficients(name)
        info = capf.jpeg_info(s.data(name))
        assert (info["width"], info["height"], info["components"], info["h_samp"], info["v_samp"]) == s.geometry(name), name
        got = capf.jpeg_coefficients(s.data(name))
        assert len(got) == len(want), name
        for c, (a, b) in enumerate(zip(got, want)):
            assert a.shape == b.shape and np.array_equal(a, b), (name, c)
        n += 1
    assert n == 84


@pytest.mark.parametrize("subseq", [4, 8, 64, 0])
def test_subsequence_emulation_equals_the_writer_and_the_host_walk(subseq):
    """the device algorithm run serially on the CPU, at subsequences of 4, 8, 64 and the default 256 bytes: the writer's coefficients where
    they are known, the host walk's on the Pillow-made files"""
    from capf import lib as capf
    s = streams()
    for name in s.decodable():
        want = s.coefficients(name) or capf.jpeg_coefficients(s.data(name))
        got = capf.jpeg_coefficients_subseq(s.data(name), subseq)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)) and len(got) == len(want), (name, subseq)


def _restated(data, coefs=None):
    import jpeg_oracle as jo
    from capf import lib as capf
    info = capf.jpeg_info(data)
    coefs = coefs if coefs is not None else capf.jpeg_coefficients(data)
    return jo.decode_from_coefficients(coefs, jw.quant_tables(data), info["width"], info["height"], info["h_samp"], info["v_samp"])


def test_restatement_reproduces_pillow_on_every_decodable_file():
    """host half + numpy restatement == Pillow's decode stored in the fixture: images down to 1 x 1 (libjpeg replicates chroma narrower than
    three samples, jdsample.c), every long-code file, every layout, and the control files, which must convert as YCbCr"""
    s = streams()
    bad = [n for n in s.decodable() if not np.array_equal(_restated(s.data(n)), s.bgr(n))]
    assert not bad, (len(bad), bad[:12])
    assert len(s.decodable()) == 325 + 49 + 25 + 10


def test_tiny_sweep_against_the_installed_pillow():
    """all of H, W in {1..9, 15..18, 31..33} x {4:4:4, 4:2:2, 4:2:0}, 768 files encoded and decoded on the spot by this environment's
    Pillow (the fixture carries a subset): the host half + restatement equal its decode everywhere"""
    pytest.importorskip("PIL")
    from PIL import Image
    rng = np.random.default_rng(7)
    sizes = list(range(1, 10)) + [15, 16, 17, 18, 31, 32, 33]
    bad, n = [], 0
    for H in sizes:
        for W in sizes:
            px = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            for sub in (0, 1, 2):
                buf = io.BytesIO()
                Image.fromarray(px).save(buf, "JPEG", quality=90, subsampling=sub)
                data = buf.getvalue()
                want = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]
                if not np.array_equal(_restated(data), want):
                    bad.append((W, H, sub))
                n += 1
    assert n == 768 and not bad, (len(bad), bad[:12])


def test_refused_files_are_refused_by_every_host_entry():
    """libjpeg decodes the RGB files WITHOUT a colour conversion (jdapimin.c default_decompress_parms) and refuses Tq = 5 ("no quantization
    table"); the product has no unconverted route, so it must refuse both kinds: CapfError from the one-file calls, the fixture's status in
    that row of the batch calls -- no scratch size, the neighbours' rows at 0"""
    from capf import lib as capf
    from capf.lib import CapfError
    s = streams()
    good = [s.data("layout/420_plain"), s.data("tiny/422_w3_h7")]
    eye = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    refused = s.family("refused")
    assert len(refused) == 9
    accepted = []
    for name in refused:
        for call in (capf.jpeg_info, capf.jpeg_coefficients, capf.jpeg_coefficients_subseq):
            try:
                call(s.data(name))
                accepted.append((name, call.__name__))
            except CapfError:
                pass
    assert not accepted, accepted
    for name in refused:
        data = s.data(name)
        rows, scratch = capf.jpeg_batch_info([good[0], data, good[1]])
        assert scratch is None and [r["status"] for r in rows] == [0, s.status(name), 0], name
        assert (rows[1]["width"], rows[1]["height"], rows[1]["coef_elems"]) == (0, 0, 0), name
        rc, rows, scratch = capf.jpeg_crop_batch_info([good[0], data, good[1]], [eye] * 3, (40, 40))
        assert rc == s.status(name) and scratch is None and [r["status"] for r in rows] == [0, s.status(name), 0], name
        assert rows[1]["coef_elems"] == 0 and rows[1]["pixel_rect"] == (0, 0, 0, 0), name
    assert sorted(s.status(n) for n in refused) == [-2] * 7 + [-1] * 2          # seven RGB files: CAPF_ERR_UNSUPPORTED; Tq = 5: CAPF_ERR_INVALID


def test_control_files_decode_as_ycbcr_and_equal_pillow():
    """JFIF + Adobe 0, Adobe 1, Adobe 2, lower-case r,g,b ids, JFIF + ids R,G,B: libjpeg converts all of these, and so must the product"""
    from capf import lib as capf
    s = streams()
    control = s.family("control")
    assert len(control) == 10
    for name in control:
        coefs = capf.jpeg_coefficients(s.data(name))
        assert all(np.array_equal(a, b) for a, b in zip(coefs, s.coefficients(name))), name
        assert np.array_equal(_restated(s.data(name), coefs), s.bgr(name)), name
    rows, scratch = capf.jpeg_batch_info([s.data(n) for n in control])
    assert scratch and not any(r["status"] for r in rows)


def test_shared_parser_reads_wide_tables_and_fill_bytes():
    """jpeg_writer.quant_tables (what test_jpeg.py's _quant_tables goes through): 16-bit tables with entries above 255, fill bytes before
    the segments, merged DQT -- the tables the writer was given come back"""
    s = streams()
    rc = np.add.outer(np.arange(8), np.arange(8)).reshape(64)              # (the recipe's tables, restated: row + column of each entry)
    luma, chroma, wide = 1 + rc, 2 + 2 * rc, np.where(rc >= 13, 260 + rc, 1 + rc)
    for base in ("420", "444"):
        got = jw.quant_tables(s.data(f"layout/{base}_everything_ri2"))
        assert len(got) == 3 and np.array_equal(got[0], wide) and np.array_equal(got[1], chroma) and np.array_equal(got[2], chroma)
        assert got[0].max() > 255
        got = jw.quant_tables(s.data(f"layout/{base}_plain"))
        assert np.array_equal(got[0], luma) and np.array_equal(got[2], chroma)
