"""Writes tests/golden/jpeg_streams.npz: JPEG files the decoders have to take (or refuse) that oracle/make_jpeg_goldens.py does not reach --
    tiny/      Pillow-encoded uniform noise at widths 1..9, 15..17, 33 x heights 1..3, 7..9, 16, 17 in 4:4:4 / 4:2:2 / 4:2:0, grey on a diagonal
    long/      written by tests/jpeg_writer.py from known coefficients with Huffman codes of every length 1..16 (dense / sparse / extreme /
               empty blocks x 4:4:4 / 4:2:2 / 4:2:0 / grey x restart interval 0 / 1 / 3, and one 400 x 300 file of one-byte segments)
    layout/    the writer's layout switches (fill bytes, merged tables, 16-bit tables, COM / APP1, DRI first, trailing bytes, odd ids, ...)
    refused/   three-component files libjpeg takes for RGB, and a quantisation-table selector of 5: only the status the parser must return
    control/   marker / id combinations next to those that libjpeg still takes for YCbCr
and, for every decodable file, its decode by Pillow's bundled libjpeg-turbo (BGR).  All files sit in ONE uint8 blob with an offsets array
(the repeated headers compress together), likewise the pixels and the writer's coefficients (int16, component after component).
    python oracle/make_jpeg_stream_goldens.py [--check]"""
import io
import os
import sys
import zlib

import numpy as np
from PIL import Image, features

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import jpeg_writer as jw  # noqa: E402

PATH = os.path.join(ROOT, "tests", "golden", "jpeg_streams.npz")
SAMPLING = {"444": (3, 1, 1), "422": (3, 2, 1), "420": (3, 2, 2), "grey": (1, 1, 1)}       # name -> components, h, v
TINY_W, TINY_H = (1, 2, 3, 4, 5, 6, 7, 8, 9, 15, 16, 17, 33), (1, 2, 3, 7, 8, 9, 16, 17)
UNSUPPORTED, INVALID = -2, -1                                                              # CAPF_ERR_UNSUPPORTED, CAPF_ERR_INVALID


def _rng(name):
    return np.random.default_rng([zlib.crc32(name.encode()), 20261019])


def _shapes(W, H, nc, hs, vs):
    mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
    return [(my * vs, mx * hs, 64)] + [(my, mx, 64)] * (nc - 1)


# ---- coefficient families (natural order) ---------------------------------------------------------------------------------------------------
def dense(rng, shape):
    """all 64 coefficients nonzero, |AC| <= 3: no EOB anywhere"""
    a = rng.integers(1, 4, shape) * rng.choice([-1, 1], shape)
    a[..., 0] = rng.integers(1, 61, shape[:2]) * rng.choice([-1, 1], shape[:2])
    return a


def sparse(rng, shape):
    """nonzeros at zigzag positions 20 and 63 only: ZRL chains, and a coefficient at k = 63"""
    a = np.zeros(shape, np.int64)
    a[..., 0] = rng.integers(-100, 101, shape[:2])
    a[..., jw.ZIGZAG[20]] = rng.integers(1, 3, shape[:2]) * rng.choice([-1, 1], shape[:2])
    a[..., jw.ZIGZAG[63]] = rng.integers(1, 3, shape[:2])
    return a


def extreme(rng, shape):
    """DC alternating +-1023 (differences up to +-2046, category 11), AC[1] in {0, +-1023} (category 10)"""
    a = np.zeros(shape, np.int64)
    by, bx = np.mgrid[0:shape[0], 0:shape[1]]
    a[..., 0] = np.where((by + bx) % 2 == 0, 1023, -1023)
    a[..., 1] = rng.choice([-1023, 0, 1023], shape[:2])
    return a


def empty(rng, shape):
    """every block DC 0 + EOB: the most blocks per byte"""
    return np.zeros(shape, np.int64)


def mixed(rng, shape):
    """the layout family's blocks: moderate DC, about one coefficient in seven nonzero, +-1 where the 16-bit tables go above 255"""
    a = np.where(rng.random(shape) < 0.15, rng.integers(1, 3, shape) * rng.choice([-1, 1], shape), 0)
    rc = np.add.outer(np.arange(8), np.arange(8)).reshape(64)
    a[..., rc >= 13] = np.sign(a[..., rc >= 13])
    a[..., 0] = rng.integers(-40, 41, shape[:2])
    return a


_RC = np.add.outer(np.arange(8), np.arange(8)).reshape(64)
Q_ONES = [np.ones(64, np.int64)] * 2
Q_LAYOUT = [1 + _RC, 2 + 2 * _RC]                                      # 1..15 and 2..30
Q_BIG = [np.where(_RC >= 13, 260 + _RC, 1 + _RC), 2 + 2 * _RC]        # three entries of the first table above 255


def _written(name, W, H, sampling, gen, qts=Q_ONES, **kw):
    nc, hs, vs = SAMPLING[sampling]
    rng = _rng(name)
    coefs = [gen(rng, s) for s in _shapes(W, H, nc, hs, vs)]
    n = min(nc, 2)
    data = jw.write(coefs, W, H, hs, vs, qts[:n], [jw.DC_LONG] * n, [jw.AC_LONG] * n, **kw)
    return name, data, (W, H, nc, hs, vs), coefs


def _pillow(name, W, H, sampling, **kw):
    nc, hs, vs = SAMPLING[sampling]
    px = _rng(name).integers(0, 256, (H, W, 3) if nc == 3 else (H, W), dtype=np.uint8)
    buf = io.BytesIO()
    if nc == 3:
        kw["subsampling"] = {"444": 0, "422": 1, "420": 2}[sampling]
    Image.fromarray(px).save(buf, "JPEG", quality=90, **kw)
    return name, buf.getvalue(), (W, H, nc, hs, vs), None


def files():
    """-> list of (name, bytes, (W, H, components, h, v), coefficients or None, expected status)"""
    out = []
    for s in ("444", "422", "420"):
        out += [_pillow(f"tiny/{s}_w{W}_h{H}", W, H, s) + (0,) for W in TINY_W for H in TINY_H]
    out += [_pillow(f"tiny/grey_w{W}_h{TINY_H[i % 8]}", W, TINY_H[i % 8], "grey") + (0,) for i, W in enumerate(TINY_W)]
    for s in SAMPLING:
        for gen in (dense, sparse, extreme, empty):
            out += [_written(f"long/{s}_{gen.__name__}_ri{ri}", 37, 29, s, gen, restart=ri) + (0,) for ri in (0, 1, 3)]
    out.append(_written("long/420_empty_ri1_400x300", 400, 300, "420", empty, restart=1) + (0,))
    for s in ("420", "444"):
        def lay(tag, status=0, qts=Q_LAYOUT, family="layout", **kw):
            return _written(f"{family}/{s}_{tag}", 21, 19, s, mixed, qts=qts, **kw) + (status,)
        out += [lay("plain"), lay("fill_ri1", restart=1, layout=("fill",)), lay("merged", layout=("merged",)),
                lay("q16", layout=("q16",)), lay("q16_above_255", qts=Q_BIG, layout=("q16",)), lay("com_app1", layout=("com_app1",)),
                lay("dri_first_ri2", restart=2, layout=("dri_first",)), lay("trailing", layout=("trailing",)),
                lay("ri_beyond_the_scan", restart=1000), lay("everything_ri2", qts=Q_BIG, restart=2,
                                                             layout=("fill", "merged", "q16", "com_app1", "dri_first", "trailing")),
                lay("ids012_nojfif", ids=(0, 1, 2), jfif=False), lay("ids789_nojfif", ids=(7, 8, 9), jfif=False)]
        out += [lay("adobe0_nojfif", UNSUPPORTED, family="refused", jfif=False, adobe=0),
                lay("adobe0_idsRGB_nojfif", UNSUPPORTED, family="refused", jfif=False, adobe=0, ids=(82, 71, 66)),
                lay("idsRGB_nojfif", UNSUPPORTED, family="refused", jfif=False, ids=(82, 71, 66)),
                lay("tq5", INVALID, family="refused", layout=("tq5",))]
        out += [lay("jfif_adobe0", family="control", adobe=0), lay("adobe1_nojfif", family="control", jfif=False, adobe=1),
                lay("adobe2_nojfif", family="control", jfif=False, adobe=2), lay("idsrgb_lower_nojfif", family="control", jfif=False, ids=(114, 103, 98)),
                lay("jfif_idsRGB", family="control", ids=(82, 71, 66))]
    out.append(_written("layout/grey_2x2", 21, 19, "grey", mixed, qts=Q_LAYOUT, layout=("grey_2x2",)) + (0,))
    out.append(_pillow("refused/pillow_keep_rgb", 24, 16, "444", keep_rgb=True) + (UNSUPPORTED,))
    return out


def _blob(arrays, dtype):
    off = np.concatenate([[0], np.cumsum([a.size for a in arrays])]).astype(np.int64)
    return (np.concatenate([a.reshape(-1) for a in arrays]).astype(dtype) if off[-1] else np.zeros(0, dtype)), off


def make():
    rec = {"pillow_version": np.array(Image.__version__), "libjpeg_turbo": np.array(str(features.version("jpg")))}
    names, infos, jpegs, pixels, coefs = [], [], [], [], []
    for name, data, geom, cf, status in files():
        names.append(name)
        infos.append(list(geom) + [status])
        jpegs.append(np.frombuffer(data, np.uint8))
        if status == 0:
            bgr = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))[..., ::-1]
            assert bgr.shape == (geom[1], geom[0], 3), name
        pixels.append(np.ascontiguousarray(bgr) if status == 0 else np.zeros(0, np.uint8))
        coefs.append(np.concatenate([c.reshape(-1) for c in cf]) if cf is not None and status == 0 else np.zeros(0, np.int16))
    rec["names"] = np.array(names)
    rec["info"] = np.array(infos, np.int32)                                # width, height, components, h_samp, v_samp, expected status
    rec["jpeg"], rec["jpeg_off"] = _blob(jpegs, np.uint8)
    rec["bgr"], rec["bgr_off"] = _blob(pixels, np.uint8)
    rec["coef"], rec["coef_off"] = _blob(coefs, np.int16)
    return rec


if __name__ == "__main__":
    rec = make()
    if "--check" in sys.argv:
        old = np.load(PATH, allow_pickle=False)
        bad = [k for k in rec if k not in ("pillow_version", "libjpeg_turbo") and not np.array_equal(rec[k], old[k])]
        print("check jpeg_streams:", "OK" if not bad and set(rec) == set(old.files) else f"MISMATCH {bad}")
        sys.exit(1 if bad or set(rec) != set(old.files) else 0)
    np.savez_compressed(PATH, **rec)
    print(f"-> {PATH} ({len(rec['names'])} files, {os.path.getsize(PATH) / 1024:.0f} KiB, Pillow {Image.__version__}, libjpeg {features.version('jpg')})")
