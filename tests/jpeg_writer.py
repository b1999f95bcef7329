"""TEST INFRASTRUCTURE (numpy only): a baseline JPEG writer that starts from quantised coefficients, so a test knows exactly what the entropy
stage must give back -- a second source of streams next to Pillow's encoder -- and a small marker parser for the tests.  Written from
ITU-T T.81 (Annex B: markers; Annex C: Huffman code assignment; Annex F.1.2: the sequential Huffman encoder); nothing here reads the
product's tables or code.

`write` emits one SOF0 frame with one interleaved scan.  `layout` is a collection of switch names for things a legal file may do and
Pillow's encoder never does:
    "fill"       0xFF fill bytes (T.81 B.1.1.2) before every marker segment and before every RSTn
    "merged"     all quantisation tables in one DQT segment and all Huffman tables in one DHT segment (default: a segment each)
    "q16"        16-bit quantisation tables (Pq = 1)
    "com_app1"   a COM segment, and an APP1 segment whose payload holds FF D8 .. FF C0 ..: the header of an embedded thumbnail
    "dri_first"  DRI in front of the tables and SOF (default: just before SOS)
    "trailing"   bytes after EOI
    "grey_2x2"   a one-component file whose SOF declares 2x2 sampling factors (they mean nothing in a non-interleaved scan, T.81 A.2.2)
    "tq5"        the first component's quantisation-table selector is 5 (T.81 B.2.2 allows 0..3: a file to refuse)"""
import numpy as np

# ZIGZAG[k] = natural (row-major) index of the k-th coefficient in zigzag order (T.81 Figure A.6)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
LAYOUTS = ("fill", "merged", "q16", "com_app1", "dri_first", "trailing", "grey_2x2", "tq5")


def huffman_codes(bits, vals):
    """T.81 Annex C: (bits[16] = number of codes of length 1..16, vals in code order) -> {symbol: (code, length)}"""
    code, k, out = 0, 0, {}
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    assert k == len(vals)
    return out


class _Bits:
    """entropy-coded segment: most significant bit first, 00 stuffed after every FF byte, 1-bits up to the byte boundary before a marker"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, length):
        self.acc = (self.acc << length) | (v & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 255
            self.out.append(b)
            if b == 255:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _magnitude(bw, v, size):
    """F.1.2.1.1 / F.1.2.2.1: the `size` low bits of v, of v - 1 when v is negative"""
    if size:
        bw.put(v if v > 0 else v + (1 << size) - 1, size)


def _encode_block(bw, zz, pred, dc, ac):
    d = zz[0] - pred
    s = abs(d).bit_length()
    bw.put(*dc[s])
    _magnitude(bw, d, s)
    last = max([k for k in range(1, 64) if zz[k]] or [0])
    run = 0
    for k in range(1, last + 1):
        if zz[k] == 0:
            run += 1
            continue
        while run > 15:
            bw.put(*ac[0xF0])                       # ZRL
            run -= 16
        s = abs(zz[k]).bit_length()
        bw.put(*ac[run << 4 | s])
        _magnitude(bw, zz[k], s)
        run = 0
    if last < 63:
        bw.put(*ac[0x00])                           # EOB, only when the last coefficient is zero


def write(coefs, W, H, hs, vs, qts, dc_tables, ac_tables, restart=0, ids=(1, 2, 3), jfif=True, adobe=None, layout=()):
    """coefs: per component [bh, bw, 64] quantised coefficients in natural order over the MCU-padded image (component 0 at hs x vs, the
    others at 1 x 1); qts: quantisation tables [64] natural order; dc_tables / ac_tables: (bits, vals) -- component c uses table
    min(c, len - 1) of each list; restart: MCUs per restart interval (0: none); adobe: None or the APP14 transform byte.  -> bytes"""
    layout = set(layout)
    assert layout <= set(LAYOUTS), layout
    nc = len(coefs)
    fill = b"\xff" * 3 if "fill" in layout else b""

    def seg(marker, payload):
        return fill + bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + bytes(payload)

    out = bytearray(b"\xff\xd8")
    if jfif:
        out += seg(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    if adobe is not None:
        out += seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([adobe]))
    if "com_app1" in layout:
        out += seg(0xFE, b"written from known coefficients")
        out += seg(0xE1, b"Exif\x00\x00" + b"\xff\xd8\xff\xdb\x00\x04\x00\x01\xff\xc0\x00\x0b\x08\x00\x08\x00\x08\x01\x01\x11\x00\xff\xda\x00\xff\xd9")
    dri = seg(0xDD, restart.to_bytes(2, "big")) if restart else b""
    if "dri_first" in layout:
        out += dri
    tabs = []
    for i, q in enumerate(qts):
        zz = [int(q[ZIGZAG[k]]) for k in range(64)]
        if "q16" in layout:
            tabs.append(bytes([0x10 | i]) + b"".join(v.to_bytes(2, "big") for v in zz))
        else:
            tabs.append(bytes([i]) + bytes(zz))
    out += seg(0xDB, b"".join(tabs)) if "merged" in layout else b"".join(seg(0xDB, t) for t in tabs)
    samp = [(hs, vs)] + [(1, 1)] * (nc - 1)
    sof = bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([nc])
    for c in range(nc):
        h, v = (2, 2) if "grey_2x2" in layout else samp[c]
        tq = 5 if "tq5" in layout and c == 0 else min(c, len(qts) - 1)
        sof += bytes([ids[c], h << 4 | v, tq])
    out += seg(0xC0, sof)
    tabs = []
    for i in range(len(dc_tables)):
        for tc, (bits, vals) in ((0, dc_tables[i]), (1, ac_tables[i])):
            tabs.append(bytes([tc << 4 | i]) + bytes(bits) + bytes(vals))
    out += seg(0xC4, b"".join(tabs)) if "merged" in layout else b"".join(seg(0xC4, t) for t in tabs)
    if "dri_first" not in layout:
        out += dri
    sos = bytes([nc])
    for c in range(nc):
        sos += bytes([ids[c], min(c, len(dc_tables) - 1) << 4 | min(c, len(ac_tables) - 1)])
    out += seg(0xDA, sos + b"\x00\x3f\x00")
    dc = [huffman_codes(*dc_tables[min(c, len(dc_tables) - 1)]) for c in range(nc)]
    ac = [huffman_codes(*ac_tables[min(c, len(ac_tables) - 1)]) for c in range(nc)]
    zz = [np.asarray(a, np.int64)[..., ZIGZAG].tolist() for a in coefs]
    mcux, mcuy = -(-W // (8 * hs)), -(-H // (8 * vs))
    bw, pred, rst = _Bits(), [0] * nc, 0
    for m in range(mcux * mcuy):
        my, mx = divmod(m, mcux)
        if restart and m and m % restart == 0:
            bw.flush()
            out += bw.out + fill + bytes([0xFF, 0xD0 + rst])
            rst = (rst + 1) & 7
            bw, pred = _Bits(), [0] * nc
        for c in range(nc):
            for by in range(samp[c][1]):
                for bx in range(samp[c][0]):
                    blk = zz[c][my * samp[c][1] + by][mx * samp[c][0] + bx]
                    _encode_block(bw, blk, pred[c], dc[c], ac[c])
                    pred[c] = blk[0]
    bw.flush()
    out += bw.out + b"\xff\xd9"
    if "trailing" in layout:
        out += b"\x00\x00trailing bytes\xff\xd8\xff"
    return bytes(out)


def segments(data):
    """(marker, payload) of every marker segment up to and including SOS; fill bytes in front of a marker are skipped"""
    out, p = [], 2
    assert data[:2] == b"\xff\xd8"
    while p < len(data):
        assert data[p] == 0xFF
        while data[p] == 0xFF:
            p += 1
        m, ln = data[p], (data[p + 1] << 8) | data[p + 2]
        out.append((m, bytes(data[p + 3:p + 1 + ln])))
        if m == 0xDA:
            break
        p += 1 + ln
    return out


def quant_tables(data):
    """natural-order quantisation tables per component, int64 [64], from the file's DQT (8- or 16-bit) and SOF segments"""
    tabs, comp_tq = {}, []
    for m, s in segments(data):
        if m == 0xDB:
            q = 0
            while q < len(s):
                wide = s[q] >> 4
                assert wide in (0, 1)
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(s[q + 1:q + 1 + 64 * (1 + wide)], ">u2" if wide else np.uint8)
                tabs[s[q] & 15] = t
                q += 1 + 64 * (1 + wide)
        elif m in (0xC0, 0xC1):
            comp_tq = [s[6 + 3 * i + 2] for i in range(s[5])]
    return [tabs[t] for t in comp_tq]


# ---- the long-code tables: every code length the decoders' lookup and slow paths can meet ---------------------------------------------------
# DC: one code at each of the lengths 1..11 and one of length 16 for the categories 0..11
DC_LONG = ([1] * 11 + [0, 0, 0, 0, 1], list(range(12)))
# AC: all 162 symbols (EOB, ZRL, run 0..15 x size 1..10): one code at each of the lengths 1..8 -- EOB, ZRL and the six symbols with the
# longest run and size -- and 154 of length 16, which leaves the all-ones code unused (2^8 - 1 = 255 free prefixes of length 16 > 154)
_AC_SYMBOLS = [r << 4 | s for s in range(1, 11) for r in range(16)]
AC_LONG = ([1] * 8 + [0] * 7 + [154], [0x00, 0xF0] + _AC_SYMBOLS[::-1])
assert len(AC_LONG[1]) == 162 == len(set(AC_LONG[1]))


# ---- reader of tests/golden/jpeg_streams.npz (oracle/make_jpeg_stream_goldens.py) ---------------------------------------------------------
class Streams:
    """the fixture: name -> file bytes, geometry, expected status, Pillow's pixels, the writer's coefficients"""

    def __init__(self, path):
        g = np.load(path, allow_pickle=False)
        self.names = [str(n) for n in g["names"]]
        self.index = {n: i for i, n in enumerate(self.names)}
        self.info = g["info"]
        self._blobs = {k: (g[k], g[k + "_off"]) for k in ("jpeg", "bgr", "coef")}

    def _part(self, kind, name):
        blob, off = self._blobs[kind]
        i = self.index[name]
        return blob[off[i]:off[i + 1]]

    def geometry(self, name):
        return tuple(int(v) for v in self.info[self.index[name]][:5])            # width, height, components, h_samp, v_samp

    def status(self, name):
        return int(self.info[self.index[name]][5])

    def data(self, name):
        return self._part("jpeg", name).tobytes()

    def bgr(self, name):
        W, H = self.geometry(name)[:2]
        return self._part("bgr", name).reshape(H, W, 3)

    def coefficients(self, name):
        """the coefficients the writer was given, per component [bh, bw, 64]; None for a Pillow-made file"""
        flat = self._part("coef", name)
        if not flat.size:
            return None
        W, H, nc, hs, vs = self.geometry(name)
        mx, my = -(-W // (8 * hs)), -(-H // (8 * vs))
        out, o = [], 0
        for bh, bw in [(my * vs, mx * hs)] + [(my, mx)] * (nc - 1):
            out.append(flat[o:o + bh * bw * 64].reshape(bh, bw, 64))
            o += bh * bw * 64
        assert o == flat.size
        return out

    def family(self, *prefixes):
        return [n for n in self.names if n.split("/")[0] in prefixes]

    def decodable(self):
        return [n for n in self.names if self.status(n) == 0]


_loaded = {}


def streams(path):
    """the fixture at `path`, loaded once per process"""
    if path not in _loaded:
        _loaded[path] = Streams(path)
    return _loaded[path]
