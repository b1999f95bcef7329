// N3 batched JPEG decode: the entropy decoder as __host__ __device__ code, shared by the GPU kernels (jpeg_batch.hip) and their serial
// CPU emulation (capf_jpeg_coefficients_subseq), so that one set of rules is tested on the build host and run on the MI355X.
//
// Self-synchronising subsequence decoding (Weissenberger & Schmidt, ICPP 2018): a SEGMENT (one restart interval, or the whole scan) is
// unstuffed into a plain bit stream and cut into subsequences of L bytes, one lane each.  A decode state is (bit position, block index in
// the MCU, coefficient index k); lane j's EXIT is the state at the first symbol boundary at or after its subsequence end.  Lane 0 starts
// from the true state, every other lane from a guess (its boundary, block 0, k 0).  Round r re-decodes lane j from lane j-1's exit of
// round r-1 (E_r[j] = f_j(E_{r-1}[j-1])), so lanes 0..r are exact after round r, and a lane whose entry did not change since the round
// before is copied, not decoded.  Huffman codes resynchronise within a few symbols, so nearly every segment reaches the fixed point
// (E_r == E_{r-1}, which only the true exits satisfy) in one or two rounds.  After the last round one lane per segment walks the lanes and
// re-decodes, serially, every lane whose entry is not proven -- results never depend on convergence.
//
// The per-symbol rules are those of jpeg.hip's host decoder (jpeg_entropy_decode, the oracle), odd streams included: an invalid code
// consumes 16 bits and yields symbol 0; a DC category > 11 or an AC size > 10 is an error; a run past k = 63 ends the block.
#pragma once
#include <hip/hip_runtime.h>

namespace capf {

// one Huffman table: jpeg.hip HuffTab's 9-bit lookup + canonical slow path, as a flat struct that can be copied to the device / LDS
struct JbHuff {
    int maxcode[18], valptr[17];
    unsigned char look_n[512], look_v[512], vals[256];
};

inline void jb_huff_build(JbHuff& t, const unsigned char* bits, const unsigned char* v) {
    int code = 0, k = 0;
    unsigned short codes[256];
    unsigned char sizes[256];
    for (int l = 1; l <= 16; ++l) {
        t.valptr[l] = k - code;
        for (int i = 0; i < bits[l]; ++i) { codes[k] = (unsigned short)code; sizes[k] = (unsigned char)l; ++k; ++code; }
        t.maxcode[l] = bits[l] ? code - 1 : -1;
        code <<= 1;
    }
    t.maxcode[0] = -1; t.valptr[0] = 0; t.maxcode[17] = 0x7FFFFFFF;
    for (int i = 0; i < 512; ++i) { t.look_n[i] = 0; t.look_v[i] = 0; }
    for (int i = 0; i < 256; ++i) t.vals[i] = i < k ? v[i] : 0;
    for (int i = 0; i < k; ++i)
        if (sizes[i] <= 9) {
            const int base = codes[i] << (9 - sizes[i]);
            for (int j = 0; j < (1 << (9 - sizes[i])); ++j) { t.look_n[base + j] = sizes[i]; t.look_v[base + j] = v[i]; }
        }
}

// what the entropy decoder needs of one image's interleaved scan.  tabs[ci] = DC table of component ci, tabs[3 + ci] its AC table.
struct JbScan {
    int bpm;                          // blocks per MCU (1, 3, 4 or 6)
    int mcux, mcus;                   // MCUs per row, in the image
    int restart;                      // MCUs per segment (the DRI interval; = mcus without one)
    int nseg;                         // segments = ceil(mcus / restart)
    long coef_elems;
    unsigned char bci[6], bby[6], bbx[6];   // block of the MCU -> component, row and column inside the MCU
    int ch[3], cv[3], cbw[3];
    long coef_off[3];
    unsigned char zz[64];             // zigzag -> natural order
};

// exit state of a lane.  err: the decode met a DC category > 11 or an AC size > 10 (and stopped there).
// changed: this round's exit differs from the round before (set for every lane by the first pass).
struct JbState {
    int pos;                          // bit position in the segment
    int nblk;                         // blocks completed between the lane's entry and its exit
    int first;                        // segment-relative index of the block in progress at the lane's entry (written by the scan)
    unsigned char b, k, err, changed;
};

__host__ __device__ inline bool jb_same(const JbState& a, const JbState& b) {
    return a.pos == b.pos && a.b == b.b && a.k == b.k && a.err == b.err;
}

// 32 bits of the segment from bit `pos` on, MSB first; bytes at or past nbytes read as zero (the host reader's zeros after a marker)
__host__ __device__ inline unsigned jb_bits32(const unsigned char* d, int nbytes, int pos) {
    const int i = pos >> 3, sh = pos & 7;
    unsigned long long v = 0;
    for (int t = 0; t < 5; ++t) v = (v << 8) | (unsigned)(i + t < nbytes ? d[i + t] : 0);
    return (unsigned)(v >> (8 - sh));
}

__host__ __device__ inline int jb_huff(const JbHuff& t, unsigned w, int& len) {
    const unsigned look = w >> 23;
    if (t.look_n[look]) { len = t.look_n[look]; return t.look_v[look]; }
    const int code = (int)(w >> 16);
    for (int l = 10; l <= 16; ++l) {
        const int c = code >> (16 - l);
        if (c <= t.maxcode[l]) { len = l; return t.vals[(t.valptr[l] + c) & 255]; }
    }
    len = 16;                                          // corrupt stream: skip 16 bits, symbol 0
    return 0;
}

__host__ __device__ inline int jb_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// offset of block `blk` (decode order, relative to MCU mcu0) in the coefficient layout of capf_jpeg_coefficients
__host__ __device__ inline long jb_block_offset(const JbScan& sc, int mcu0, int blk) {
    const int m = mcu0 + blk / sc.bpm, bm = blk - (blk / sc.bpm) * sc.bpm;
    const int my = m / sc.mcux, mx = m - my * sc.mcux, ci = sc.bci[bm];
    return sc.coef_off[ci] + ((long)(my * sc.cv[ci] + sc.bby[bm]) * sc.cbw[ci] + (mx * sc.ch[ci] + sc.bbx[bm])) * 64;
}

// crop-aware route: which MCUs of the image are kept, and the compact coefficient layout over them -- component after component, blocks
// [rows][cols][64] over the MCU rectangle, i.e. capf_jpeg_coefficients' layout of an image that is just the rectangle
struct JbCrop {
    int mcu[4];                       // kept MCUs [mx0, my0, mx1, my1); empty when the crop reads no pixel of the image
    int rect[4];                      // the pixels the warp reads, [x0, y0, x1, y1), inside those MCUs
    long coef_off[3];
    int cbw[3];                       // blocks per row of the rectangle, per component
    long coef_elems;
    short* dc;                        // [mcus * bpm] every block's DC difference, decode order, rectangle or not
    double m[6];                      // the crop's forward matrix
};

// offset of block `blk` in the rectangle's coefficient layout, -1 for a block outside the rectangle
__host__ __device__ inline long jb_crop_offset(const JbScan& sc, const JbCrop& cr, int mcu0, int blk) {
    const int m = mcu0 + blk / sc.bpm, bm = blk - (blk / sc.bpm) * sc.bpm;
    const int my = m / sc.mcux, mx = m - my * sc.mcux, ci = sc.bci[bm];
    if (mx < cr.mcu[0] || mx >= cr.mcu[2] || my < cr.mcu[1] || my >= cr.mcu[3]) return -1;
    const long off = cr.coef_off[ci] + ((long)((my - cr.mcu[1]) * sc.cv[ci] + sc.bby[bm]) * cr.cbw[ci] + ((mx - cr.mcu[0]) * sc.ch[ci] + sc.bbx[bm])) * 64;
    return off >= 0 && off + 64 <= cr.coef_elems ? off : -1;
}

// Decodes the symbols that START before bit `end` from state st (pos, b, k), stopping early once max_blocks blocks are complete.  The
// count goes to st.nblk.  WRITE: coefficients of block st.first + (completed blocks) while that is < max_blocks -- AC at natural
// positions, the DC DIFFERENCE at [0] (jb_dc_values turns differences into values).  Loops are bounded by the bit position (every
// symbol consumes at least one bit) and by max_blocks; writes by the image's coefficient count.
// WRITE = JB_WRITE_CROP (crop-aware route; `coef` is the rectangle's compact buffer): the DC difference of EVERY block goes to crop->dc
// [mcu0 * bpm + block] -- a block's DC value needs all differences before it in the segment --, AC only for blocks inside the rectangle.
enum { JB_COUNT = 0, JB_WRITE = 1, JB_WRITE_CROP = 2 };
template <int WRITE>
__host__ __device__ inline void jb_run(const unsigned char* d, int nbytes, int end, int max_blocks, const JbHuff* tabs, const JbScan& sc, JbState& st,
                                       short* coef, int mcu0, const JbCrop* crop = nullptr) {
    int pos = st.pos, b = st.b, k = st.k, n = 0;
    st.nblk = 0;
    if (st.err) return;
    short* blk = nullptr;
    short* dcp = nullptr;             // JB_WRITE_CROP: where this block's DC difference goes; null past the segment's last block
    auto locate = [&]() {
        const int g = st.first + n;
        blk = nullptr;
        dcp = nullptr;
        if (g >= 0 && g < max_blocks) {
            if (WRITE == JB_WRITE_CROP) {
                dcp = crop->dc + ((long)mcu0 * sc.bpm + g);
                const long off = jb_crop_offset(sc, *crop, mcu0, g);
                if (off >= 0) blk = coef + off;
            } else {
                const long off = jb_block_offset(sc, mcu0, g);
                if (off >= 0 && off + 64 <= sc.coef_elems) blk = coef + off;
            }
        }
    };
    if (WRITE) locate();
    while (pos < end && n < max_blocks) {
        if (WRITE == JB_WRITE && !blk) break;
        if (WRITE == JB_WRITE_CROP && !dcp) break;
        const int ci = sc.bci[b];
        int len;
        if (k == 0) {
            const int s = jb_huff(tabs[ci], jb_bits32(d, nbytes, pos), len);
            if (s > 11) { st.err = 1; break; }         // (8-bit baseline: DC differences have at most 11 magnitude bits)
            pos += len;
            int diff = 0;
            if (s) { diff = jb_extend((int)(jb_bits32(d, nbytes, pos) >> (32 - s)), s); pos += s; }
            if (WRITE == JB_WRITE) blk[0] = (short)diff;
            if (WRITE == JB_WRITE_CROP) *dcp = (short)diff;
            k = 1;
            continue;
        }
        const int rs = jb_huff(tabs[3 + ci], jb_bits32(d, nbytes, pos), len);
        pos += len;
        const int r = rs >> 4, sz = rs & 15;
        if (sz == 0) {
            k = r != 15 ? 64 : k + 16;                 // EOB / ZRL
        } else {
            k += r;
            if (k > 63) {
                k = 64;
            } else {
                if (sz > 10) { st.err = 1; break; }
                const int v = jb_extend((int)(jb_bits32(d, nbytes, pos) >> (32 - sz)), sz);
                pos += sz;
                if (WRITE == JB_WRITE || (WRITE == JB_WRITE_CROP && blk)) blk[sc.zz[k]] = (short)v;
                ++k;
            }
        }
        if (k >= 64) {
            k = 0;
            b = b + 1 == sc.bpm ? 0 : b + 1;
            ++n;
            if (WRITE) locate();
        }
    }
    st.pos = pos; st.b = (unsigned char)b; st.k = (unsigned char)k; st.nblk = n;
}

// ---- one segment, as the kernels and the emulation see it --------------------------------------------------------------------------
struct JbSeg {
    const unsigned char* d;           // unstuffed bytes
    int nbytes;
    int nlanes;                       // max(1, ceil(nbytes / L))
    int nblocks;                      // blocks the segment must hold: (MCUs in it) * bpm
    int mcu0;                         // its first MCU
};

__host__ __device__ inline int jb_lane_end(const JbSeg& s, int L, int j) {
    const long e = (long)(j + 1) * L * 8, bits = (long)s.nbytes * 8;
    return (int)(j + 1 == s.nlanes || e > bits ? bits : e);
}

// first pass: lane j from its guessed entry
__host__ __device__ inline void jb_lane_init(const JbSeg& s, int L, int j, const JbHuff* tabs, const JbScan& sc, JbState& out) {
    out.pos = j * L * 8; out.b = 0; out.k = 0; out.err = 0; out.first = 0;
    jb_run<JB_COUNT>(s.d, s.nbytes, jb_lane_end(s, L, j), s.nblocks, tabs, sc, out, nullptr, 0);
    out.changed = 1;
}

// one sync round: dst[j] from src[j-1] (lane j-1's previous exit); a lane whose entry did not change is copied
__host__ __device__ inline void jb_lane_round(const JbSeg& s, int L, int j, const JbHuff* tabs, const JbScan& sc, const JbState* src, JbState* dst) {
    JbState e = src[j];
    if (j == 0 || !src[j - 1].changed) {
        e.changed = 0;
    } else {
        e = src[j - 1];
        e.first = 0;
        jb_run<JB_COUNT>(s.d, s.nbytes, jb_lane_end(s, L, j), s.nblocks, tabs, sc, e, nullptr, 0);
        e.changed = !jb_same(e, src[j]);
    }
    dst[j] = e;
}

// the correctness net, one lane per segment: lanes before j0 (the first lane whose exit changed in the last round) hold true exits; from
// there on a lane keeps its stored exit only if it was decoded from its predecessor's true exit, and is re-decoded serially otherwise
__host__ __device__ inline void jb_lane_fallback(const JbSeg& s, int L, int j0, const JbHuff* tabs, const JbScan& sc, JbState* st) {
    if (j0 >= s.nlanes) return;
    JbState v = st[j0];                                // exit of lane j0: decoded from lane j0-1's unchanged, true exit
    bool proven = false;                               // (lane j0 changed, so lane j0+1's stored exit came from another entry)
    for (int j = j0 + 1; j < s.nlanes; ++j) {
        const JbState old = st[j];
        JbState t = old;
        if (!proven) {
            t = v;
            t.first = 0;
            jb_run<JB_COUNT>(s.d, s.nbytes, jb_lane_end(s, L, j), s.nblocks, tabs, sc, t, nullptr, 0);
            t.changed = 0;
            st[j] = t;
        }
        proven = jb_same(old, t) && !old.changed;      // then lane j's previous exit was true too, and lane j+1's stored exit follows from it
        v = t;
    }
}

// DC differences -> values for the blocks [b0, b1) of a segment in decode order; pred[ci] enters holding the running sum before b0
__host__ __device__ inline void jb_dc_values(const JbScan& sc, int mcu0, int b0, int b1, int pred[3], short* coef, bool write) {
    for (int g = b0; g < b1; ++g) {
        const int bm = g % sc.bpm, ci = sc.bci[bm];
        const long off = jb_block_offset(sc, mcu0, g);
        if (off < 0 || off + 64 > sc.coef_elems) continue;
        pred[ci] += coef[off];
        if (write) coef[off] = (short)pred[ci];
    }
}

// the same for the crop-aware route: sums over crop.dc (every block of the segment), values stored only where the block is kept
__host__ __device__ inline void jb_dc_values_crop(const JbScan& sc, const JbCrop& cr, int mcu0, int b0, int b1, int pred[3], short* coef, bool write) {
    for (int g = b0; g < b1; ++g) {
        const int bm = g % sc.bpm, ci = sc.bci[bm];
        pred[ci] += cr.dc[(long)mcu0 * sc.bpm + g];
        if (!write) continue;
        const long off = jb_crop_offset(sc, cr, mcu0, g);
        if (off >= 0) coef[off] = (short)pred[ci];
    }
}

// status bits of capf_jpeg_decode_batch (include/capf.h)
enum { JB_ERR_SIZE = 1, JB_ERR_BLOCKS = 2, JB_ERR_RESTART = 4 };

// the marker rules of jpeg.hip's BitReader, byte by byte: a byte is DATA unless it is an FF that does not stand before 00 (a marker, a fill
// byte, a lone FF at the end) or follows an FF (the 00 of a stuffed FF, a marker code)
__host__ __device__ inline bool jb_keep(const unsigned char* d, long n, long i) {
    return d[i] == 0xFF ? (i + 1 < n && d[i + 1] == 0) : !(i > 0 && d[i - 1] == 0xFF);
}
__host__ __device__ inline bool jb_marker(const unsigned char* d, long n, long i) { return d[i] == 0xFF && !(i + 1 < n && d[i + 1] == 0); }
__host__ __device__ inline bool jb_rst(const unsigned char* d, long n, long i) {
    return d[i] == 0xFF && i + 1 < n && d[i + 1] >= 0xD0 && d[i + 1] <= 0xD7;
}
__host__ __device__ inline bool jb_eoi(const unsigned char* d, long n, long i) { return d[i] == 0xFF && i + 1 < n && d[i + 1] == 0xD9; }

}  // namespace capf
