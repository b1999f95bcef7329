// N3 JPEG decode: what jpeg.hip (one file per call, host Huffman walk) and jpeg_batch.hip (a batch per call, device Huffman walk) share --
// the marker parser up to SOS, the per-image geometry the pixel kernels read, and libjpeg's islow IDCT / fancy upsampling / colour
// conversion as __device__ functions (the arithmetic notes are in jpeg.hip's head comment).
#pragma once
#include <stddef.h>

#include <hip/hip_runtime.h>

namespace capf {

struct JpegComp { int id, h, v, tq, td, ta; int bw, bh; size_t coef_off; int pw, ph; size_t plane_off; };   // bw / bh: blocks; pw / ph: plane size in samples
struct JpegHeader {
    int W = 0, H = 0, nc = 0, hmax = 1, vmax = 1, mcux = 0, mcuy = 0, restart = 0;
    JpegComp c[3];
    unsigned short qt[4][64];
    bool have_qt[4] = {false, false, false, false};
    unsigned char bits[2][4][17], vals[2][4][256];
    bool have_ht[2][4] = {{false, false, false, false}, {false, false, false, false}};
    size_t scan_off = 0;              // first byte of the entropy-coded segment
    size_t coef_elems = 0, plane_bytes = 0;
};

static const unsigned char kZigzag[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// marker segments up to and including SOS; CAPF_OK / CAPF_ERR_INVALID (not a JPEG, truncated) / CAPF_ERR_UNSUPPORTED (a JPEG this path does not decode)
int jpeg_parse(const unsigned char* d, size_t n, JpegHeader& h);

struct JpegDev {
    int W, H, nc, hmax, vmax;
    int bw[3], bh[3], pw[3], ph[3], dw[3], dh[3];      // blocks, plane size, true ("downsampled") size of each component
    long coef_off[3], plane_off[3];
    unsigned short qt[3][64];
    // crop-aware route (jpeg_batch.hip) only, 0 elsewhere: the planes hold the image from luma pixel (pox, poy) on -- whole MCUs, bw / bh /
    // pw / ph are the patch's -- and the output buffer from pixel (ox, oy) on.  W, H, dw, dh stay the image's: edges are image edges.
    int pox, poy, ox, oy;
};

// the pixel kernels' view of a parsed header
inline JpegDev jpeg_dev(const JpegHeader& h) {
    JpegDev jd{};
    jd.W = h.W; jd.H = h.H; jd.nc = h.nc; jd.hmax = h.hmax; jd.vmax = h.vmax;
    for (int i = 0; i < h.nc; ++i) {
        const JpegComp& c = h.c[i];
        jd.bw[i] = c.bw; jd.bh[i] = c.bh; jd.pw[i] = c.pw; jd.ph[i] = c.ph;
        jd.dw[i] = (h.W * c.h + h.hmax - 1) / h.hmax; jd.dh[i] = (h.H * c.v + h.vmax - 1) / h.vmax;
        jd.coef_off[i] = (long)c.coef_off; jd.plane_off[i] = (long)c.plane_off;
        for (int k = 0; k < 64; ++k) jd.qt[i][k] = h.qt[c.tq][k];
    }
    return jd;
}

// jidctint.c jpeg_idct_islow on block b of component comp (dequantised here); samples into the component's plane
__device__ __forceinline__ void jpeg_idct_block(const short* __restrict__ coef, unsigned char* __restrict__ planes, const JpegDev& jd, int comp, int b) {
    constexpr int CB = 13, P1 = 2;
    constexpr long F0298 = 2446, F0390 = 3196, F0541 = 4433, F0765 = 6270, F0899 = 7373, F1175 = 9633, F1501 = 12299, F1847 = 15137, F1961 = 16069,
                   F2053 = 16819, F2562 = 20995, F3072 = 25172;
    const short* in = coef + jd.coef_off[comp] + (long)b * 64;
    const unsigned short* q = jd.qt[comp];
    long ws[64];
    auto pass = [&](const long v[8], long o[8], int shift) {
        long z2 = v[2], z3 = v[6];
        long z1 = (z2 + z3) * F0541;
        long tmp2 = z1 + z3 * (-F1847), tmp3 = z1 + z2 * F0765;
        z2 = v[0]; z3 = v[4];
        long tmp0 = (z2 + z3) << CB, tmp1 = (z2 - z3) << CB;
        const long tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
        tmp0 = v[7]; tmp1 = v[5]; tmp2 = v[3]; tmp3 = v[1];
        z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
        long z4 = tmp1 + tmp3;
        const long z5 = (z3 + z4) * F1175;
        tmp0 *= F0298; tmp1 *= F2053; tmp2 *= F3072; tmp3 *= F1501;
        z1 *= -F0899; z2 *= -F2562; z3 *= -F1961; z4 *= -F0390;
        z3 += z5; z4 += z5;
        tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
        const long r = 1L << (shift - 1);
        o[0] = (tmp10 + tmp3 + r) >> shift; o[7] = (tmp10 - tmp3 + r) >> shift;
        o[1] = (tmp11 + tmp2 + r) >> shift; o[6] = (tmp11 - tmp2 + r) >> shift;
        o[2] = (tmp12 + tmp1 + r) >> shift; o[5] = (tmp12 - tmp1 + r) >> shift;
        o[3] = (tmp13 + tmp0 + r) >> shift; o[4] = (tmp13 - tmp0 + r) >> shift;
    };
    for (int c = 0; c < 8; ++c) {                      // pass 1: columns (the all-zero-AC shortcut of the C code gives the same numbers)
        long v[8], o[8];
        for (int r = 0; r < 8; ++r) v[r] = (long)in[r * 8 + c] * (long)q[r * 8 + c];
        pass(v, o, CB - P1);
        for (int r = 0; r < 8; ++r) ws[r * 8 + c] = o[r];
    }
    const int by = b / jd.bw[comp], bx = b - by * jd.bw[comp];
    unsigned char* dst = planes + jd.plane_off[comp] + (long)(by * 8) * jd.pw[comp] + bx * 8;
    for (int r = 0; r < 8; ++r) {                      // pass 2: rows, + 128, clamp
        long o[8];
        pass(ws + r * 8, o, CB + P1 + 3);
        unsigned long long pk = 0;
        for (int c = 0; c < 8; ++c) {
            // range_limit[x & RANGE_MASK] of jdmaster.c prepare_range_limit_table: the 10-bit masked index selects, in order, [0, 127] -> x + 128,
            // [128, 511] -> 255, [512, 895] -> 0, [896, 1023] -> x - 1024 + 128 (i.e. the clamp of x + 128 for every x in [-512, 511])
            const int x = (int)(o[c] & 1023);
            const int sv = x < 128 ? x + 128 : (x < 512 ? 255 : (x < 896 ? 0 : x - 896));
            pk |= (unsigned long long)sv << (8 * c);
        }
        *reinterpret_cast<unsigned long long*>(dst + (long)r * jd.pw[comp]) = pk;
    }
}

// chroma sample at full resolution: jdsample.c fullsize / h2v1_fancy / h2v2_fancy with libjpeg's edge handling (context rows replicated at the
// top and below the component's last true row; first / last column special-cased).  jinit_upsampler picks the fancy routines only for a
// component with downsampled_width > 2; a narrower one goes through h2v1_upsample / h2v2_upsample, which replicate each sample -- no
// filter along either axis, no context row.
__device__ __forceinline__ int jpeg_chroma(const unsigned char* pl, int pw, int dw, int dh, int hs, int vs, int x, int y, int cox, int coy) {
    // (x, y): image coordinates, which the edge rules are about; pl holds the plane from chroma sample (cox, coy) on
    if (hs == 1 && vs == 1) return pl[(long)(y - coy) * pw + (x - cox)];
    if (dw <= 2) return pl[(long)(y / vs - coy) * pw + (x / hs - cox)];
    const int cx = x >> 1, odd = x & 1, lx = cx - cox;
    if (vs == 1) {                                      // h2v1
        const unsigned char* r = pl + (long)(y - coy) * pw;
        const int v = r[lx];
        if (!odd) return cx == 0 ? v : (v * 3 + r[lx - 1] + 1) >> 2;
        return cx == dw - 1 ? v : (v * 3 + r[lx + 1] + 2) >> 2;
    }
    const int cy = y >> 1;                              // h2v2: nearer row cy, farther row cy -/+ 1
    const int fy = min(max((y & 1) ? cy + 1 : cy - 1, 0), dh - 1);
    const unsigned char* r0 = pl + (long)(cy - coy) * pw;
    const unsigned char* r1 = pl + (long)(fy - coy) * pw;
    const int cur = r0[lx] * 3 + r1[lx];
    if (!odd) {
        if (cx == 0) return (cur * 4 + 8) >> 4;
        return (cur * 3 + (r0[lx - 1] * 3 + r1[lx - 1]) + 8) >> 4;
    }
    if (cx == dw - 1) return (cur * 4 + 7) >> 4;
    return (cur * 3 + (r0[lx + 1] * 3 + r1[lx + 1]) + 7) >> 4;
}

// pixel (x, y) of the image: upsampling + YCbCr -> BGR
__device__ __forceinline__ void jpeg_color_pixel(const unsigned char* __restrict__ planes, unsigned char* __restrict__ out, const JpegDev& jd, long out_pitch,
                                                 int x, int y) {
    const int Y = planes[jd.plane_off[0] + (long)(y - jd.poy) * jd.pw[0] + (x - jd.pox)];
    int r = Y, g = Y, b = Y;
    if (jd.nc == 3) {
        const int cox = jd.pox / jd.hmax, coy = jd.poy / jd.vmax;
        const int cb = jpeg_chroma(planes + jd.plane_off[1], jd.pw[1], jd.dw[1], jd.dh[1], jd.hmax, jd.vmax, x, y, cox, coy) - 128;
        const int cr = jpeg_chroma(planes + jd.plane_off[2], jd.pw[2], jd.dw[2], jd.dh[2], jd.hmax, jd.vmax, x, y, cox, coy) - 128;
        // jdcolor.c build_ycc_rgb_table, SCALEBITS 16: FIX(1.40200) = 91881, FIX(1.77200) = 116130, FIX(0.71414) = 46802, FIX(0.34414) = 22554
        r = Y + ((91881 * cr + 32768) >> 16);
        b = Y + ((116130 * cb + 32768) >> 16);
        g = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16);
        r = min(max(r, 0), 255); g = min(max(g, 0), 255); b = min(max(b, 0), 255);
    }
    unsigned char* o = out + (long)(y - jd.oy) * out_pitch + 3L * (x - jd.ox);
    o[0] = (unsigned char)b; o[1] = (unsigned char)g; o[2] = (unsigned char)r;
}

}  // namespace capf
