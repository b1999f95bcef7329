// N3, batched: capf_jpeg_decode_batch decodes a batch of baseline JPEG files in one call with the entropy decode on the GPU too (jpeg.hip's
// capf_jpeg_decode walks the Huffman stream of one file on the host).  The output bits are those of capf_jpeg_decode: the same symbol
// rules (jpeg_sync.h, shared with the CPU emulation capf_jpeg_coefficients_subseq) and the same pixel arithmetic (jpeg.h).
//
// One call = one H2D copy of [image descriptors | work tables | raw entropy bytes], then, all on the stream:
//   jb_unstuff_kernel   one workgroup per image: FF 00 stuffing out, RSTn / other markers found, segment table + lanes per segment;
//   jb_lane_kernel      one lane per L-byte subsequence, workgroups = (image, run of 256 lanes) with that image's Huffman tables in LDS:
//                       first pass from guessed states, kJbRounds sync rounds, and at the end the write pass;
//   jb_seg_kernel       one workgroup per segment: the serial fallback for lanes still unproven, the block scan (each lane's first
//                       block), the block-count / error checks;
//   jb_dc_kernel        one workgroup per segment: DC differences -> values per component;
//   jb_idct_kernel, jb_color_kernel: one grid over all blocks / pixels of all images.
//
// capf_jpeg_decode_crop_batch is the same up to jb_seg_kernel, for a caller that only wants an affine crop of each file (warp_rule.h says
// which pixels that reads): the write pass keeps the AC coefficients of the MCUs around those pixels only, in a compact buffer, and every
// block's DC difference (a DC value needs all differences before it in the segment); IDCT and colour run over that rectangle into a
// BGR patch, and jb_warp_crop_kernel samples the patch with the image's border.  No full-frame buffer exists on that route.
// No kernel waits on another workgroup; the host never reads anything back.  A corrupt file sets its status word, the others are unaffected.
#include <string.h>

#include <algorithm>
#include <vector>

#include "capf.h"
#include "jpeg.h"
#include "jpeg_sync.h"
#include "kernels.h"
#include "warp_rule.h"

namespace capf {

// default subsequence length in bytes, measured (EXPERIMENTS R7.2, 64 frames of 1000 x 1002 4:2:0 at q75 / q90, ms per batch):
// L = 16: 98.6 / 212; 64: 25.1 / 55.2; 128: 8.2 / 14.5; 256: 6.0 / 8.3; 512: 7.3 / 8.8; 1024: 9.8 / 12.4.  Shorter lanes leave the
// block-in-MCU index unsynchronised for the serial fallback; longer ones lengthen each lane's serial decode.
constexpr int kJbSubseqDefault = 256;
constexpr int kJbRounds = 3;                     // sync rounds before the serial fallback
constexpr int kJbLanesPerWg = 256;

struct JbTables { JbScan sc; JbHuff tabs[6]; };

struct JbImage {
    JbTables t;
    JpegDev jd;
    const unsigned char* raw;            // entropy-coded bytes (SOS payload to the end of the file)
    unsigned char* bytes;                // unstuffed
    int* seg;                            // [nseg] start, [nseg] end (unstuffed byte offsets), [nseg + 1] lane offsets
    JbState* st[2];
    short* coef;
    unsigned char* planes;
    unsigned char* out;
    long pitch;
    int* status;
    int raw_len, lane_bound, L, nblocks_idct;
    JbCrop cr;                           // crop-aware route only: there jd, coef, planes and out (the BGR patch) are the rectangle's
};

// host side of one file: parsed header, decoder tables, sizes
struct JbPrep {
    JpegHeader h;
    JbTables t;
    const unsigned char* raw = nullptr;
    int raw_len = 0, lane_bound = 0;
    bool crop = false;                   // crop-aware route: the rectangle, its geometry (jd) and its buffer sizes
    JbCrop cr{};
    JpegDev jd{};
    size_t crop_plane_bytes = 0, patch_pitch = 0, patch_bytes = 0;
};

static int jb_prepare(const unsigned char* d, size_t n, int L, JbPrep& p) {
    if (!d) return CAPF_ERR_INVALID;
    const int rc = jpeg_parse(d, n, p.h);
    if (rc != CAPF_OK) return rc;
    const JpegHeader& h = p.h;
    if (n - h.scan_off >= (size_t)1 << 27) return CAPF_ERR_UNSUPPORTED;        // (bit positions are int32)
    JbScan& sc = p.t.sc;
    memset(&sc, 0, sizeof(sc));
    for (int ci = 0; ci < h.nc; ++ci) {
        const JpegComp& c = h.c[ci];
        for (int by = 0; by < c.v; ++by)
            for (int bx = 0; bx < c.h; ++bx) { sc.bci[sc.bpm] = (unsigned char)ci; sc.bby[sc.bpm] = (unsigned char)by; sc.bbx[sc.bpm] = (unsigned char)bx; ++sc.bpm; }
        sc.ch[ci] = c.h; sc.cv[ci] = c.v; sc.cbw[ci] = c.bw; sc.coef_off[ci] = (long)c.coef_off;
        jb_huff_build(p.t.tabs[ci], h.bits[0][c.td], h.vals[0][c.td]);
        jb_huff_build(p.t.tabs[3 + ci], h.bits[1][c.ta], h.vals[1][c.ta]);
    }
    sc.mcux = h.mcux;
    sc.mcus = h.mcux * h.mcuy;
    sc.restart = h.restart ? h.restart : sc.mcus;
    sc.nseg = (sc.mcus + sc.restart - 1) / sc.restart;
    sc.coef_elems = (long)h.coef_elems;
    memcpy(sc.zz, kZigzag, 64);
    p.raw = d + h.scan_off;
    p.raw_len = (int)(n - h.scan_off);
    p.lane_bound = p.raw_len / L + sc.nseg + 1;          // >= sum over segments of max(1, ceil(bytes / L))
    return CAPF_OK;
}

// crop-aware route: the source rectangle of crop matrix m (warp_rule.h), its MCUs, and the pixel kernels' geometry over those MCUs alone
static void jb_prepare_crop(JbPrep& p, const double* m, int out_w, int out_h) {
    const JpegHeader& h = p.h;
    JbCrop& cr = p.cr;
    p.crop = true;
    memset(&cr, 0, sizeof(cr));
    memcpy(cr.m, m, sizeof(cr.m));
    warp_source_rect(h.W, h.H, m, out_w, out_h, cr.rect);
    warp_mcu_rect(h.W, h.H, h.hmax, h.vmax, cr.rect, cr.mcu);
    const int rw = cr.mcu[2] - cr.mcu[0], rh = cr.mcu[3] - cr.mcu[1];
    p.jd = jpeg_dev(h);
    size_t co = 0, po = 0;
    for (int i = 0; i < h.nc; ++i) {
        const JpegComp& c = h.c[i];
        p.jd.bw[i] = rw * c.h; p.jd.bh[i] = rh * c.v; p.jd.pw[i] = p.jd.bw[i] * 8; p.jd.ph[i] = p.jd.bh[i] * 8;
        p.jd.coef_off[i] = cr.coef_off[i] = (long)co; co += (size_t)p.jd.bw[i] * p.jd.bh[i] * 64;
        p.jd.plane_off[i] = (long)po; po += (size_t)p.jd.pw[i] * p.jd.ph[i];
        cr.cbw[i] = p.jd.bw[i];
    }
    cr.coef_elems = (long)co;
    p.crop_plane_bytes = (po + 15) & ~(size_t)15;
    p.jd.pox = cr.mcu[0] * 8 * h.hmax; p.jd.poy = cr.mcu[1] * 8 * h.vmax;
    p.jd.ox = cr.rect[0]; p.jd.oy = cr.rect[1];
    p.patch_pitch = 3 * (size_t)(cr.rect[2] - cr.rect[0]);
    p.patch_bytes = (p.patch_pitch * (cr.rect[3] - cr.rect[1]) + 15) & ~(size_t)15;
}

__host__ __device__ static inline JbSeg jb_segment(const JbScan& sc, const unsigned char* bytes, const int* seg, int s) {
    const int* end = seg + sc.nseg;
    const int* lane_off = end + sc.nseg;
    JbSeg g;
    g.d = bytes + seg[s];
    g.nbytes = end[s] - seg[s];
    g.nlanes = lane_off[s + 1] - lane_off[s];
    g.mcu0 = s * sc.restart;
    g.nblocks = ((g.mcu0 + sc.restart < sc.mcus ? g.mcu0 + sc.restart : sc.mcus) - g.mcu0) * sc.bpm;
    return g;
}

// ---- serial CPU emulation of the device algorithm (capf_jpeg_coefficients_subseq) ---------------------------------------------------
static int jb_emulate(const JbPrep& p, int L, short* coef) {
    const JbScan& sc = p.t.sc;
    const JbHuff* tabs = p.t.tabs;
    const unsigned char* d = p.raw;
    const long n = p.raw_len;
    const int S = sc.nseg;
    int status = 0;
    // unstuff + segment table (jb_unstuff_kernel's rules)
    long eoi = n;
    for (long i = 0; i < n; ++i)
        if (jb_eoi(d, n, i)) { eoi = i; break; }
    std::vector<unsigned char> bytes(std::max(n, 1L));
    std::vector<int> seg(3 * S + 1, 0);
    int* start = seg.data();
    int* end = start + S;
    int* lane_off = end + S;
    long kept = 0;
    for (long i = 0; i < n; ++i) kept += jb_keep(d, n, i);
    for (int j = 1; j < S; ++j) start[j] = (int)kept;
    int c = 0, q = 0;
    for (long i = 0; i < n; ++i) {
        if (i < eoi && jb_rst(d, n, i)) { if (q < S - 1) start[q + 1] = c; ++q; }
        if (jb_keep(d, n, i)) bytes[c++] = d[i];
    }
    if (q != S - 1) status |= JB_ERR_RESTART;
    for (int j = 0; j < S; ++j) end[j] = j + 1 < S ? start[j + 1] : (int)kept;
    c = 0; q = 0;
    for (long i = 0; i < n; ++i) {
        if (i <= eoi && jb_marker(d, n, i) && !jb_rst(d, n, i)) { const int s = std::min(q, S - 1); end[s] = std::min(end[s], c); }
        if (i < eoi && jb_rst(d, n, i)) ++q;
        c += jb_keep(d, n, i);
    }
    lane_off[0] = 0;
    for (int j = 0; j < S; ++j) lane_off[j + 1] = lane_off[j] + std::max(1, (end[j] - start[j] + L - 1) / L);
    // first pass, sync rounds, fallback, scan, write, DC: lane by lane, in the kernels' order
    const int lanes = lane_off[S];
    std::vector<JbState> st[2] = {std::vector<JbState>(lanes), std::vector<JbState>(lanes)};
    for (int s = 0; s < S; ++s) {
        const JbSeg g = jb_segment(sc, bytes.data(), start, s);
        for (int j = 0; j < g.nlanes; ++j) jb_lane_init(g, L, j, tabs, sc, st[0][lane_off[s] + j]);
    }
    for (int r = 1; r <= kJbRounds; ++r)
        for (int s = 0; s < S; ++s) {
            const JbSeg g = jb_segment(sc, bytes.data(), start, s);
            for (int j = 0; j < g.nlanes; ++j) jb_lane_round(g, L, j, tabs, sc, st[(r - 1) & 1].data() + lane_off[s], st[r & 1].data() + lane_off[s]);
        }
    JbState* fin = st[kJbRounds & 1].data();
    memset(coef, 0, sc.coef_elems * sizeof(short));
    for (int s = 0; s < S; ++s) {
        const JbSeg g = jb_segment(sc, bytes.data(), start, s);
        JbState* f = fin + lane_off[s];
        int j0 = g.nlanes;
        for (int j = 0; j < g.nlanes; ++j)
            if (f[j].changed) { j0 = j; break; }
        jb_lane_fallback(g, L, j0, tabs, sc, f);
        int total = 0, err = 0;
        for (int j = 0; j < g.nlanes; ++j) { f[j].first = total; total += f[j].nblk; err |= f[j].err; }
        if (err) status |= JB_ERR_SIZE;
        if (total != g.nblocks) status |= JB_ERR_BLOCKS;
        for (int j = 0; j < g.nlanes; ++j) {
            JbState e{};
            if (j) e = f[j - 1];
            e.first = f[j].first;
            jb_run<JB_WRITE>(g.d, g.nbytes, jb_lane_end(g, L, j), g.nblocks, tabs, sc, e, coef, g.mcu0);
        }
        int pred[3] = {0, 0, 0};
        jb_dc_values(sc, g.mcu0, 0, g.nblocks, pred, coef, true);
    }
    return status;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void jb_load_tables(JbTables& lt, const JbTables& g) {
    const int* src = reinterpret_cast<const int*>(&g);
    int* dst = reinterpret_cast<int*>(&lt);
    for (int i = threadIdx.x; i < (int)(sizeof(JbTables) / 4); i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

__device__ __forceinline__ int jb_exclusive_scan(int* a, int nthreads) {     // a[0..nthreads) in LDS -> exclusive prefix; returns the total
    __syncthreads();
    if (threadIdx.x == 0) {
        int s = 0;
        for (int i = 0; i < nthreads; ++i) { const int v = a[i]; a[i] = s; s += v; }
        a[nthreads] = s;
    }
    __syncthreads();
    return a[nthreads];
}

// one workgroup per image: the byte rules of jpeg_sync.h over per-thread runs of the entropy bytes
__global__ __launch_bounds__(1024) void jb_unstuff_kernel(const JbImage* __restrict__ imgs) {
    const JbImage& im = imgs[blockIdx.x];
    const unsigned char* d = im.raw;
    const long n = im.raw_len;
    const int S = im.t.sc.nseg, L = im.L, t = threadIdx.x;
    int* start = im.seg;
    int* end = start + S;
    int* lane_off = end + S;
    __shared__ int eoi, kept[1025], rsts[1025];
    const long per = (n + 1023) / 1024, a = std::min(n, t * per), b = std::min(n, a + per);
    if (t == 0) eoi = (int)n;
    __syncthreads();
    for (long i = a; i < b; ++i)
        if (jb_eoi(d, n, i)) { atomicMin(&eoi, (int)i); break; }
    __syncthreads();
    const long E = eoi;
    int kc = 0, rc = 0;
    for (long i = a; i < b; ++i) { kc += jb_keep(d, n, i); rc += i < E && jb_rst(d, n, i); }
    kept[t] = kc; rsts[t] = rc;
    const int total_kept = jb_exclusive_scan(kept, 1024);
    const int total_rst = jb_exclusive_scan(rsts, 1024);
    if (t == 0) { start[0] = 0; if (total_rst != S - 1) atomicOr(im.status, JB_ERR_RESTART); }
    for (int j = 1 + t; j < S; j += 1024) start[j] = total_kept;
    __syncthreads();
    int c = kept[t], q = rsts[t];
    for (long i = a; i < b; ++i) {
        if (i < E && jb_rst(d, n, i)) { if (q < S - 1) start[q + 1] = c; ++q; }
        if (jb_keep(d, n, i)) im.bytes[c++] = d[i];
    }
    __syncthreads();
    for (int j = t; j < S; j += 1024) end[j] = j + 1 < S ? start[j + 1] : total_kept;
    __syncthreads();
    c = kept[t]; q = rsts[t];
    for (long i = a; i < b; ++i) {
        if (i <= E && jb_marker(d, n, i) && !jb_rst(d, n, i)) atomicMin(&end[min(q, S - 1)], c);
        if (i < E && jb_rst(d, n, i)) ++q;
        c += jb_keep(d, n, i);
    }
    __syncthreads();
    // lanes per segment -> lane offsets (exclusive scan over the segments, per-thread runs)
    const int sper = (S + 1023) / 1024, s0 = std::min(S, t * sper), s1 = std::min(S, s0 + sper);
    int lc = 0;
    for (int j = s0; j < s1; ++j) lc += max(1, (end[j] - start[j] + L - 1) / L);
    kept[t] = lc;
    const int lanes = jb_exclusive_scan(kept, 1024);
    int o = kept[t];
    for (int j = s0; j < s1; ++j) { lane_off[j] = o; o += max(1, (end[j] - start[j] + L - 1) / L); }
    if (t == 0) lane_off[S] = min(lanes, im.lane_bound);
}

// MODE 0: first pass; 1: sync round `round` (reads st[(round - 1) & 1], writes st[round & 1]); 2: write pass from st[kJbRounds & 1];
// 3: the crop-aware route's write pass (DC differences of all blocks, AC of the blocks inside im.cr's MCU rectangle)
template <int MODE>
__global__ __launch_bounds__(kJbLanesPerWg) void jb_lane_kernel(const JbImage* __restrict__ imgs, const int2* __restrict__ wg, int round) {
    const int2 w = wg[blockIdx.x];                         // (image, first lane)
    const JbImage& im = imgs[w.x];
    __shared__ JbTables lt;
    jb_load_tables(lt, im.t);
    const int S = lt.sc.nseg;
    const int* lane_off = im.seg + 2 * S;
    const int g = w.y + threadIdx.x;
    if (g >= lane_off[S]) return;
    int lo = 0, hi = S - 1;                                // the segment holding lane g: the last s with lane_off[s] <= g
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (lane_off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const JbSeg sg = jb_segment(lt.sc, im.bytes, im.seg, lo);
    const int j = g - lane_off[lo];
    if (MODE == 0) {
        jb_lane_init(sg, im.L, j, lt.tabs, lt.sc, im.st[0][g]);
    } else if (MODE == 1) {
        jb_lane_round(sg, im.L, j, lt.tabs, lt.sc, im.st[(round - 1) & 1] + lane_off[lo], im.st[round & 1] + lane_off[lo]);
    } else {
        const JbState* f = im.st[kJbRounds & 1] + lane_off[lo];
        JbState e{};
        if (j) e = f[j - 1];
        e.first = f[j].first;
        if (MODE == 2) jb_run<JB_WRITE>(sg.d, sg.nbytes, jb_lane_end(sg, im.L, j), sg.nblocks, lt.tabs, lt.sc, e, im.coef, sg.mcu0);
        else jb_run<JB_WRITE_CROP>(sg.d, sg.nbytes, jb_lane_end(sg, im.L, j), sg.nblocks, lt.tabs, lt.sc, e, im.coef, sg.mcu0, &im.cr);
    }
}

// one workgroup per (image, segment): serial fallback for unproven lanes, then each lane's first block and the segment's checks
__global__ __launch_bounds__(256) void jb_seg_kernel(const JbImage* __restrict__ imgs, const int2* __restrict__ wg) {
    const int2 w = wg[blockIdx.x];                         // (image, segment)
    const JbImage& im = imgs[w.x];
    __shared__ JbTables lt;
    __shared__ int j0, err, part[257];
    jb_load_tables(lt, im.t);
    const JbSeg sg = jb_segment(lt.sc, im.bytes, im.seg, w.y);
    JbState* f = im.st[kJbRounds & 1] + im.seg[2 * lt.sc.nseg + w.y];
    const int t = threadIdx.x, nl = sg.nlanes;
    if (t == 0) { j0 = nl; err = 0; }
    __syncthreads();
    for (int j = t; j < nl; j += 256)
        if (f[j].changed) atomicMin(&j0, j);
    __syncthreads();
    if (t == 0) jb_lane_fallback(sg, im.L, j0, lt.tabs, lt.sc, f);
    __syncthreads();
    const int per = (nl + 255) / 256, a = min(nl, t * per), b = min(nl, a + per);
    int c = 0, e = 0;
    for (int j = a; j < b; ++j) { c += f[j].nblk; e |= f[j].err; }
    part[t] = c;
    if (e) atomicOr(&err, 1);
    const int total = jb_exclusive_scan(part, 256);
    c = part[t];
    for (int j = a; j < b; ++j) { f[j].first = c; c += f[j].nblk; }
    if (t == 0) {
        const int bits = (err ? JB_ERR_SIZE : 0) | (total != sg.nblocks ? JB_ERR_BLOCKS : 0);
        if (bits) atomicOr(im.status, bits);
    }
}

// one workgroup per (image, segment): DC differences -> values, per component, over per-thread runs of blocks (CROP: differences from
// im.cr.dc, values into the rectangle's blocks)
template <bool CROP>
__global__ __launch_bounds__(256) void jb_dc_kernel(const JbImage* __restrict__ imgs, const int2* __restrict__ wg) {
    const int2 w = wg[blockIdx.x];
    const JbImage& im = imgs[w.x];
    const JbScan& sc = im.t.sc;
    const int mcu0 = w.y * sc.restart, nb = (min(mcu0 + sc.restart, sc.mcus) - mcu0) * sc.bpm;
    __shared__ int part[3][257];
    const int t = threadIdx.x, per = (nb + 255) / 256, a = min(nb, t * per), b = min(nb, a + per);
    int pred[3] = {0, 0, 0};
    if (CROP) jb_dc_values_crop(sc, im.cr, mcu0, a, b, pred, im.coef, false);
    else jb_dc_values(sc, mcu0, a, b, pred, im.coef, false);
    for (int ci = 0; ci < 3; ++ci) part[ci][t] = pred[ci];
    for (int ci = 0; ci < 3; ++ci) jb_exclusive_scan(part[ci], 256);
    for (int ci = 0; ci < 3; ++ci) pred[ci] = part[ci][t];
    if (CROP) jb_dc_values_crop(sc, im.cr, mcu0, a, b, pred, im.coef, true);
    else jb_dc_values(sc, mcu0, a, b, pred, im.coef, true);
}

__global__ __launch_bounds__(64) void jb_idct_kernel(const JbImage* __restrict__ imgs) {
    const JbImage& im = imgs[blockIdx.y];
    int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= im.nblocks_idct) return;
    int comp = 0;
    while (comp + 1 < im.jd.nc && b >= im.jd.bw[comp] * im.jd.bh[comp]) { b -= im.jd.bw[comp] * im.jd.bh[comp]; ++comp; }
    jpeg_idct_block(im.coef, im.planes, im.jd, comp, b);
}

__global__ __launch_bounds__(256) void jb_color_kernel(const JbImage* __restrict__ imgs) {
    const JbImage& im = imgs[blockIdx.z];
    const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= im.jd.W || y >= im.jd.H) return;
    jpeg_color_pixel(im.planes, im.out, im.jd, im.pitch, x, y);
}

// crop-aware route: colour over the pixels the warp reads (image coordinates; im.jd places them in the rectangle's planes and patch)
__global__ __launch_bounds__(256) void jb_color_crop_kernel(const JbImage* __restrict__ imgs) {
    const JbImage& im = imgs[blockIdx.z];
    const int x = im.cr.rect[0] + blockIdx.x * 64 + (threadIdx.x & 63), y = im.cr.rect[1] + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (x >= im.cr.rect[2] || y >= im.cr.rect[3]) return;
    jpeg_color_pixel(im.planes, im.out, im.jd, im.pitch, x, y);
}

// crop-aware route: capf_warp_affine's arithmetic (warp_rule.h) on the patch; out = [n, out_h, out_w, 3]
__global__ __launch_bounds__(256) void jb_warp_crop_kernel(const JbImage* __restrict__ imgs, unsigned char* __restrict__ out, int n, int out_h, int out_w) {
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    if (t >= (long)n * out_h * out_w) return;
    const int x = (int)(t % out_w), y = (int)((t / out_w) % out_h);
    const JbImage& im = imgs[t / ((long)out_w * out_h)];
    const WarpMap w = warp_inverse(im.cr.m);
    warp_affine_pixel<true>(im.out, im.jd.H, im.jd.W, im.pitch, im.cr.rect, w, x, y, out + t * 3);
}

// ---- batch layout -----------------------------------------------------------------------------------------------------------------
static inline size_t jb_align(size_t x) { return (x + 255) & ~(size_t)255; }

struct JbLayout {
    size_t desc, wg_lane, wg_seg, raw, upload;             // the uploaded prefix
    size_t bytes, seg, st, coef, dc, planes, patch, total;  // device-only areas (dc, patch: crop-aware route, empty otherwise)
    std::vector<size_t> raw_off, bytes_off, seg_off, st_off, coef_off, dc_off, planes_off, patch_off;
    int n_wg_lane = 0, n_wg_seg = 0;
};

static void jb_layout(const std::vector<JbPrep>& p, JbLayout& l) {
    const int n = (int)p.size();
    l.raw_off.resize(n); l.bytes_off.resize(n); l.seg_off.resize(n); l.st_off.resize(n); l.coef_off.resize(n); l.planes_off.resize(n);
    l.dc_off.resize(n); l.patch_off.resize(n);
    size_t raw = 0, bytes = 0, seg = 0, st = 0, coef = 0, planes = 0, dc = 0, patch = 0;
    l.n_wg_lane = l.n_wg_seg = 0;
    for (int i = 0; i < n; ++i) {
        l.raw_off[i] = raw; raw += (p[i].raw_len + 15) & ~15;
        l.bytes_off[i] = bytes; bytes += (p[i].raw_len + 15) & ~15;
        l.seg_off[i] = seg; seg += ((3 * (size_t)p[i].t.sc.nseg + 1) * sizeof(int) + 15) & ~(size_t)15;
        l.st_off[i] = st; st += 2 * (size_t)p[i].lane_bound * sizeof(JbState);
        l.coef_off[i] = coef; coef += ((p[i].crop ? (size_t)p[i].cr.coef_elems : p[i].h.coef_elems) * sizeof(short) + 15) & ~(size_t)15;
        l.dc_off[i] = dc; dc += p[i].crop ? ((size_t)p[i].t.sc.mcus * p[i].t.sc.bpm * sizeof(short) + 15) & ~(size_t)15 : 0;
        l.planes_off[i] = planes; planes += p[i].crop ? p[i].crop_plane_bytes : p[i].h.plane_bytes;
        l.patch_off[i] = patch; patch += p[i].patch_bytes;
        l.n_wg_lane += (p[i].lane_bound + kJbLanesPerWg - 1) / kJbLanesPerWg;
        l.n_wg_seg += p[i].t.sc.nseg;
    }
    l.desc = 0;
    l.wg_lane = jb_align(n * sizeof(JbImage));
    l.wg_seg = jb_align(l.wg_lane + l.n_wg_lane * sizeof(int2));
    l.raw = jb_align(l.wg_seg + l.n_wg_seg * sizeof(int2));
    l.upload = l.raw + raw;
    l.bytes = jb_align(l.upload);
    l.seg = jb_align(l.bytes + bytes);
    l.st = jb_align(l.seg + seg);
    l.coef = jb_align(l.st + st);
    l.dc = jb_align(l.coef + coef);                         // (coef and dc are zeroed together: [l.coef, l.planes))
    l.planes = jb_align(l.dc + dc);
    l.patch = jb_align(l.planes + planes);
    l.total = jb_align(l.patch + patch);
}

static int jb_subseq(int subseq_bytes) {
    if (subseq_bytes == 0) return kJbSubseqDefault;
    return subseq_bytes >= 1 && subseq_bytes <= (1 << 20) ? subseq_bytes : -1;
}

// What both routes do with a prepared batch: stage [descriptors | work tables | raw bytes] (fill(i, im) sets the route's own fields of
// descriptor i), upload once, zero the status words and [zero, zero + zero_bytes), and enqueue the entropy stages up to jb_seg_kernel.
struct JbCall {
    hipStream_t s;
    const JbImage* desc;
    const int2 *wl, *ws;
};

template <class Fill>
static int jb_enqueue_entropy(void* stream, const std::vector<JbPrep>& p, const JbLayout& l, int L, unsigned char* dev, int32_t* status, void* zero,
                              size_t zero_bytes, Fill fill, JbCall& c, hipEvent_t& uploaded_out) {
    const int n = (int)p.size();
    static thread_local std::vector<unsigned char> host;  // (one call at a time per thread: the upload is waited for before returning)
    host.assign(l.upload, 0);
    JbImage* desc = reinterpret_cast<JbImage*>(host.data() + l.desc);
    int2* wl = reinterpret_cast<int2*>(host.data() + l.wg_lane);
    int2* ws = reinterpret_cast<int2*>(host.data() + l.wg_seg);
    for (int i = 0, nl = 0, ns = 0; i < n; ++i) {
        JbImage& im = desc[i];
        im.t = p[i].t;
        im.raw = dev + l.raw + l.raw_off[i];
        im.bytes = dev + l.bytes + l.bytes_off[i];
        im.seg = reinterpret_cast<int*>(dev + l.seg + l.seg_off[i]);
        im.st[0] = reinterpret_cast<JbState*>(dev + l.st + l.st_off[i]);
        im.st[1] = im.st[0] + p[i].lane_bound;
        im.planes = dev + l.planes + l.planes_off[i];
        im.status = status + i;
        im.raw_len = p[i].raw_len;
        im.lane_bound = p[i].lane_bound;
        im.L = L;
        fill(i, im);
        memcpy(host.data() + l.raw + l.raw_off[i], p[i].raw, p[i].raw_len);
        for (int w = 0; w < (p[i].lane_bound + kJbLanesPerWg - 1) / kJbLanesPerWg; ++w) wl[nl++] = make_int2(i, w * kJbLanesPerWg);
        for (int s = 0; s < p[i].t.sc.nseg; ++s) ws[ns++] = make_int2(i, s);
    }
    hipStream_t s = static_cast<hipStream_t>(stream);
    static thread_local hipEvent_t uploaded = nullptr;
    if (!uploaded && hipEventCreateWithFlags(&uploaded, hipEventDisableTiming) != hipSuccess) return CAPF_ERR_HIP;
    uploaded_out = uploaded;
    if (hipMemcpyAsync(dev, host.data(), l.upload, hipMemcpyHostToDevice, s) != hipSuccess) return CAPF_ERR_HIP;
    if (hipEventRecord(uploaded, s) != hipSuccess) return CAPF_ERR_HIP;
    if (hipMemsetAsync(status, 0, n * sizeof(int32_t), s) != hipSuccess) return CAPF_ERR_HIP;
    if (zero_bytes && hipMemsetAsync(zero, 0, zero_bytes, s) != hipSuccess) return CAPF_ERR_HIP;
    c.s = s;
    c.desc = reinterpret_cast<const JbImage*>(dev + l.desc);
    c.wl = reinterpret_cast<const int2*>(dev + l.wg_lane);
    c.ws = reinterpret_cast<const int2*>(dev + l.wg_seg);
    hipLaunchKernelGGL(jb_unstuff_kernel, dim3(n), dim3(1024), 0, s, c.desc);
    hipLaunchKernelGGL(jb_lane_kernel<0>, dim3(l.n_wg_lane), dim3(kJbLanesPerWg), 0, s, c.desc, c.wl, 0);
    for (int r = 1; r <= kJbRounds; ++r) hipLaunchKernelGGL(jb_lane_kernel<1>, dim3(l.n_wg_lane), dim3(kJbLanesPerWg), 0, s, c.desc, c.wl, r);
    hipLaunchKernelGGL(jb_seg_kernel, dim3(l.n_wg_seg), dim3(256), 0, s, c.desc, c.ws);
    return CAPF_OK;
}

// the staging buffer is reused by this thread's next call: wait for the upload only, never for the kernels
static int jb_finish(hipEvent_t uploaded) {
    if (hipGetLastError() != hipSuccess) return CAPF_ERR_HIP;
    return hipEventSynchronize(uploaded) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

}  // namespace capf

using capf::JbPrep;

int capf_jpeg_batch_info(int n, const uint8_t* const* data, const size_t* n_bytes, int subseq_bytes, int32_t* info, size_t* scratch_bytes) {
    const int L = capf::jb_subseq(subseq_bytes);
    if (n < 0 || (n && (!data || !n_bytes)) || L < 0) return CAPF_ERR_INVALID;
    std::vector<JbPrep> p(n);
    int worst = CAPF_OK;
    for (int i = 0; i < n; ++i) {
        const int rc = capf::jb_prepare(data[i], n_bytes[i], L, p[i]);
        if (info) {
            int32_t* r = info + 5 * i;
            r[0] = rc == CAPF_OK ? p[i].h.W : 0; r[1] = rc == CAPF_OK ? p[i].h.H : 0; r[2] = rc == CAPF_OK ? p[i].h.nc : 0;
            r[3] = rc == CAPF_OK ? (int32_t)p[i].h.coef_elems : 0; r[4] = rc;
        }
        if (rc != CAPF_OK && worst == CAPF_OK) worst = rc;
    }
    if (worst != CAPF_OK) return worst;
    capf::JbLayout l;
    capf::jb_layout(p, l);
    if (scratch_bytes) *scratch_bytes = l.total;
    return CAPF_OK;
}

int capf_jpeg_coefficients_subseq(const uint8_t* data, size_t n_bytes, int16_t* coef, size_t coef_elems, int subseq_bytes) {
    const int L = capf::jb_subseq(subseq_bytes);
    if (!data || !coef || L < 0) return CAPF_ERR_INVALID;
    JbPrep p;
    const int rc = capf::jb_prepare(data, n_bytes, L, p);
    if (rc != CAPF_OK) return rc;
    if (coef_elems < p.h.coef_elems) return CAPF_ERR_INVALID;
    return capf::jb_emulate(p, L, coef) ? CAPF_ERR_INVALID : CAPF_OK;
}

int capf_jpeg_decode_batch(void* stream, int n, const uint8_t* const* data, const size_t* n_bytes, uint8_t* const* out_bgr, const size_t* out_pitch_bytes,
                           int16_t* coef_out, void* scratch, size_t scratch_bytes, int32_t* status, int subseq_bytes) {
    using namespace capf;
    const int L = jb_subseq(subseq_bytes);
    if (n <= 0 || !data || !n_bytes || !out_bgr || !out_pitch_bytes || !scratch || !status || L < 0) return CAPF_ERR_INVALID;
    std::vector<JbPrep> p(n);
    for (int i = 0; i < n; ++i) {                        // the whole batch is checked before anything is enqueued
        const int rc = jb_prepare(data[i], n_bytes[i], L, p[i]);
        if (rc != CAPF_OK) return rc;
        if (!out_bgr[i] || out_pitch_bytes[i] < (size_t)p[i].h.W * 3) return CAPF_ERR_INVALID;
    }
    JbLayout l;
    jb_layout(p, l);
    if (scratch_bytes < l.total) return CAPF_ERR_INVALID;
    unsigned char* dev = static_cast<unsigned char*>(scratch);
    size_t coef_base = 0;
    int max_blocks = 0, max_w = 0, max_h = 0;
    for (int i = 0; i < n; ++i) {
        coef_base += p[i].h.coef_elems;
        max_blocks = std::max(max_blocks, (int)(p[i].h.coef_elems / 64));
        max_w = std::max(max_w, p[i].h.W);
        max_h = std::max(max_h, p[i].h.H);
    }
    size_t coef_at = 0;
    auto fill = [&](int i, JbImage& im) {
        im.jd = jpeg_dev(p[i].h);
        im.coef = coef_out ? coef_out + coef_at : reinterpret_cast<short*>(dev + l.coef + l.coef_off[i]);
        coef_at += p[i].h.coef_elems;
        im.out = out_bgr[i];
        im.pitch = (long)out_pitch_bytes[i];
        im.nblocks_idct = (int)(p[i].h.coef_elems / 64);
    };
    JbCall c;
    hipEvent_t uploaded;
    const int rc = jb_enqueue_entropy(stream, p, l, L, dev, status, coef_out ? (void*)coef_out : (void*)(dev + l.coef),
                                      coef_out ? coef_base * sizeof(short) : l.planes - l.coef, fill, c, uploaded);
    if (rc != CAPF_OK) return rc;
    hipLaunchKernelGGL(jb_lane_kernel<2>, dim3(l.n_wg_lane), dim3(kJbLanesPerWg), 0, c.s, c.desc, c.wl, 0);
    hipLaunchKernelGGL(jb_dc_kernel<false>, dim3(l.n_wg_seg), dim3(256), 0, c.s, c.desc, c.ws);
    hipLaunchKernelGGL(jb_idct_kernel, dim3((max_blocks + 63) / 64, n), dim3(64), 0, c.s, c.desc);
    hipLaunchKernelGGL(jb_color_kernel, dim3((max_w + 63) / 64, (max_h + 3) / 4, n), dim3(256), 0, c.s, c.desc);
    return jb_finish(uploaded);
}

// ---- crop-aware route ---------------------------------------------------------------------------------------------------------------
int capf_jpeg_crop_rect(int width, int height, int h_samp, int v_samp, const double m[6], int out_w, int out_h, int32_t pixel_rect[4], int32_t mcu_rect[4]) {
    const bool sampling = (h_samp == 1 && v_samp == 1) || (h_samp == 2 && v_samp == 1) || (h_samp == 2 && v_samp == 2);
    if (width <= 0 || height <= 0 || !sampling || !m || out_w <= 0 || out_h <= 0 || !pixel_rect || !mcu_rect) return CAPF_ERR_INVALID;
    int rect[4], mcu[4];
    capf::warp_source_rect(width, height, m, out_w, out_h, rect);
    capf::warp_mcu_rect(width, height, h_samp, v_samp, rect, mcu);
    for (int k = 0; k < 4; ++k) { pixel_rect[k] = rect[k]; mcu_rect[k] = mcu[k]; }
    return CAPF_OK;
}

int capf_jpeg_crop_batch_info(int n, const uint8_t* const* data, const size_t* n_bytes, const double* m, int out_w, int out_h, int subseq_bytes,
                              int32_t* info, size_t* scratch_bytes) {
    const int L = capf::jb_subseq(subseq_bytes);
    if (n <= 0 || !data || !n_bytes || !m || out_w <= 0 || out_h <= 0 || L < 0) return CAPF_ERR_INVALID;
    std::vector<JbPrep> p(n);
    int worst = CAPF_OK;
    for (int i = 0; i < n; ++i) {
        const int rc = capf::jb_prepare(data[i], n_bytes[i], L, p[i]);
        if (rc == CAPF_OK) capf::jb_prepare_crop(p[i], m + 6 * (size_t)i, out_w, out_h);
        if (info) {
            int32_t* r = info + 13 * i;
            for (int k = 0; k < 13; ++k) r[k] = 0;
            r[4] = rc;
            if (rc == CAPF_OK) {
                r[0] = p[i].h.W; r[1] = p[i].h.H; r[2] = p[i].h.nc; r[3] = (int32_t)p[i].cr.coef_elems;
                for (int k = 0; k < 4; ++k) { r[5 + k] = p[i].cr.rect[k]; r[9 + k] = p[i].cr.mcu[k]; }
            }
        }
        if (rc != CAPF_OK && worst == CAPF_OK) worst = rc;
    }
    if (worst != CAPF_OK) return worst;
    capf::JbLayout l;
    capf::jb_layout(p, l);
    if (scratch_bytes) *scratch_bytes = l.total;
    return CAPF_OK;
}

int capf_jpeg_decode_crop_batch(void* stream, int n, const uint8_t* const* data, const size_t* n_bytes, const double* m, int out_h, int out_w, uint8_t* out,
                                void* scratch, size_t scratch_bytes, int32_t* status, int subseq_bytes) {
    using namespace capf;
    const int L = jb_subseq(subseq_bytes);
    if (n <= 0 || !data || !n_bytes || !m || out_h <= 0 || out_w <= 0 || !out || !scratch || !status || L < 0) return CAPF_ERR_INVALID;
    std::vector<JbPrep> p(n);
    int max_blocks = 0, max_w = 0, max_h = 0;
    for (int i = 0; i < n; ++i) {                        // the whole batch is checked before anything is enqueued
        const int rc = jb_prepare(data[i], n_bytes[i], L, p[i]);
        if (rc != CAPF_OK) return rc;
        jb_prepare_crop(p[i], m + 6 * (size_t)i, out_w, out_h);
        max_blocks = std::max(max_blocks, (int)(p[i].cr.coef_elems / 64));
        max_w = std::max(max_w, p[i].cr.rect[2] - p[i].cr.rect[0]);
        max_h = std::max(max_h, p[i].cr.rect[3] - p[i].cr.rect[1]);
    }
    JbLayout l;
    jb_layout(p, l);
    if (scratch_bytes < l.total) return CAPF_ERR_INVALID;
    unsigned char* dev = static_cast<unsigned char*>(scratch);
    auto fill = [&](int i, JbImage& im) {
        im.jd = p[i].jd;
        im.cr = p[i].cr;
        im.cr.dc = reinterpret_cast<short*>(dev + l.dc + l.dc_off[i]);
        im.coef = reinterpret_cast<short*>(dev + l.coef + l.coef_off[i]);
        im.out = dev + l.patch + l.patch_off[i];
        im.pitch = (long)p[i].patch_pitch;
        im.nblocks_idct = (int)(p[i].cr.coef_elems / 64);
    };
    JbCall c;
    hipEvent_t uploaded;
    const int rc = jb_enqueue_entropy(stream, p, l, L, dev, status, dev + l.coef, l.planes - l.coef, fill, c, uploaded);
    if (rc != CAPF_OK) return rc;
    hipLaunchKernelGGL(jb_lane_kernel<3>, dim3(l.n_wg_lane), dim3(kJbLanesPerWg), 0, c.s, c.desc, c.wl, 0);
    hipLaunchKernelGGL(jb_dc_kernel<true>, dim3(l.n_wg_seg), dim3(256), 0, c.s, c.desc, c.ws);
    if (max_blocks) {                                    // (no file's crop touches its image: nothing to transform, the warp writes the border)
        hipLaunchKernelGGL(jb_idct_kernel, dim3((max_blocks + 63) / 64, n), dim3(64), 0, c.s, c.desc);
        hipLaunchKernelGGL(jb_color_crop_kernel, dim3((max_w + 63) / 64, (max_h + 3) / 4, n), dim3(256), 0, c.s, c.desc);
    }
    const long total = (long)n * out_h * out_w;
    hipLaunchKernelGGL(jb_warp_crop_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, c.s, c.desc, out, n, out_h, out_w);
    return jb_finish(uploaded);
}
