// CPN's two-peak heatmap decode (gfx950): what cpn/test.py:79-108 does to the heatmaps of refine_net.final_predict, per (frame, joint) --
// normalise by the maximum, pad by 10, 21 x 21 Gaussian blur, first and second maximum, a quarter pixel from the first towards the second.
// include/capf.h (capf_cpn_decode) has the rules and the ONE summation order of the blur; this file is compiled with -ffp-contract=off, every
// fma below is written out.
//
// One workgroup of 512 threads per (frame, joint); everything it needs stays in LDS -- no scratch, no atomics, no second launch:
//   n   [H][W]            fp32   the map divided by its maximum (the zero border of the padded plane P is index arithmetic, not memory)
//   R   [H + 20][W + 20]  fp64   the row pass over P
// The column pass D is never stored (a second fp64 plane of 116 x 92 would not fit beside the first for a 96 x 72 map): a thread folds the
// cells it computes -- cell c = tid + 512 k, ascending -- into its own two best (value, index) pairs; the first maximum is the best of the
// threads' firsts, the second the best of {the winner's runner-up, every other thread's first, the zeroed cell itself}.
// "Best" is one total order, value descending then index ascending, so the wave64 butterfly (__shfl_xor) and the fold over the 8 waves give
// the first maximum in row-major order whatever the order of the merges.
// LDS banking: both planes are dense (pitch = width), a wave's 64 cells are 64 consecutive indices, and tap i of either pass reads them at one
// common offset -- 64 consecutive fp32 / fp64 words (two at a row end), conflict-free for ds_read_b32 / ds_read_b64 at any pitch, even ones
// included; the column pass needs no padding column.
//
// Flip-test pair (capf_cpn_decode_pair), the PAIR instantiations of the same kernel: the map holds [2 B] frames, frame B + b the mirror of source
// frame b, and workgroup (b, j) loads zf = 0.5f * (z[b, y, x, j] + z[B + b, y, W - 1 - x, swap[j]]) where the single form loads z (cpn/test.py:62-70:
// cv2.flip(.., 1), the symmetric joints exchanged, no column shift; the fp32 sum rounded once, then halved).  Planes, passes, reductions and
// their orders are the single form's; the score re-reads BOTH frames, and the workgroup also writes joint swap[j] of the mirrored set of the
// stacks -- swap is a permutation, so every element has one writer.
#include <math.h>

#include "fmt16.h"
#include "kernels.h"
#include "pair_stacks.h"

namespace capf {

static constexpr int CPN_THREADS = 512, CPN_WAVES = CPN_THREADS / 64;
static constexpr size_t CPN_RED_BYTES = 256;       // reduction scratch in front of the planes: CPN_WAVES (double, int) pairs + flags

size_t cpn_decode_lds_bytes(int H, int W) {
    if (H < 1 || W < 1 || H > (1 << 14) || W > (1 << 14)) return (size_t)-1;
    return CPN_RED_BYTES + (size_t)(H + 2 * CPN_BORDER) * (W + 2 * CPN_BORDER) * sizeof(double) + (size_t)H * W * sizeof(float);
}

// g_i = e_i / sum(e), e_i = exp(-(i - 10)^2 / (2 * 3.5^2)): e mirrored (bit-symmetric by construction), the sum compensated (Neumaier) and the
// quotient corrected by its residual against the two-word sum, so that the taps add up to 1 within 2^-52
void cpn_decode_taps(double g[CPN_TAPS]) {
    const double sigma = 0.3 * ((CPN_TAPS - 1) * 0.5 - 1.0) + 0.8;       // OpenCV's rule for ksize = 21, sigma = 0: 3.5
    double e[CPN_TAPS];
    for (int i = 0; i <= CPN_BORDER; ++i) {
        const double d = (double)(i - CPN_BORDER);
        e[i] = e[CPN_TAPS - 1 - i] = exp(-(d * d) / (2.0 * sigma * sigma));
    }
    double s = 0.0, c = 0.0;
    for (int i = 0; i < CPN_TAPS; ++i) {
        const double t = s + e[i];
        c += fabs(s) >= fabs(e[i]) ? (s - t) + e[i] : (e[i] - t) + s;
        s = t;
    }
    for (int i = 0; i <= CPN_BORDER; ++i) {
        const double q = e[i] / s;
        const double r = fma(-q, s, e[i]) - q * c;                       // e_i - q (s + c)
        g[i] = g[CPN_TAPS - 1 - i] = q + r / s;
    }
}

template <bool PAIR> struct CpnArgsOf { typedef CpnDecodeArgs type; };
template <> struct CpnArgsOf<true> { typedef CpnPairArgs type; };

// pixel p of the map the decode works on: the frame's own value, or (PAIR) its fold with the mirror frame's -- zm points at channel swap[j] of
// frame B + b
template <class L, bool PAIR>
__device__ __forceinline__ float cpn_pixel(const typename L::T* __restrict__ z, const typename L::T* __restrict__ zm, const int p, const int W,
                                           const int C) {
    const float zo = L::ld1(z + (size_t)p * C);
    if constexpr (PAIR) {
        const int x = p % W;                                             // row y = p / W: column W - 1 - x of it is pixel p - x + (W - 1 - x)
        const float sum = zo + L::ld1(zm + (size_t)(p - x + (W - 1 - x)) * C);       // (the sum rounded to fp32 ...
        return 0.5f * sum;                                               //  ... then halved)
    } else {
        return zo;
    }
}

struct CpnBest { double v; int i; };
__device__ __forceinline__ bool cpn_better(const double v, const int i, const CpnBest& b) { return v > b.v || (v == b.v && i < b.i); }

// every thread gets the block's best pair (all threads call; `red` holds CPN_WAVES pairs)
__device__ __forceinline__ CpnBest cpn_block_best(CpnBest b, double* red_v, int* red_i) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double ov = __shfl_xor(b.v, m, 64);
        const int oi = __shfl_xor(b.i, m, 64);
        if (cpn_better(ov, oi, b)) { b.v = ov; b.i = oi; }
    }
    __syncthreads();                                                     // (the scratch of an earlier reduction has been read)
    if ((threadIdx.x & 63) == 0) { red_v[threadIdx.x >> 6] = b.v; red_i[threadIdx.x >> 6] = b.i; }
    __syncthreads();
    CpnBest r{red_v[0], red_i[0]};
#pragma unroll
    for (int w = 1; w < CPN_WAVES; ++w)
        if (cpn_better(red_v[w], red_i[w], r)) { r.v = red_v[w]; r.i = red_i[w]; }
    return r;
}

__device__ __forceinline__ int cpn_reflect(const int t, const int n) { return t < 0 ? -t : t >= n ? 2 * (n - 1) - t : t; }   // reflect-101, |overhang| <= 10 < n

template <class L, bool PAIR>
__global__ void __launch_bounds__(CPN_THREADS) cpn_decode_kernel(const typename CpnArgsOf<PAIR>::type a) {
    extern __shared__ double cpn_lds[];
    const int tid = threadIdx.x;
    const int H = a.H, W = a.W, HW = H * W, Hp = H + 2 * CPN_BORDER, Wp = W + 2 * CPN_BORDER, cells = Hp * Wp;
    double* const red_v = cpn_lds;                                       // [CPN_WAVES]
    int* const red_i = reinterpret_cast<int*>(cpn_lds + CPN_WAVES);      // [CPN_WAVES]
    float* const red_f = reinterpret_cast<float*>(red_i + CPN_WAVES);    // [CPN_WAVES] maxima, then [CPN_WAVES] flags
    double* const R = cpn_lds + CPN_RED_BYTES / sizeof(double);          // [Hp][Wp]
    float* const n = reinterpret_cast<float*>(R + cells);                // [H][W]
    const int b = (int)blockIdx.x / a.J, j = (int)blockIdx.x - b * a.J;
    const typename L::T* __restrict__ z = static_cast<const typename L::T*>(a.heat) + (size_t)b * HW * a.C + j;
    const size_t o = (size_t)blockIdx.x;                                 // = b * J + j
    const typename L::T* __restrict__ zm = nullptr;
    size_t om = 0;                                                       // PAIR: (b, swap[j]) of the mirrored set of the stacks
    if constexpr (PAIR) {
        const int js = a.swap.j[j];
        zm = static_cast<const typename L::T*>(a.heat) + ((size_t)a.B + b) * HW * a.C + js;
        om = ((size_t)a.B + b) * a.J + js;
    }

    // ---- the map, its maximum, and whether every value is finite
    float m = -INFINITY;
    int bad = 0;
    for (int p = tid; p < HW; p += CPN_THREADS) {
        const float v = cpn_pixel<L, PAIR>(z, zm, p, W, a.C);
        n[p] = v;
        if constexpr (PAIR)
            if (a.fused) a.fused[o * HW + p] = v;
        if (!(fabsf(v) <= 3.4028234663852886e38f)) bad = 1;              // NaN or +-Inf
        if (v > m) m = v;
    }
#pragma unroll
    for (int k = 1; k < 64; k <<= 1) {
        const float om = __shfl_xor(m, k, 64);
        bad |= __shfl_xor(bad, k, 64);
        if (om > m) m = om;
    }
    if ((tid & 63) == 0) { red_f[tid >> 6] = m; red_f[CPN_WAVES + (tid >> 6)] = bad ? 1.f : 0.f; }
    __syncthreads();
    float M = red_f[0];
    bad = red_f[CPN_WAVES] != 0.f;
#pragma unroll
    for (int w = 1; w < CPN_WAVES; ++w) {
        if (red_f[w] > M) M = red_f[w];
        bad |= red_f[CPN_WAVES + w] != 0.f;
    }
    if (bad || M == 0.f) {                                               // (uniform over the workgroup)
        const double qnan = __builtin_nan("");
        if (a.blurred)
            for (int c = tid; c < cells; c += CPN_THREADS) a.blurred[o * cells + c] = qnan;
        if (tid == 0) {
            const float fn = __builtin_nanf("");
            a.kcrop[o * 2] = fn; a.kcrop[o * 2 + 1] = fn;
            if (a.k2d) { a.k2d[o * 2] = fn; a.k2d[o * 2 + 1] = fn; }
            if (a.score) a.score[o] = fn;
            if constexpr (PAIR) {
                a.kcrop[om * 2] = fn; a.kcrop[om * 2 + 1] = fn;
                if (a.k2d) { a.k2d[om * 2] = fn; a.k2d[om * 2 + 1] = fn; }
            }
        }
        return;
    }
    for (int p = tid; p < HW; p += CPN_THREADS) n[p] = n[p] / M;         // (a thread's own elements; IEEE division)
    __syncthreads();

    // ---- row pass: R[y][x] = fold over i ascending of fma(g_i, P[y][reflect(x + i - 10)], acc), acc = +0
    for (int c = tid; c < cells; c += CPN_THREADS) {
        const int y = c / Wp, x = c - y * Wp, yy = y - CPN_BORDER;
        double acc = 0.0;
        if (yy >= 0 && yy < H) {                                         // (a border row of P is zeros: every fma leaves +0)
            const float* row = n + yy * W;
#pragma unroll
            for (int i = 0; i < CPN_TAPS; ++i) {
                const int xx = cpn_reflect(x + i - CPN_BORDER, Wp) - CPN_BORDER;
                const double v = (xx >= 0 && xx < W) ? (double)row[xx] : 0.0;
                acc = fma(a.g[i], v, acc);
            }
        }
        R[c] = acc;
    }
    __syncthreads();

    // ---- column pass: D[y][x] = the same fold over R[reflect(y + i - 10)][x]; the thread's two best cells
    CpnBest b1{-INFINITY, 0x7fffffff}, b2{-INFINITY, 0x7fffffff};
    for (int c = tid; c < cells; c += CPN_THREADS) {
        const int y = c / Wp, x = c - y * Wp;
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < CPN_TAPS; ++i) acc = fma(a.g[i], R[cpn_reflect(y + i - CPN_BORDER, Hp) * Wp + x], acc);
        if (a.blurred) a.blurred[o * cells + c] = acc;
        if (acc > b1.v) { b2 = b1; b1.v = acc; b1.i = c; }               // (c ascends: a tie keeps the earlier cell)
        else if (acc > b2.v) { b2.v = acc; b2.i = c; }
    }
    const CpnBest first = cpn_block_best(b1, red_v, red_i);
    // D[y1][x1] = 0, then the first maximum again: the zeroed cell competes with its 0
    CpnBest cand = (first.i != 0x7fffffff && first.i % CPN_THREADS == tid) ? b2 : b1;
    CpnBest second = cpn_block_best(cand, red_v, red_i);
    if (tid != 0) return;
    const int i1 = first.i == 0x7fffffff ? 0 : first.i;                  // (every D a NaN: outside the contract, cell 0)
    if (cpn_better(0.0, i1, second)) { second.v = 0.0; second.i = i1; }
    const int i2 = second.i == 0x7fffffff ? 0 : second.i;
    const int y1 = i1 / Wp, x1 = i1 - y1 * Wp, y2 = i2 / Wp, x2 = i2 - y2 * Wp;
    double x = (double)(x1 - CPN_BORDER), y = (double)(y1 - CPN_BORDER);
    const double px = (double)(x2 - x1), py = (double)(y2 - y1);
    const double ln = sqrt(px * px + py * py);
    if (ln > 1e-3) {
        x += (0.25 * px) / ln;
        y += (0.25 * py) / ln;
    }
    x = fmax(0.0, fmin(x, (double)(W - 1)));
    y = fmax(0.0, fmin(y, (double)(H - 1)));
    const int rx = (int)rint(x), ry = (int)rint(y);                      // (the fraction is 0 or at most 0.25 either way: never a half)
    const float zs = cpn_pixel<L, PAIR>(z, zm, ry * W + rx, W, a.C);     // (PAIR: r0 is taken from the fused map -- both frames again)
    const float sc = zs / 255.0f + 0.5f;                                 // r0 = z / 255 + 0.5, both rounded to fp32
    const float xf = (float)x, yf = (float)y;
    const float kx = a.dec[0] * xf + a.dec[1], ky = a.dec[2] * yf + a.dec[3];      // (contraction is off: product rounded, then the sum)
    if constexpr (PAIR) {                                                // both sets of the stacks, the mirrored one at joint swap[j]
        write_pair_stacks(a.kcrop, a.k2d, a.score, o, om, a.k2d ? a.to_image + (size_t)b * 6 : nullptr, a.mirror_w, kx, ky, sc);
    } else {                                                             // (statement for statement what the single form always was)
        a.kcrop[o * 2] = kx;
        a.kcrop[o * 2 + 1] = ky;
        if (a.score) a.score[o] = sc;
        if (a.k2d) {
            const float* A = a.to_image + (size_t)b * 6;
            a.k2d[o * 2] = (A[0] * kx + A[1] * ky) + A[2];
            a.k2d[o * 2 + 1] = (A[3] * kx + A[4] * ky) + A[5];
        }
    }
}

template <class L, bool PAIR>
static hipError_t launch_cpn_decode_t(const typename CpnArgsOf<PAIR>::type& a, size_t lds, hipStream_t s) {
    static DynLdsAttr attr;
    const hipError_t e = attr.ensure(reinterpret_cast<const void*>(&cpn_decode_kernel<L, PAIR>), (int)CPN_LDS_LIMIT);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL((cpn_decode_kernel<L, PAIR>), dim3((unsigned)(a.B * a.J)), dim3(CPN_THREADS), lds, s, a);
    return hipGetLastError();
}

template <bool PAIR>
static hipError_t launch_cpn_decode_any(typename CpnArgsOf<PAIR>::type& a, hipStream_t s) {
    const size_t lds = cpn_decode_lds_bytes(a.H, a.W);
    if (!a.heat || !a.kcrop || a.B < 1 || a.J < 1 || a.J > a.C || a.C > MAX_JOINTS || lds > CPN_LDS_LIMIT || (long)a.B * a.J >= (1L << 31) ||
        (a.k2d && !a.to_image) || a.dtype < CAPF_F32 || a.dtype > CAPF_F16)
        return hipErrorInvalidValue;
    cpn_decode_taps(a.g);
    return with_map_loader(a.dtype, [&](auto l) { return launch_cpn_decode_t<decltype(l), PAIR>(a, lds, s); });
}

hipError_t launch_cpn_decode(CpnDecodeArgs a, hipStream_t s) { return launch_cpn_decode_any<false>(a, s); }

hipError_t launch_cpn_decode_pair(CpnPairArgs a, hipStream_t s) {
    if (!swap_table_ok(a.swap.j, a.J)) return hipErrorInvalidValue;      // (capf_cpn_decode_pair has judged the table; a kernel never indexes past it)
    return launch_cpn_decode_any<true>(a, s);
}

}  // namespace capf
