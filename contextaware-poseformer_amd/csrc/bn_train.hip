// Training-mode BatchNorm2d over a raw conv output (gfx950): batch statistics in two launches, then one normalise / residual / ReLU pass.
// All tensors NHWC fp32, seen as [rows = B * H * W][C]; C % 4 == 0, C <= 1024; every lane moves 16 bytes, consecutive lanes consecutive addresses.
//
// Statistics, no atomics, one fixed summation order (the same input gives the same bits on every run):
//   stage 1  a block owns a slab of `slab_rows` consecutive rows.  Thread (r, g) of the block -- 256 / (C / 4) row slots r, C / 4 four-channel
//            groups g -- walks rows r, r + R, ... of the slab and keeps, per channel, the count and the fp32 sums of d = x - k and d * d, k being
//            the FIRST value the thread saw: a few dozen values at most, shifted by one of them, so a channel whose mean is far above its spread
//            cancels nothing.  The thread's (n, mean, M2) go through LDS as fp64; thread (0, g) combines the R row slots in ascending r
//            (N = sum n, mean = sum n mean_i / N, M2 = sum M2_i + sum n_i (mean_i - mean)^2) and writes the slab's mean and M2 as fp64.
//   stage 2  a SEPARATE launch (an in-launch hand-off between blocks would cross eight non-coherent L2s): 16 channels x 16 parts per block; part q
//            combines slabs q, q + 16, ... in ascending order, the parts in ascending q, in fp64 (bn_stats_final has the formulas).  It writes
//            scale = gamma / sqrt(var + eps), shift = beta - mean * scale and, where given, the running statistics
//            (running_mean <- (1 - m) running_mean + m mean;  running_var <- (1 - m) running_var + m var n / (n - 1)).
// Apply: y = act(fma(x, scale[c], shift[c]) + residual), in place allowed; ReLU as relu_f (a NaN stays a NaN).
// Grouped forms: up to 4 independent BatchNorms (the branches of an HRNet level) in one grid, as fuse_sum_group_kernel has.
#include "kernels.h"

namespace capf {

typedef float f32x4 __attribute__((ext_vector_type(4)));

static constexpr int BN_THREADS = 256;
static constexpr int BN_PARTS = BN_THREADS / 16;      // stage 2: parts per channel

int bn_slab_rows(long rows, int C) {
    const int R = BN_THREADS / (C / 4);
    long per = (rows + BN_MAX_SLABS - 1) / BN_MAX_SLABS;
    if (per < 4L * R) per = 4L * R;
    return (int)((per + R - 1) / R * R);
}
int bn_num_slabs(long rows, int C) {
    const int sr = bn_slab_rows(rows, C);
    return (int)((rows + sr - 1) / sr);
}
size_t bn_scratch_elems(long rows, int C) {            // floats: [nslab][2][C] fp64
    if (rows < 1 || C < 4 || C % 4 != 0 || C > 1024 || rows * (long)(C / 4) >= (1L << 31)) return 0;
    return (size_t)bn_num_slabs(rows, C) * 2 * (size_t)C * 2;
}

__device__ __forceinline__ void bn_stats_slab(const BnStatsArgs& a, const int slab) {
    __shared__ double sh_mean[BN_THREADS][4];
    __shared__ double sh_m2[BN_THREADS][4];
    __shared__ int sh_n[BN_THREADS];
    const int C4 = a.C >> 2, R = BN_THREADS / C4;
    const int tid = threadIdx.x, r = tid / C4, g = tid - r * C4;
    const long r0 = (long)slab * a.slab_rows;
    const long r1 = r0 + a.slab_rows < a.rows ? r0 + a.slab_rows : a.rows;
    int n = 0;
    f32x4 k = {0.f, 0.f, 0.f, 0.f}, s1 = k, s2 = k;
    if (r < R && r0 + r < r1) {
        const f32x4* x = reinterpret_cast<const f32x4*>(a.x) + g;
        k = x[(r0 + r) * C4];
#pragma unroll 4
        for (long row = r0 + r; row < r1; row += R) {
            const f32x4 d = x[row * C4] - k;
            s1 += d;
            s2 += d * d;
            ++n;
        }
    }
    sh_n[tid] = n;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const double dn = n > 0 ? (double)n : 1.0, d1 = (double)s1[e], d2 = (double)s2[e];
        sh_mean[tid][e] = (double)k[e] + d1 / dn;
        sh_m2[tid][e] = d2 - d1 * d1 / dn;
    }
    __syncthreads();
    if (tid >= C4) return;
    double N = 0.0, mean[4] = {0.0, 0.0, 0.0, 0.0}, m2[4] = {0.0, 0.0, 0.0, 0.0};
    for (int q = 0; q < R; ++q) {                       // ascending row slot: one order
        const double nq = (double)sh_n[q * C4 + g];
        N += nq;
#pragma unroll
        for (int e = 0; e < 4; ++e) mean[e] += nq * sh_mean[q * C4 + g][e];
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) mean[e] /= N;           // (N >= 1: a slab holds at least one row)
    for (int q = 0; q < R; ++q) {
        const double nq = (double)sh_n[q * C4 + g];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const double d = sh_mean[q * C4 + g][e] - mean[e];
            m2[e] += sh_m2[q * C4 + g][e] + nq * d * d;
        }
    }
    double* pm = a.part + ((size_t)slab * 2) * a.C + g * 4;
#pragma unroll
    for (int e = 0; e < 4; ++e) { pm[e] = mean[e]; pm[a.C + e] = m2[e]; }
}

// Stage 2 for 16 channels: 16 parts x 16 channels per block.  Part q sums slabs q, q + 16, ... in ascending order, the parts are added in
// ascending q.  One pass, in fp64, shifted by k = the mean of slab 0 (an estimate of the mean good to the slab-to-slab variation, so the
// subtraction below cancels nothing that fp64 does not hold):  S1 = sum n_i (m_i - k),  S2 = sum M2_i + n_i (m_i - k)^2,
// mean = k + S1 / N,  M2 = S2 - S1^2 / N
__device__ __forceinline__ void bn_stats_final(const BnStatsArgs& a, const int cblock) {
    __shared__ double sh1[BN_PARTS][16], sh2[BN_PARTS][16];
    const int lc = threadIdx.x & 15, q = threadIdx.x >> 4;
    const int c = cblock * 16 + lc;
    const int cc = c < a.C ? c : a.C - 1;               // (lanes beyond C compute a copy and write nothing)
    const double N = (double)a.rows;
    const double* __restrict__ part = a.part;
    const double k = part[cc];
    const double n_full = (double)a.slab_rows, n_last = (double)(a.rows - (long)(a.nslab - 1) * a.slab_rows);
    double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
    for (int sl = q; sl < a.nslab; sl += BN_PARTS) {
        const double n = sl == a.nslab - 1 ? n_last : n_full;
        const double d = part[((size_t)sl * 2) * a.C + cc] - k;
        s1 += n * d;
        s2 += part[((size_t)sl * 2 + 1) * a.C + cc] + n * d * d;
    }
    sh1[q][lc] = s1;
    sh2[q][lc] = s2;
    __syncthreads();
    if (q != 0 || c >= a.C) return;
    s1 = s2 = 0.0;
    for (int p = 0; p < BN_PARTS; ++p) { s1 += sh1[p][lc]; s2 += sh2[p][lc]; }
    const double mean = k + s1 / N;
    const double m2 = s2 - s1 * s1 / N;
    const double var = m2 / N;                          // biased: what normalises
    const double scale = (double)a.gamma[c] / sqrt(var + (double)a.eps);
    a.scale[c] = (float)scale;
    a.shift[c] = (float)((double)a.beta[c] - mean * scale);
    const double m = (double)a.momentum;
    if (a.rmean) a.rmean[c] = (float)((1.0 - m) * (double)a.rmean[c] + m * mean);
    if (a.rvar) a.rvar[c] = (float)((1.0 - m) * (double)a.rvar[c] + m * (m2 / (N - 1.0)));     // unbiased: what is tracked
}

__device__ __forceinline__ void bn_apply_body(const BnApplyArgs& a, const long first, const long stride) {
    const int C4 = a.C >> 2;
    const long total = a.rows * C4;
    if (first >= total) return;
    const int g = (int)(first % C4);                    // stride % C4 == 0 (launcher): a thread stays on its four channels
    const f32x4 sc = reinterpret_cast<const f32x4*>(a.scale)[g], sf = reinterpret_cast<const f32x4*>(a.shift)[g];
    const f32x4* x = reinterpret_cast<const f32x4*>(a.x);
    const f32x4* res = reinterpret_cast<const f32x4*>(a.res);
    f32x4* y = reinterpret_cast<f32x4*>(a.y);
    for (long i = first; i < total; i += stride) {
        const f32x4 v = x[i];
        f32x4 t;
#pragma unroll
        for (int e = 0; e < 4; ++e) t[e] = fmaf(v[e], sc[e], sf[e]);
        if (res) t += res[i];
        if (a.act) {
#pragma unroll
            for (int e = 0; e < 4; ++e) t[e] = relu_f(t[e]);
        }
        y[i] = t;
    }
}

struct BnStatsGroup { BnStatsArgs p[4]; int bstart[5]; int n; };
struct BnApplyGroup { BnApplyArgs p[4]; int bstart[5]; int n; };

template <class G>
__device__ __forceinline__ int bn_group_problem(const G& g) {
    int pi = 0;
#pragma unroll
    for (int i = 1; i < 4; ++i)
        if (i < g.n && (int)blockIdx.x >= g.bstart[i]) pi = i;
    return pi;
}

__global__ void __launch_bounds__(BN_THREADS) bn_stats_slab_kernel(BnStatsGroup g) {
    const int pi = bn_group_problem(g);
    bn_stats_slab(g.p[pi], (int)blockIdx.x - g.bstart[pi]);
}
__global__ void __launch_bounds__(BN_THREADS) bn_stats_final_kernel(BnStatsGroup g) {
    const int pi = bn_group_problem(g);
    bn_stats_final(g.p[pi], (int)blockIdx.x - g.bstart[pi]);
}
__global__ void __launch_bounds__(BN_THREADS) bn_apply_kernel(BnApplyGroup g) {
    const int pi = bn_group_problem(g);
    const int nb = g.bstart[pi + 1] - g.bstart[pi];
    bn_apply_body(g.p[pi], (long)((int)blockIdx.x - g.bstart[pi]) * BN_THREADS + threadIdx.x, (long)nb * BN_THREADS);
}

static bool bn_shape_ok(long rows, int C) { return rows >= 1 && rows * (long)(C / 4) < (1L << 31) && C >= 4 && C % 4 == 0 && C <= 1024; }

// n <= 4 BatchNorms: slab statistics, then -- a launch of its own -- their combination, scale / shift and the running statistics
hipError_t launch_bn_stats_group(const BnStatsArgs* a, int n, hipStream_t s) {
    if (n < 1 || n > 4) return hipErrorInvalidValue;
    BnStatsGroup g1{}, g2{};
    g1.n = g2.n = n;
    int b1 = 0, b2 = 0;
    for (int i = 0; i < n; ++i) {
        // rows < 2: "Expected more than 1 value per channel when training"
        if (!bn_shape_ok(a[i].rows, a[i].C) || a[i].rows < 2 || !a[i].x || !a[i].gamma || !a[i].beta || !a[i].part || !a[i].scale || !a[i].shift) return hipErrorInvalidValue;
        BnStatsArgs p = a[i];
        p.slab_rows = bn_slab_rows(p.rows, p.C);
        p.nslab = bn_num_slabs(p.rows, p.C);
        g1.p[i] = g2.p[i] = p;
        g1.bstart[i] = b1; b1 += p.nslab;
        g2.bstart[i] = b2; b2 += (p.C + 15) / 16;
    }
    for (int i = n; i < 5; ++i) { g1.bstart[i] = b1; g2.bstart[i] = b2; }
    hipLaunchKernelGGL(bn_stats_slab_kernel, dim3(b1), dim3(BN_THREADS), 0, s, g1);
    hipLaunchKernelGGL(bn_stats_final_kernel, dim3(b2), dim3(BN_THREADS), 0, s, g2);
    return hipGetLastError();
}

hipError_t launch_bn_apply_group(const BnApplyArgs* a, int n, hipStream_t s) {
    if (n < 1 || n > 4) return hipErrorInvalidValue;
    BnApplyGroup g{};
    g.n = n;
    int blocks = 0;
    for (int i = 0; i < n; ++i) {
        if (!bn_shape_ok(a[i].rows, a[i].C) || !a[i].x || !a[i].y || !a[i].scale || !a[i].shift) return hipErrorInvalidValue;
        const int C4 = a[i].C / 4;
        int m = C4;                                     // blocks in multiples of m: (m * 256) % C4 == 0
        for (int k = 0; k < 8 && m % 2 == 0; ++k) m /= 2;
        const long total = a[i].rows * C4;
        long want = (total + BN_THREADS - 1) / BN_THREADS;
        if (want > 8192) want = 8192;
        want = (want + m - 1) / m * m;
        g.p[i] = a[i];
        g.bstart[i] = blocks;
        blocks += (int)want;
    }
    for (int i = n; i < 5; ++i) g.bstart[i] = blocks;
    hipLaunchKernelGGL(bn_apply_kernel, dim3(blocks), dim3(BN_THREADS), 0, s, g);
    return hipGetLastError();
}

}  // namespace capf
