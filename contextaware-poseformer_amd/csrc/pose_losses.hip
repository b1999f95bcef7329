// The pose losses of ContextPose/mvn/models/loss.py that metrics.hip does not carry, each with its gradient:
//   KeypointsL2Loss  loss.py:140-147   (validity-masked mean of per-row Euclidean distances)
//   LimbLengthError  loss.py:181-201   (mean absolute difference of bone lengths over a table of limbs)
//   UNCERTAINTY      loss.py:7-13      (residual scaled by predicted sigmas + 0.01 mean log sigma)
// The reference's KeypointsL2Loss has no usable gradient at its singular points (sqrt at 0: NaN as soon as one row is masked or hit
// exactly) and LimbLengthError has none at all (it returns a Python float after sixteen .cpu() calls).  Here every gradient is defined:
// 0 where the norm or square root it divides by is 0, capf_mpjpe's rule (train_kernels.hip).
//
// Arithmetic: fp64 from the fp32 inputs, every operation rounded on its own (no contraction), one fp32 store per output element; sums
// in fixed orders, no atomics -- the same bits on every call, and a float64 restatement (tests/loss_extra_cases.py) is one store away.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace capf {

// sum of the N per-thread values of one block of N threads, fixed tree; every thread returns the total
template <int N>
__device__ inline double block_sum(double v, double* red) {
    const int t = threadIdx.x;
    __syncthreads();                      // (red may still be read from the previous sum)
    red[t] = v;
    __syncthreads();
    for (int o = N / 2; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    return red[0];
}

// KeypointsL2Loss: thread t takes rows t, t + 1024, ... in order.  One block, like keypoints_loss_kernel.
__global__ __launch_bounds__(1024) void keypoints_l2_loss_kernel(const float* __restrict__ pred, const float* __restrict__ gt,
                                                                 const float* __restrict__ val, int rows, int D, float* __restrict__ loss,
                                                                 float* __restrict__ dpred, float gscale) {
#pragma clang fp contract(off)
    __shared__ double red[1024];
    const int t = threadIdx.x;
    double v = 0.0;
    for (int r = t; r < rows; r += 1024) v += (double)val[r];
    const double denom = fmax(1.0, block_sum<1024>(v, red));         // max(1, sum(validity)), loss.py:146
    double acc = 0.0;
    for (int r = t; r < rows; r += 1024) {
        const float* p = pred + (size_t)r * D;
        const float* g = gt + (size_t)r * D;
        double d2 = 0.0;
        for (int c = 0; c < D; ++c) {
            const double d = (double)g[c] - (double)p[c];
            d2 = d2 + d * d;
        }
        const double w = (double)val[r];
        const double s = sqrt(w * d2);                              // sqrt(sum((gt - pred)^2 * validity)), :145
        acc += s;
        if (dpred) {
            // d sqrt(w d2) / dpred = w (pred - gt) / sqrt(w d2); exactly 0 at s == 0 (a masked row, an exact hit), where autograd gives NaN
            const bool live = s > 0.0;
            const double k = live ? (double)gscale * w / (s * denom) : 0.0;
            for (int c = 0; c < D; ++c) dpred[(size_t)r * D + c] = live ? (float)(k * ((double)p[c] - (double)g[c])) : 0.f;
        }
    }
    const double total = block_sum<1024>(acc, red);
    if (t == 0) loss[0] = (float)(total / denom);
}

hipError_t launch_keypoints_l2_loss(const float* pred, const float* gt, const float* validity, int rows, int D, float* loss, float* dpred,
                                    float gscale, hipStream_t s) {
    if (rows <= 0 || D <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(keypoints_l2_loss_kernel, dim3(1), dim3(1024), 0, s, pred, gt, validity, rows, D, loss, dpred, gscale);
    return hipGetLastError();
}

// length of limb (a, b) of one pose and its difference vector x[a] - x[b]
__device__ inline double limb_vector(const float* __restrict__ x, int a, int b, double d[3]) {
#pragma clang fp contract(off)
    for (int c = 0; c < 3; ++c) d[c] = (double)x[a * 3 + c] - (double)x[b * 3 + c];
    return sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
}

// LimbLengthError per pose, one pose per thread (pose_errors_kernel's shape).  The limb table is uniform over the grid (kernel
// arguments): the gradient of joint j gathers, in limb order, the limbs whose table entry names j -- a branch every lane takes alike --
// into three registers and stores them once.  No atomics, no scatter.
__global__ __launch_bounds__(128) void limb_length_errors_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int n, int J,
                                                                 LimbTable limbs, int L, float* __restrict__ err, float* __restrict__ dpred,
                                                                 float gscale) {
#pragma clang fp contract(off)
    const long i = (long)blockIdx.x * 128 + threadIdx.x;
    if (i >= n) return;
    const float* P = pred + (size_t)i * J * 3;
    const float* G = gt + (size_t)i * J * 3;
    for (int l = 0; l < L; ++l) {
        double d[3];
        const int a = limbs.a[l], b = limbs.b[l];
        const double lp = limb_vector(P, a, b, d), lg = limb_vector(G, a, b, d);
        err[(size_t)i * L + l] = (float)fabs(lp - lg);              // torch.abs(limb_length_pred - limb_length_gt), :199
    }
    if (!dpred) return;
    float* dp = dpred + (size_t)i * J * 3;
    for (int j = 0; j < J; ++j) {
        double g[3] = {0.0, 0.0, 0.0};
        for (int l = 0; l < L; ++l) {
            const int a = limbs.a[l], b = limbs.b[l];
            if (a == b || (a != j && b != j)) continue;             // (a == b: a limb of length 0 by construction)
            double d[3], dg[3];
            const double lp = limb_vector(P, a, b, d), lg = limb_vector(G, a, b, dg);
            if (!(lp > 0.0)) continue;                              // coincident joints in pred: no direction, contributes 0
            const double sgn = lp > lg ? 1.0 : (lp < lg ? -1.0 : 0.0);
            const double w = (a == j ? sgn : -sgn) / lp;
            for (int c = 0; c < 3; ++c) g[c] += w * d[c];
        }
        for (int c = 0; c < 3; ++c) dp[j * 3 + c] = (float)((double)gscale * g[c]);
    }
}

hipError_t launch_limb_length_errors(const float* pred, const float* gt, int n, int J, const LimbTable& limbs, int L, float* err, float* dpred,
                                     float gscale, hipStream_t s) {
    if (n <= 0 || J <= 0 || J > MAX_JOINTS || L < 1 || L > LIMB_MAX) return hipErrorInvalidValue;
    for (int l = 0; l < L; ++l)
        if (limbs.a[l] >= J || limbs.b[l] >= J) return hipErrorInvalidValue;
    hipLaunchKernelGGL(limb_length_errors_kernel, dim3((unsigned)(((long)n + 127) / 128)), dim3(128), 0, s, pred, gt, n, J, limbs, L, err, dpred,
                       gscale);
    return hipGetLastError();
}

// One block per (segment, limb), pck_counts_kernel's shape: thread t of 256 adds poses t, t + 256, ... in order, then a fixed tree.
static constexpr int SUM_THREADS = 256;
__global__ __launch_bounds__(SUM_THREADS) void limb_length_sums_kernel(const float* __restrict__ err, const int* __restrict__ seg, int n, int L,
                                                               double* __restrict__ sums, long long* __restrict__ counts) {
    __shared__ double red[SUM_THREADS];
    __shared__ long long cnt[SUM_THREADS];
    const int sid = blockIdx.x / L, l = blockIdx.x - sid * L, t = threadIdx.x;
    double a = 0.0;
    long long c = 0;
    for (long i = t; i < n; i += SUM_THREADS) {
        if (seg && seg[i] != sid) continue;
        ++c;
        a += (double)err[(size_t)i * L + l];
    }
    red[t] = a;
    cnt[t] = c;
    __syncthreads();
    for (int o = SUM_THREADS / 2; o > 0; o >>= 1) {
        if (t < o) { red[t] += red[t + o]; cnt[t] += cnt[t + o]; }
        __syncthreads();
    }
    if (t == 0) {
        sums[(size_t)sid * L + l] = red[0];
        if (l == 0) counts[sid] = cnt[0];
    }
}

hipError_t launch_limb_length_sums(const float* err, const int* seg, int n, int L, int n_seg, double* sums, long long* counts, hipStream_t s) {
    if (n <= 0 || L < 1 || L > LIMB_MAX || n_seg <= 0 || (long)n_seg * L > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(limb_length_sums_kernel, dim3(n_seg * L), dim3(SUM_THREADS), 0, s, err, seg, n, L, sums, counts);
    return hipGetLastError();
}

// UNCERTAINTY: thread t takes rows t, t + 512, ... in order; per row the residual is read once for all K sigmas (and once more, from
// cache, for the gradients).  s = sigma + 1e-6 in fp64.  One block of 512 threads: the eight norms, log sums and [rows, 1] gradient sums of a
// row live in registers, which 1024 threads a block would not leave room for.
static constexpr int UNC_THREADS = 512;
__global__ __launch_bounds__(UNC_THREADS) void uncertainty_loss_kernel(const float* __restrict__ pred, const float* __restrict__ gt, int rows, int D,
                                                                UncertaintySigmas sg, int K, float* __restrict__ loss, float* __restrict__ dpred,
                                                                float gscale) {
#pragma clang fp contract(off)
    constexpr int MK = UNCERTAINTY_MAX_SIGMAS;
    __shared__ double red[UNC_THREADS];
    const int t = threadIdx.x;
    const double inv_rows = 1.0 / (double)rows, nan = __builtin_nan("");
    bool any_grad = dpred != nullptr;
#pragma unroll
    for (int k = 0; k < MK; ++k) any_grad = any_grad || (k < K && sg.dsigma[k] != nullptr);
    double acc = 0.0;
    for (int r = t; r < rows; r += UNC_THREADS) {
        const float* p = pred + (size_t)r * D;
        const float* g = gt + (size_t)r * D;
        double q[MK], lg[MK];
        unsigned bad = 0;                                           // bit k: sigma k has an s <= 0 (or NaN) in this row
#pragma unroll
        for (int k = 0; k < MK; ++k) q[k] = lg[k] = 0.0;
        for (int c = 0; c < D; ++c) {
            const double d = (double)p[c] - (double)g[c];
#pragma unroll
            for (int k = 0; k < MK; ++k) {
                if (k >= K) continue;
                const int w = sg.width[k];
                const double s = (double)sg.sigma[k][(size_t)r * w + (w == 1 ? 0 : c)] + 1e-6;
                const double u = d / s;
                q[k] += u * u;
                if (w != 1 || c == 0) lg[k] += log(s);
                if (!(s > 0.0)) bad |= 1u << k;
            }
        }
        double row = 0.0;
#pragma unroll
        for (int k = 0; k < MK; ++k) {
            if (k >= K) continue;
            q[k] = sqrt(q[k]);                                      // torch.norm(diff / (sigma + 1e-6), dim=-1), :11
            row += q[k] * inv_rows + 0.01 * (lg[k] / ((double)rows * (double)sg.width[k]));
        }
        acc += bad ? nan : row;                                     // the reference's log(s <= 0); not clamped
        if (!any_grad) continue;
        double ds1[MK];
#pragma unroll
        for (int k = 0; k < MK; ++k) ds1[k] = 0.0;
        for (int c = 0; c < D; ++c) {
            const double d = (double)p[c] - (double)g[c];
            double dp = 0.0;
#pragma unroll
            for (int k = 0; k < MK; ++k) {
                if (k >= K) continue;
                const int w = sg.width[k];
                const double s = (double)sg.sigma[k][(size_t)r * w + (w == 1 ? 0 : c)] + 1e-6;
                const double u = d / s;
                const double dn = q[k] > 0.0 ? u / (s * q[k]) : 0.0;   // d|u| / dpred[c]; 0 at |u| == 0
                dp += dn;
                const double dsn = -(u * dn);                       // d|u| / ds = -u^2 / (s |u|)
                if (w == 1) {
                    ds1[k] += dsn;
                } else if (sg.dsigma[k]) {
                    const double v = (double)gscale * (dsn * inv_rows + 0.01 / ((double)rows * (double)D) / s);
                    sg.dsigma[k][(size_t)r * D + c] = (bad >> k & 1u) ? (float)nan : (float)v;
                }
            }
            if (dpred) dpred[(size_t)r * D + c] = bad ? (float)nan : (float)((double)gscale * (dp * inv_rows));
        }
#pragma unroll
        for (int k = 0; k < MK; ++k) {
            if (k >= K || sg.width[k] != 1 || !sg.dsigma[k]) continue;
            const double s = (double)sg.sigma[k][r] + 1e-6;
            const double v = (double)gscale * (ds1[k] * inv_rows + 0.01 * inv_rows / s);
            sg.dsigma[k][r] = (bad >> k & 1u) ? (float)nan : (float)v;
        }
    }
    const double total = block_sum<UNC_THREADS>(acc, red);
    if (t == 0) loss[0] = (float)total;
}

hipError_t launch_uncertainty_loss(const float* pred, const float* gt, int rows, int D, const UncertaintySigmas& sg, int K, float* loss,
                                   float* dpred, float gscale, hipStream_t s) {
    if (rows <= 0 || D <= 0 || K < 1 || K > UNCERTAINTY_MAX_SIGMAS) return hipErrorInvalidValue;
    for (int k = 0; k < K; ++k)
        if (!sg.sigma[k] || (sg.width[k] != D && sg.width[k] != 1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(uncertainty_loss_kernel, dim3(1), dim3(UNC_THREADS), 0, s, pred, gt, rows, D, sg, K, loss, dpred, gscale);
    return hipGetLastError();
}

}  // namespace capf
