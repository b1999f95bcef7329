// The step just before the hot path and the step just after it, each as one
// launch instead of the reference's dozen elementwise ops:
//   preprocess_*  — data_prefetcher.preload, ContextPose/mvn/datasets/utils.py:33-82: uint8 BGR crop ->
//                   normalised fp32 RGB NHWC (channel flip :45, /255 - mean (/ std) :47-50), root-relative
//                   ground truth (:52-53), optional train-time horizontal flip with left/right joint swap
//                   (:55-65) or flip-test stacking of the original and the mirrored sample (:67-80);
//   fliptest_fuse — ContextPose/train.py:177-180 (H36M) and ContextPose_mpi/run_3dhp.py:169-180 (3DHP, the caller's
//                   swap table): un-mirror the second prediction and average.
// Same fp32 operation order as the reference as it runs on a GPU ((u * (1/255) - mean) / std; 192 - x - 1), so
// results are bit-identical to the torch expressions.  Built with -ffp-contract=off.
#include "kernels.h"
#include "warp_rule.h"
#include "pixel_rule.h"

namespace capf {

// H36M skeleton: joints_left / joints_right of mvn/datasets/utils.py:12-13 as a swap table (launch_fliptest_fuse holds a host copy)
__device__ __constant__ int kSwap[17] = {0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13};

// out[s, b, h, w, c] for s in {0 (as is), 1 (mirrored along W)}; `mirror_first` mirrors sample 0 (train flip)
__global__ void preprocess_images_kernel(const unsigned char* __restrict__ in, float* __restrict__ out, int B, int H, int W,
                                         float m0, float m1, float m2, float s0, float s1, float s2, int use_std,
                                         int nsets, int mirror_first) {
    const long npix = (long)B * H * W;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < npix * nsets; i += (long)gridDim.x * blockDim.x) {
        const int set = (int)(i / npix);
        const long pix = i - (long)set * npix;
        const int w = (int)(pix % W);
        const long row = pix / W;
        const bool mirror = set == 1 || (set == 0 && mirror_first);
        const long src = (row * W + (mirror ? W - 1 - w : w)) * 3;
        // BGR in memory; the arithmetic is pixel_rule.h's, shared with the stem kernels' uint8 forms and with capf_input_rule_host
        const float mean[3] = {m0, m1, m2}, stdv[3] = {s0, s1, s2};
        float* o = out + i * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = pixel_rule(in[src + 2 - c], c, mean, use_std ? stdv : nullptr);
    }
}

// keypoints / ground truth: one thread per (set, b, joint)
__global__ void preprocess_points_kernel(const float* __restrict__ gt_in, float* __restrict__ gt_out,
                                         const float* __restrict__ k2d_in, float* __restrict__ k2d_out,
                                         const float* __restrict__ kc_in, float* __restrict__ kc_out, int B, int nsets,
                                         int mirror_first) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nsets * B * 17) return;
    const int j = t % 17, b = (t / 17) % B, set = t / (17 * B);
    const bool mirror = set == 1 || (set == 0 && mirror_first);
    const int js = mirror ? kSwap[j] : j;            // value written at joint j comes from joint js
    {
        const float* s = k2d_in + ((long)b * 17 + js) * 2;
        float* d = k2d_out + (((long)set * B + b) * 17 + j) * 2;
        d[0] = mirror ? -s[0] : s[0];
        d[1] = s[1];
    }
    {
        const float* s = kc_in + ((long)b * 17 + js) * 2;
        float* d = kc_out + (((long)set * B + b) * 17 + j) * 2;
        d[0] = mirror ? __fsub_rn(__fsub_rn(192.0f, s[0]), 1.0f) : s[0];
        d[1] = s[1];
    }
    if (set == 0 && gt_in) {     // root-relative ground truth (only the train flip mirrors it)
        const float* root = gt_in + (long)b * 17 * 3;
        const float* s = gt_in + ((long)b * 17 + js) * 3;
        float* d = gt_out + ((long)b * 17 + j) * 3;
        float x = js == 0 ? 0.f : __fsub_rn(s[0], root[0]);
        const float y = js == 0 ? 0.f : __fsub_rn(s[1], root[1]);
        const float z = js == 0 ? 0.f : __fsub_rn(s[2], root[2]);
        if (mirror_first) x = -x;
        d[0] = x; d[1] = y; d[2] = z;
    }
}

hipError_t launch_preprocess(const unsigned char* images_bgr, int B, int H, int W, const float mean[3], const float* stdv,
                             int mode, float* images_out, const float* gt_in, float* gt_out, const float* k2d_in,
                             float* k2d_out, const float* kc_in, float* kc_out, hipStream_t s) {
    const int nsets = mode == 2 ? 2 : 1, mirror_first = mode == 1 ? 1 : 0;
    const long n = (long)B * H * W * nsets;
    const long want = (n + 255) / 256;
    hipLaunchKernelGGL(preprocess_images_kernel, dim3((unsigned)(want < 8192 ? want : 8192)), dim3(256), 0, s, images_bgr,
                       images_out, B, H, W, mean[0], mean[1], mean[2], stdv ? stdv[0] : 1.f, stdv ? stdv[1] : 1.f,
                       stdv ? stdv[2] : 1.f, stdv ? 1 : 0, nsets, mirror_first);
    return launch_preprocess_points(B, mode, gt_in, gt_out, k2d_in, k2d_out, kc_in, kc_out, s);
}

// the points half alone (the image-less route: capf_forward_u8 reads the crop itself, the keypoints still want their mirror / stacking)
hipError_t launch_preprocess_points(int B, int mode, const float* gt_in, float* gt_out, const float* k2d_in, float* k2d_out,
                                    const float* kc_in, float* kc_out, hipStream_t s) {
    const int nsets = mode == 2 ? 2 : 1, mirror_first = mode == 1 ? 1 : 0;
    const int np = nsets * B * 17;
    hipLaunchKernelGGL(preprocess_points_kernel, dim3((np + 127) / 128), dim3(128), 0, s, gt_in, gt_out, k2d_in, k2d_out, kc_in,
                       kc_out, B, nsets, mirror_first);
    return hipGetLastError();
}

// out[b, j, :] = 0.5 * (pred[0, b, j, :] + unmirror(pred[1, b, :, :])[j])     (train.py:177-180)
// (the swap table is kernels.h' SwapTable)
__global__ void fliptest_fuse_kernel(const float* __restrict__ pred2, float* __restrict__ out, int B, int J, SwapTable sw) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= B * J) return;
    const int j = t % J, b = t / J;
    const float* p = pred2 + ((long)b * J + j) * 3;
    const float* q = pred2 + (((long)B + b) * J + sw.j[j]) * 3;
    float* o = out + (long)t * 3;
    // torch.mean over a dim of size 2: ((0 + a) + b) / 2 -- the sum starts from +0, which shows in one case only: a = b = -0 gives +0
    o[0] = __fdiv_rn(__fadd_rn(__fadd_rn(0.0f, p[0]), -q[0]), 2.0f);
    o[1] = __fdiv_rn(__fadd_rn(__fadd_rn(0.0f, p[1]), q[1]), 2.0f);
    o[2] = __fdiv_rn(__fadd_rn(__fadd_rn(0.0f, p[2]), q[2]), 2.0f);
}

hipError_t launch_fliptest_fuse_swap(const float* pred2, int B, int J, const int* swap, float* out, hipStream_t s) {
    if (B <= 0 || !swap_table_ok(swap, J) || (long)B * J > 0x7fffffffL) return hipErrorInvalidValue;
    SwapTable sw{};
    for (int j = 0; j < J; ++j) sw.j[j] = swap[j];
    hipLaunchKernelGGL(fliptest_fuse_kernel, dim3((B * J + 127) / 128), dim3(128), 0, s, pred2, out, B, J, sw);
    return hipGetLastError();
}

// the H36M entry: kSwap's table through the same kernel
hipError_t launch_fliptest_fuse(const float* pred2, int B, float* out, hipStream_t s) {
    static const int h36m[17] = {0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13};
    return launch_fliptest_fuse_swap(pred2, B, 17, h36m, out, s);
}

// ---- N3: the per-frame affine crop (mvn/utils/img.py:16-69, human36m.py:281-302) ------------------------
// get_affine_transform with rot = 0, shift = 0: three float32 point pairs (centre, centre + (0, -(src_w-1)/2),
// and the 90-degree companion of img.py:11-13) -> the 2x3 double matrix cv2.getAffineTransform solves for.
// Host code; compiled without FMA contraction so that it rounds like the numpy expressions it restates.
static bool solve3(double a[3][4]) {      // Gaussian elimination with partial pivoting, in place; solution in a[i][3]
    for (int c = 0; c < 3; ++c) {
        int piv = c;
        for (int r = c + 1; r < 3; ++r)
            if (fabs(a[r][c]) > fabs(a[piv][c])) piv = r;
        if (a[piv][c] == 0.0) return false;
        for (int k = 0; k < 4; ++k) { const double t = a[c][k]; a[c][k] = a[piv][k]; a[piv][k] = t; }
        for (int r = c + 1; r < 3; ++r) {
            const double f = a[r][c] / a[c][c];
            for (int k = c; k < 4; ++k) a[r][k] -= f * a[c][k];
        }
    }
    for (int r = 2; r >= 0; --r) {
        double v = a[r][3];
        for (int k = r + 1; k < 3; ++k) v -= a[r][k] * a[k][3];
        a[r][3] = v / a[r][r];
    }
    return true;
}

bool affine_from_center_scale(const double center[2], const double scale[2], int out_w, int out_h, double M[6]) {
    const double src_w = scale[0] * 200.0;
    const float src_dir1 = (float)((src_w - 1) * -0.5), dst_dir1 = (float)((out_w - 1) * -0.5);
    float src[3][2], dst[3][2];
    src[0][0] = (float)center[0];
    src[0][1] = (float)center[1];
    src[1][0] = (float)(center[0] + 0.0);
    src[1][1] = (float)(center[1] + (double)src_dir1);
    const double dcx = (out_w - 1) * 0.5, dcy = (out_h - 1) * 0.5;
    dst[0][0] = (float)dcx;
    dst[0][1] = (float)dcy;
    dst[1][0] = (float)(dcx + 0.0);
    dst[1][1] = (float)(dcy + (double)dst_dir1);
    for (int w = 0; w < 2; ++w) {         // third point: b + (-(a-b).y, (a-b).x) in float32
        float (*p)[2] = w == 0 ? src : dst;
        const float dx = p[0][0] - p[1][0], dy = p[0][1] - p[1][1];
        p[2][0] = p[1][0] + (-dy);
        p[2][1] = p[1][1] + dx;
    }
    for (int row = 0; row < 2; ++row) {
        double a[3][4];
        for (int i = 0; i < 3; ++i) { a[i][0] = src[i][0]; a[i][1] = src[i][1]; a[i][2] = 1.0; a[i][3] = dst[i][row]; }
        if (!solve3(a)) return false;
        for (int k = 0; k < 3; ++k) M[row * 3 + k] = a[k][3];
    }
    return true;
}

// cv2.warpAffine(frame, M, (out_w, out_h), INTER_LINEAR, BORDER_CONSTANT 0) for 8-bit 3-channel frames: OpenCV's
// fixed-point pipeline (10-bit coordinates, 5-bit fractions, 15-bit weights) restated per output pixel.
// frames[b]: device pointer of frame b; dims[b] = {rows, cols, row pitch in bytes}; M[b]: forward 2x3 matrix.  The arithmetic itself is
// warp_rule.h's, shared with the crop-aware JPEG route and with the host rule that bounds what a crop reads.
__global__ void warp_affine_u8_kernel(const unsigned char* const* __restrict__ frames, const int* __restrict__ dims,
                                      const double* __restrict__ M, unsigned char* __restrict__ out, int B, int out_h, int out_w) {
    const long t = blockIdx.x * (long)blockDim.x + threadIdx.x;
    const long total = (long)B * out_h * out_w;
    if (t >= total) return;
    const int x = (int)(t % out_w);
    const int y = (int)((t / out_w) % out_h);
    const int b = (int)(t / ((long)out_w * out_h));
    const WarpMap w = warp_inverse(M + (long)b * 6);
    warp_affine_pixel<false>(frames[b], dims[b * 3 + 0], dims[b * 3 + 1], dims[b * 3 + 2], nullptr, w, x, y, out + t * 3);
}

hipError_t launch_warp_affine_u8(const unsigned char* const* frames, const int* dims, const double* M, unsigned char* out,
                                 int B, int out_h, int out_w, hipStream_t s) {
    const long total = (long)B * out_h * out_w;
    if (total <= 0) return hipSuccess;
    hipLaunchKernelGGL(warp_affine_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, frames, dims, M, out, B,
                       out_h, out_w);
    return hipGetLastError();
}

}  // namespace capf
