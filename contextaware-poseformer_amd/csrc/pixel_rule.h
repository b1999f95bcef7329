// N1: the normalisation rule of the input image (data_prefetcher.preload, ContextPose/mvn/datasets/utils.py:45-50) as __host__ __device__
// code, written once: preprocess_images_kernel expands a uint8 crop with it, the uint8 forms of the stem kernels (igemm_stem.hip:
// U8) fill their per-block value table with it, and capf_input_rule_host evaluates it on the host -- as warp_rule.h shares
// the crop's coordinate rule.
//
// Every step is a single rounded fp32 operation (contraction off, IEEE division), in the order of the torch expressions as they run on a
// GPU: `images / 255.0` with a Python scalar is a multiplication by the fp32 reciprocal (ATen div_true_kernel_cuda, CPU-scalar fast
// path); mean and std are tensors: a subtraction, then a true division.  So every caller gets the same bits, whatever flags its
// translation unit is built with.
#pragma once
#include <hip/hip_runtime.h>

namespace capf {

// byte `u` of RGB channel `c` -> ((float)u * (1 / 255) - mean[c]) (/ std[c]; stdv == nullptr: no division -- CPN, utils.py:49-50)
__host__ __device__ inline float pixel_rule(unsigned char u, int c, const float* mean, const float* stdv) {
#pragma clang fp contract(off)
    const float inv255 = 1.0f / 255.0f;
#if defined(__HIP_DEVICE_COMPILE__)
    float v = __fsub_rn(__fmul_rn((float)u, inv255), mean[c]);
    if (stdv) v = __fdiv_rn(v, stdv[c]);
#else
    float v = (float)u * inv255;
    v = v - mean[c];
    if (stdv) v = v / stdv[c];
#endif
    return v;
}

// The uint8 image a stem kernel's U8 form reads instead of GemmArgs::A (an extra kernel argument of those instantiations alone):
// img [Bsrc, H, W, 3] uint8, BGR in memory, any alignment.  Engine frame f, input row hi, column wi, RGB channel c is byte
//     ((bs * H + hi) * W + ws) * 3 + (2 - c),   bs = f (modes 0, 1) or f mod Bsrc (mode 2),
//     ws = W - 1 - wi where the frame is mirrored (mode 1: every frame; mode 2: frames f >= Bsrc), else wi
// -- capf_preprocess's modes, so that the conv sees the tensor capf_preprocess would have written.
struct U8Input {
    const unsigned char* img;
    int Bsrc, mode;
    float mean[3], stdv[3];
    int use_std;
};

static constexpr int U8_TAB = 3 * 256;       // floats of the per-block value table: tab[c * 256 + u] = pixel_rule(u, c)

#if defined(__HIPCC__)
// the table, by the whole block (nt threads); the caller's barrier comes before the first lookup
__device__ __forceinline__ void u8_fill_table(float* tab, const U8Input& in, int tid, int nt) {
    for (int i = tid; i < U8_TAB; i += nt) tab[i] = pixel_rule((unsigned char)(i & 255), i >> 8, in.mean, in.use_std ? in.stdv : nullptr);
}
// byte offset of pixel (hi, wi) of engine frame f (channel B); the caller has checked 0 <= hi < H, 0 <= wi < W, 0 <= f < frames
__device__ __forceinline__ long u8_pixel(const U8Input& in, int f, int hi, int wi, int H, int W) {
    const bool second = in.mode == 2 && f >= in.Bsrc;
    const int bs = second ? f - in.Bsrc : f;
    const int ws = (in.mode == 1 || second) ? W - 1 - wi : wi;
    return (((long)bs * H + hi) * W + ws) * 3;
}
// the normalised value of RGB channel c of that pixel (valid), or of nothing (0.0f: zero padding of the NORMALISED image).  An invalid
// tap reads byte 0 of the image and drops it: no branch, and no address outside [img, img + Bsrc * H * W * 3)
__device__ __forceinline__ unsigned u8_load(const U8Input& in, bool valid, long pixel, int c) {
    return in.img[valid ? pixel + (2 - c) : 0];
}
__device__ __forceinline__ float u8_value(const float* tab, bool valid, unsigned byte, int c) { return valid ? tab[c * 256 + byte] : 0.f; }
#endif

}  // namespace capf
