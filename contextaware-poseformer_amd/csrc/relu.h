// ReLU of the conv / GEMM epilogues (shared by kernels.h and the stand-alone tile headers).
#pragma once
#include <hip/hip_runtime.h>

namespace capf {

// ReLU as torch computes it: a NaN stays a NaN.  fmaxf alone returns 0 for one, which hid a poisoned input (one NaN pixel) from the
// context maps, the loss and the optimizer's non-finite guard (train.py:194).  Every other value keeps fmaxf(t, 0)'s bits.
__host__ __device__ __forceinline__ float relu_f(float t) { return t != t ? t : fmaxf(t, 0.f); }

}  // namespace capf
