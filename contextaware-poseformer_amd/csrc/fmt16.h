// The two 16-bit element formats of the 16-bit kernel families -- bf16 and fp16 -- and everything in those kernels that depends on which
// one an element is.  Stand-alone (device code shared with the harnesses under tools/ includes it without kernels.h).
#pragma once
#include <hip/hip_runtime.h>

namespace capf {

// fp32 -> bf16, round to nearest even: gfx950 has the conversion in hardware (v_cvt_pk_bf16_f32, two values per instruction);
// the software form (5 integer ops per value) made the bf16 epilogues VALU-bound.  Host passes never call these.
__host__ __device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {          // lo in bits 0-15
#if defined(__HIP_DEVICE_COMPILE__)
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2_t{lo, hi}, bf16x2_t));
#else
    (void)lo; (void)hi;
    return 0u;
#endif
}
__host__ __device__ __forceinline__ unsigned short to_bf16(float f) { return (unsigned short)(pack_bf16x2(f, 0.f) & 0xFFFFu); }

// fp32 -> fp16 as every fp16 store of the 16-bit kernels does it: round to nearest even (v_cvt_pk_f16_f32 / v_cvt_f16_f32, not the
// round-toward-zero pack), finite values beyond +-65504 and the infinities saturate to +-65504 (an activation that outgrows the format
// stays a large finite number instead of poisoning every later layer with Inf - Inf), NaN stays NaN (fminf / fmaxf return the other
// operand for a NaN, hence the select).  Subnormal results are kept.  The host copy is the same expression (capf_debug_f16_round).
__host__ __device__ __forceinline__ float f16_saturate(float f) {
    const float c = fminf(fmaxf(f, -65504.f), 65504.f);
    return f != f ? f : c;
}
__host__ __device__ __forceinline__ unsigned short to_f16(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f16_saturate(f)); }
__host__ __device__ __forceinline__ float from_f16(unsigned short h) { return (float)__builtin_bit_cast(_Float16, h); }
__host__ __device__ __forceinline__ unsigned pack_f16x2(float lo, float hi) {           // lo in bits 0-15
    typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(unsigned, __builtin_convertvector(f32x2_t{f16_saturate(lo), f16_saturate(hi)}, f16x2_t));
}

// What the 16-bit kernel families (igemm_bf16*.hip, bneck_bf16.hip, the 16-bit paths of elementwise.hip and of the samplers) need to know
// about their element format; nothing else in them depends on it -- an element is two bytes in HBM, LDS and the LDS-DMA tiles, eight of
// them are one operand of v_mfma_f32_32x32x16_{bf16,f16}, and both instructions issue at the same rate.  Every kernel template takes one of
// these as its last parameter F; GemmArgs::f16 (and the f16 / format arguments of the other launchers) picks the instantiation on the host.
//   pack2(lo, hi)  two fp32 values -> one 32-bit word of two elements (lo in bits 0-15), the format's store rounding
//   narrow / widen one element;  lo(u) / hi(u): the two elements of a packed word, widened
//   mfma           D = A x B + C on the matrix pipe (operand order as the builtins take it)
typedef float fmt_f32x16 __attribute__((ext_vector_type(16)));
struct Bf16Fmt {
    static constexpr int code = 0;
    typedef __bf16 x8 __attribute__((ext_vector_type(8)));
    static __host__ __device__ __forceinline__ unsigned pack2(float lo, float hi) { return pack_bf16x2(lo, hi); }
    static __host__ __device__ __forceinline__ unsigned short narrow(float f) { return to_bf16(f); }
    static __device__ __forceinline__ float widen(unsigned short h) { return __uint_as_float((unsigned)h << 16); }
    static __device__ __forceinline__ float lo(unsigned u) { return __uint_as_float(u << 16); }
    static __device__ __forceinline__ float hi(unsigned u) { return __uint_as_float(u & 0xFFFF0000u); }
#if defined(__HIP_DEVICE_COMPILE__)
    static __device__ __forceinline__ fmt_f32x16 mfma(x8 a, x8 b, fmt_f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0); }
#endif
};
struct F16Fmt {
    static constexpr int code = 1;
    typedef _Float16 x8 __attribute__((ext_vector_type(8)));
    static __host__ __device__ __forceinline__ unsigned pack2(float lo, float hi) { return pack_f16x2(lo, hi); }
    static __host__ __device__ __forceinline__ unsigned short narrow(float f) { return to_f16(f); }
    static __device__ __forceinline__ float widen(unsigned short h) { return from_f16(h); }
    static __device__ __forceinline__ float lo(unsigned u) { return from_f16((unsigned short)(u & 0xFFFFu)); }
    static __device__ __forceinline__ float hi(unsigned u) { return from_f16((unsigned short)(u >> 16)); }
#if defined(__HIP_DEVICE_COMPILE__)
    static __device__ __forceinline__ fmt_f32x16 mfma(x8 a, x8 b, fmt_f32x16 c) { return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0); }
#endif
};
// a launch site names its kernel once: with_fmt(f16, [&](auto f) { using F = decltype(f); ... kernel<.., F> ... }) runs the body for the
// format a code stands for (0 bf16, 1 fp16)
template <class Fn>
inline auto with_fmt(int f16, Fn&& fn) { return f16 ? fn(F16Fmt{}) : fn(Bf16Fmt{}); }
// How a kernel that takes an activation map in any capf_dtype (the keypoint head, CPN's decode) reads it: one element, or four consecutive
// ones in one load, widened to fp32.  T is the element as it lies in memory; the loaders hold no arithmetic.
typedef float fmt_f32x4 __attribute__((ext_vector_type(4)));
struct MapLdF32 {
    typedef float T;
    static __device__ __forceinline__ fmt_f32x4 ld4(const T* p) { return *reinterpret_cast<const fmt_f32x4*>(p); }
    static __device__ __forceinline__ float ld1(const T* p) { return *p; }
};
template <class F>
struct MapLd16 {
    typedef unsigned short T;
    static __device__ __forceinline__ fmt_f32x4 ld4(const T* p) {
        const uint2 u = *reinterpret_cast<const uint2*>(p);
        return fmt_f32x4{F::lo(u.x), F::hi(u.x), F::lo(u.y), F::hi(u.y)};
    }
    static __device__ __forceinline__ float ld1(const T* p) { return F::widen(*p); }
};
// ... and its launch site: with_map_loader(dtype, [&](auto l) { using L = decltype(l); ... kernel<L, ..> ... }) runs the body for the loader
// of a capf_dtype code (0 fp32, 1 bf16, 2 fp16; the caller has refused every other code)
template <class Fn>
inline auto with_map_loader(int dtype, Fn&& fn) {
    if (dtype == 0) return fn(MapLdF32{});
    if (dtype == 1) return fn(MapLd16<Bf16Fmt>{});
    return fn(MapLd16<F16Fmt>{});
}
// a 16-bit kernel's reported name for a format: the bf16 name as it is, or with every "bf16" replaced by "f16" (interned, never freed)
const char* fmt_kernel_name(const char* bf16_name, int f16);

}  // namespace capf
