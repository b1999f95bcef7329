// The Cin = 3 stem convolution for gfx950: five kernels (two fp32, three 16-bit), each with a float form (the fp32 NHWC image at GemmArgs::A)
// and a U8 form (the uint8 BGR crop itself, pixel_rule.h U8Input), behind ONE route (gemm_stem_route), ONE launcher (launch_gemm_stem) and ONE
// name function (gemm_stem_kernel_name): the image source is an argument, so the uint8 form is the float form's route, kernel and bits by
// construction.
//
//   igemm_f32_smallc          fp32, any small Cin, k = 3 or 7: element-wise gather, 128 x 64 tiles
//   igemm_f32_stem_stream     fp32 3x3 / pad 1, Cout <= 64: persistent blocks, run loads in flight across the previous tile
//   igemm_bf16_smallc         16-bit result (bf16 / fp16: Bf16Fmt / F16Fmt), element-wise gather
//   igemm_bf16_stem           16-bit, 7x7 / 3x3: one contiguous run per (pixel, kh), whole K staged once
//   igemm_bf16_stem_stream    16-bit, persistent streaming form of the former
//
// The weights are the fp32 pack [N][Kpad], Kpad % 32 == 0, K order (kh, kw, c), for every one of them.
#include <stdio.h>
#include <stdlib.h>

#include <type_traits>

#include "kernels.h"

namespace capf {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
typedef __amdgpu_buffer_rsrc_t rsrc_t;

static constexpr int BK = 32;      // K chunk (floats) of the fp32 pack = 128 B per tile row

__device__ __forceinline__ long rowmap(const RowMap& r, int m) {
    if (r.G == 1) return (long)m * r.S1 + r.off;
    int q = m / r.G;
    return (long)q * r.S1 + (long)(m - q * r.G) * r.S2 + r.off;
}

// n / d for n < 2^31 with a host-computed (mul, shift): q = (umulhi(n, mul) + n) >> shift
__device__ __forceinline__ int fast_div(int n, FastDiv d) {
    return (int)((__umulhi((unsigned)n, d.mul) + (unsigned)n) >> d.shift);
}
__device__ __forceinline__ int fast_div_b(int n, FastDiv d) { return fast_div(n, d); }     // (the 16-bit bodies' name for it)

// XCD-aware tile order: physical block b runs on XCD b % 8; give each XCD a contiguous range of logical
// tiles (bijective for any grid size).
__device__ __forceinline__ int xcd_remap_b(int b, int nblk) {
    const int q = nblk >> 3, r = nblk & 7, x = b & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (b >> 3);
}

// =====================================================================================================
// Small-Cin (stem: Cin = 3, k = 3 or 7) variant: K is gathered element-wise into registers, staged with
// ds_write_b128 into a padded LDS tile (pitch 36 floats: conflict-free b128 without a swizzle).  0.3 % of
// the FLOPs of the path; kept simple.
// =====================================================================================================
static constexpr int PITCH = 36;

//
// U8 (every kernel of this file): the image is the uint8 BGR crop itself (pixel_rule.h U8Input: normalisation,
// BGR -> RGB, mirror and the flip-test frame mapping of capf_preprocess happen in this load).  The form differs from the float one ONLY in how
// a tap's value reaches the register that the float form fills from p.A: same tile, same K order, same MFMA sequence, hence the same bits as
// the float kernel on capf_preprocess's output.
//   * values: a per-block table tab[c][u] = pixel_rule(u, c) in LDS (3 KiB, 768 evaluations per block -- against one IEEE division per tap
//     and pixel, 27 / 147 per output pixel, in the gather): the same function as preprocess_images_kernel's, so the same bits by construction;
//   * bytes: one byte load per tap (global_load_ubyte in the ISA), each with its own validity -- a run of 9 / 21 bytes starts at any byte
//     offset of a base of any alignment, runs backwards pixel by pixel in a mirrored frame, and the first / last run of the tensor would
//     start before / end behind it: dword loads would have to be split at both ends or read outside the tensor.  An invalid tap reads byte 0
//     and drops it, so no load leaves [img, img + Bsrc H W 3) and none is behind a branch; padding is 0.0f AFTER normalisation;
//   * GemmArgs keeps its layout: the descriptor is an extra argument of the *_u8_kernel entry points alone (p.A is not read).
template <int BM, int BN, int WM, int WN, bool U8>
__device__ __forceinline__ void igemm_f32_smallc_body(const GemmArgs& p, const U8Input* u8) {
    constexpr int WAVES_N = BN / WN;
    constexpr int TM = WM / 32, TN = WN / 32;
    constexpr int RA = BM / 32, RB = BN / 32;
    static_assert((BM / WM) * (BN / WN) == 4, "4 waves per block");
    __shared__ __attribute__((aligned(16))) float lds[(BM + BN) * PITCH + (U8 ? U8_TAB : 0)];
    float* As = lds;
    float* Bs = lds + BM * PITCH;
    const float* tab = lds + (BM + BN) * PITCH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (U8) {
        u8_fill_table(lds + (BM + BN) * PITCH, *u8, tid, 256);
        __syncthreads();
    }
    const int nbn = (p.N + BN - 1) / BN;
    const int tile_m = blockIdx.x / nbn, tile_n = blockIdx.x - tile_m * nbn;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int srow = tid >> 3, kq = (tid & 7) * 4;

    long a_base[RA];
    int a_h0[RA], a_w0[RA], a_f[RA];                 // (a_f: the frame, read by the U8 form alone)
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const int m = m0 + srow + 32 * i;
        if (m < p.M) {
            const int b = fast_div(m, p.fd_hw), rem = m - b * p.Ho * p.Wo;
            const int ho = fast_div(rem, p.fd_wo), wo = rem - ho * p.Wo;
            a_base[i] = (long)b * p.H * p.W * p.Cin;
            a_h0[i] = ho * p.stride - p.pad;
            a_w0[i] = wo * p.stride - p.pad;
            a_f[i] = b;
        } else {
            a_base[i] = 0;
            a_h0[i] = -(1 << 20);
            a_w0[i] = 0;
            a_f[i] = 0;
        }
    }
    f32x4 a_reg[RA], b_reg[RB];
    auto load_chunk = [&](int c) {
        const int k = c * BK + kq;
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int ke = k + e;
                const int t = ke / p.Cin, c1 = ke - t * p.Cin;
                const int kh = t / p.ks, kw = t - kh * p.ks;
                const int hi = a_h0[i] + kh, wi = a_w0[i] + kw;
                const bool ok = ke < p.K && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                if (U8) {
                    v[e] = u8_value(tab, ok, u8_load(*u8, ok, u8_pixel(*u8, a_f[i], hi, wi, p.H, p.W), c1), ok ? c1 : 0);
                } else if (ok)
                    v[e] = p.A[a_base[i] + ((long)hi * p.W + wi) * p.Cin + c1];
            }
            a_reg[i] = v;
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int n = n0 + srow + 32 * i;
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (n < p.N) v = *reinterpret_cast<const f32x4*>(p.Wp + (long)n * p.Kpad + c * BK + kq);
            b_reg[i] = v;
        }
    };
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int wm0 = (wave / WAVES_N) * WM, wn0 = (wave % WAVES_N) * WN;
    const int frow = lane & 31, fk = (lane >> 5) * 4;
    const int nchunks = p.Kpad / BK;
    load_chunk(0);
    for (int c = 0; c < nchunks; ++c) {
#pragma unroll
        for (int i = 0; i < RA; ++i) *reinterpret_cast<f32x4*>(&As[(srow + 32 * i) * PITCH + kq]) = a_reg[i];
#pragma unroll
        for (int i = 0; i < RB; ++i) *reinterpret_cast<f32x4*>(&Bs[(srow + 32 * i) * PITCH + kq]) = b_reg[i];
        __syncthreads();
        if (c + 1 < nchunks) load_chunk(c + 1);
#pragma unroll
        for (int kk = 0; kk < BK; kk += 8) {
            f32x4 af[TM], bf[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[i] = *reinterpret_cast<const f32x4*>(&As[(wm0 + i * 32 + frow) * PITCH + kk + fk]);
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bf[j] = *reinterpret_cast<const f32x4*>(&Bs[(wn0 + j * 32 + frow) * PITCH + kk + fk]);
#pragma unroll
            for (int e = 0; e < 4; ++e)
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int j = 0; j < TN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + wn0 + j * 32 + (lane & 31);
        const bool n_ok = n < p.N;
        const float bv = (p.bias && n_ok) ? p.bias[n] : 0.f;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = m0 + wm0 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
                if (n_ok && m < p.M) {
                    float v = acc[i][j][r] + bv;
                    if (p.res) v += p.res[rowmap(p.rmap, m) + n];
                    if (p.act == ACT_RELU) v = relu_f(v);
                    if (p.out_bf16) {
                        reinterpret_cast<unsigned short*>(p.out)[rowmap(p.omap, m) + n] = to_bf16(v);
                    } else
                    p.out[rowmap(p.omap, m) + n] = v;
                }
            }
        }
    }
}

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void igemm_f32_smallc_kernel(GemmArgs p) {
    igemm_f32_smallc_body<BM, BN, WM, WN, false>(p, nullptr);
}
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(256) void igemm_f32_smallc_u8_kernel(GemmArgs p, U8Input in) {
    igemm_f32_smallc_body<BM, BN, WM, WN, true>(p, &in);
}

// =====================================================================================================
// The 3x3 / stride-2 fp32 stem as a persistent streaming kernel -- the fp32 twin of igemm_bf16_stem_stream_kernel
// (below, where the scheme is described): weights staged once per block, the next 64-pixel tile's runs (for a fixed
// (pixel, kh) the 9 input floats are contiguous in the NHWC image: two 16-byte loads + one dword, raw buffer loads with
// out-of-range offsets instead of branches) in flight across the MFMAs and stores of the current tile, LDS-transposed 16-byte
// stores (128 B contiguous per row), XCD-contiguous tile walk.  K in LDS = (kh, 12): 9 values + 3 zeros per kh, 40 staged
// floats per row.  The element-wise kernel above moved 2.0 TB/s at batch 64 (155 us for 268 MB out + 50 MB in).
// =====================================================================================================
// U8 (see igemm_f32_smallc_body): issue() requests the run's 9 bytes one by one -- they stay in flight across the previous tile's MFMAs and
// stores exactly as the float form's three loads do -- and the table turns them into the float run just before put_run.  Every byte carries
// its own validity, so the float form's patch of the runs that start before the tensor has nothing to do here.
template <int KS, bool U8>
__device__ __forceinline__ void igemm_f32_stem_stream_body(const GemmArgs& p, const int ntiles, const U8Input* u8) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int BM = 64, BN = 64;
    constexpr int RUN = KS * 3, NX4 = RUN / 4;      // 9 floats = 2 quads + 1 dword
    static_assert(RUN % 4 == 1, "one dword behind the quads (a 16-byte load with dead upper dwords costs a vmcnt(0))");
    constexpr int PKH = (RUN + 3) / 4 * 4;          // floats per kh in LDS (12)
    constexpr int KP = (KS * PKH + 7) / 8 * 8;      // staged K (40)
    constexpr int SP = KP + 4;                      // floats per LDS row: conflict-free b128 reads
    constexpr int EPS = 36;
    constexpr unsigned OOB = 0x80000000u;
    static_assert(BM * KS <= 256, "one run per thread");
    __shared__ __attribute__((aligned(16))) float lds[(BM + BN) * SP + 4 * 32 * EPS + (U8 ? U8_TAB : 0)];
    float* As = lds;
    float* Bs = lds + BM * SP;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* ep = lds + (BM + BN) * SP + wave * (32 * EPS);
    const float* tab = lds + (BM + BN) * SP + 4 * 32 * EPS;
    if (U8) u8_fill_table(lds + (BM + BN) * SP + 4 * 32 * EPS, *u8, tid, 256);     // (the barrier behind the first put_run's comes before its first lookup: below)
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const long total = (long)(p.M / (p.Ho * p.Wo)) * p.H * p.W * 3;              // floats of the image tensor (< 2^29: launcher)
    const rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(U8 ? (void*)p.out : (void*)p.A, 0, U8 ? 0u : (unsigned)(total * 4), 0x00020000);
    const rsrc_t rs_bias = __builtin_amdgcn_make_buffer_rsrc(p.bias ? (void*)p.bias : (void*)p.out, 0,
                                                             p.bias ? (unsigned)p.N * 4u : 0u, 0x00020000);
    auto ldq = [&](rsrc_t r, unsigned off) { return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0)); };
    auto ldd = [&](rsrc_t r, unsigned off) { return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0)); };
    auto put_run = [&](float* dst, const f32x4 (&q)[NX4], float last, unsigned mask, int kh) {
        auto val = [&](int e) { return e < NX4 * 4 ? q[e >> 2][e & 3] : (e == NX4 * 4 ? last : 0.f); };
#pragma unroll
        for (int g = 0; g < PKH / 4; ++g) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = (4 * g + e < RUN && ((mask >> (4 * g + e)) & 1u)) ? val(4 * g + e) : 0.f;
            *reinterpret_cast<f32x4*>(dst + kh * PKH + 4 * g) = v;
        }
        if (KP > KS * PKH && kh == KS - 1) *reinterpret_cast<f32x4*>(dst + KS * PKH) = f32x4{0.f, 0.f, 0.f, 0.f};
    };
    {   // weights, once per block: runs of the fp32 pack [N][Kpad], K order (kh, kw, c)
        const rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.Wp, 0, (unsigned)p.N * (unsigned)p.Kpad * 4u, 0x00020000);
        for (int t = tid; t < BN * KS; t += 256) {
            const int kh = t / BN, n = t - kh * BN;
            const unsigned wo = n < p.N ? (unsigned)(n * p.Kpad + kh * RUN) * 4u : OOB;
            f32x4 q[NX4];
#pragma unroll
            for (int x = 0; x < NX4; ++x) q[x] = ldq(rs_w, n < p.N ? wo + 16u * x : OOB);
            const float last = ldd(rs_w, n < p.N ? wo + 16u * NX4 : OOB);
            put_run(Bs + n * SP, q, last, (1u << RUN) - 1u, kh);
        }
    }
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslots = gridDim.x >> 3;
    const int per_xcd = (ntiles + 7) >> 3;
    const int t_end = min(ntiles, (xcd + 1) * per_xcd);
    int tile = xcd * per_xcd + slot;

    f32x4 q[NX4];
    float qlast;
    unsigned mask;
    unsigned raw[RUN];                               // U8: the run's bytes, (kw, c) order like the float run
    const int t_run = tid % (BM * KS);              // (threads beyond the 192 runs repeat one: same loads, same LDS bytes)
    const int r_kh = t_run / BM, r_row = t_run - r_kh * BM;
    auto issue = [&](int tl) {
        const int m = tl * BM + r_row;
        bool ok = tl < t_end && m < p.M;
        const int mm = ok ? m : 0;
        const int b = fast_div(mm, p.fd_hw), rem = mm - b * p.Ho * p.Wo;
        const int ho = fast_div(rem, p.fd_wo), wo = rem - ho * p.Wo;
        const int hi = ho * p.stride - p.pad + r_kh, wi0 = wo * p.stride - p.pad;
        ok = ok && (unsigned)hi < (unsigned)p.H;
        const int o = ((b * p.H + hi) * p.W + wi0) * 3;
        const int lo = max(0, -wi0), hn = max(lo, min(KS, p.W - wi0));
        mask = ok ? (((1u << (3 * hn)) - 1u) & ~((1u << (3 * lo)) - 1u)) : 0u;
        if (U8) {
#pragma unroll
            for (int kw = 0; kw < KS; ++kw) {
                const bool v = (mask >> (3 * kw)) & 1u;
                const long px = u8_pixel(*u8, b, hi, wi0 + kw, p.H, p.W);
#pragma unroll
                for (int c = 0; c < 3; ++c) raw[3 * kw + c] = u8_load(*u8, v, px, c);
            }
            return;
        }
#pragma unroll
        for (int x = 0; x < NX4; ++x) q[x] = ldq(rs_in, (ok && o + 4 * x >= 0) ? (unsigned)(o + 4 * x) * 4u : OOB);
        qlast = ldd(rs_in, (ok && o + 4 * NX4 >= 0) ? (unsigned)(o + 4 * NX4) * 4u : OOB);
    };
    auto decode = [&]() {                            // U8: bytes -> the float run (masked elements are zeroed by put_run)
#pragma unroll
        for (int e = 0; e < RUN; ++e) {
            const float v = tab[(e % 3) * 256 + raw[e]];
            if (e < NX4 * 4) q[e >> 2][e & 3] = v; else qlast = v;
        }
    };
    const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
    const int frow = lane & 31, fhalf = lane >> 5, fk = fhalf * 4;
    const int er = lane >> 3, ec = (lane & 7) * 4;          // epilogue: 8 lanes x 16 B = one 128-B row of the wave's 32 channels
    const f32x4 bv = ldq(rs_bias, (unsigned)(wn0 + ec) * 4u);

    issue(tile);
    {   // four dropped stores: the loop is entered with the same "loads, then four stores" in flight as its back edge leaves
        const rsrc_t rs_none = __builtin_amdgcn_make_buffer_rsrc((void*)p.out, 0, 0u, 0x00020000);
#pragma unroll
        for (int k = 0; k < 4; ++k)                 // (distinct offsets: identical stores would be merged into one)
            __builtin_amdgcn_raw_buffer_store_b128(u32x4{0u, 0u, 0u, 0u}, rs_none, OOB + 16u * k, 0, 0);
    }
    if (U8) __syncthreads();                         // the value table is complete
    for (; tile < t_end; tile += nslots) {
        const int m0 = tile * BM;
        if (U8) decode();
        put_run(As + r_row * SP, q, qlast, mask, r_kh);
        const int ho_max = p.pad / p.stride;
        if (!U8 && m0 < (ho_max + 1) * p.Wo) {      // frame 0, input row 0, window left of the image: negative tensor offsets
            __syncthreads();
            const int nw = min(p.Wo, (p.pad + p.stride - 1) / p.stride);
            for (int idx = tid; idx < (ho_max + 1) * nw * PKH; idx += 256) {
                const int e = idx % PKH, r = idx / PKH, wo = r % nw, ho = r / nw;
                const int kh = p.pad - ho * p.stride, m = ho * p.Wo + wo;
                if (kh >= 0 && kh < KS && m >= m0 && m < m0 + BM) {
                    const int wi = wo * p.stride - p.pad + e / 3;
                    float v = 0.f;
                    if (e < RUN && (unsigned)wi < (unsigned)p.W) v = p.A[wi * 3 + e % 3];
                    As[(m - m0) * SP + kh * PKH + e] = v;
                }
            }
        }
        __syncthreads();
        issue(tile + nslots);

        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < KP; kk += 8) {
            const f32x4 af = *reinterpret_cast<const f32x4*>(&As[(wm0 + frow) * SP + kk + fk]);
            const f32x4 bf = *reinterpret_cast<const f32x4*>(&Bs[(wn0 + frow) * SP + kk + fk]);
#pragma unroll
            for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf[e], af[e], acc, 0, 0, 0);
        }
        // transposed accumulator: lane = row m (lane & 31), register 4 g + e = channel 8 g + 4 fhalf + e
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<f32x4*>(&ep[frow * EPS + 8 * g + 4 * fhalf]) = f32x4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        __builtin_amdgcn_wave_barrier();
        const rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc((void*)(p.out + (long)m0 * p.omap.S1 + p.omap.off), 0, 0x7FFFFF00u, 0x00020000);
#pragma unroll
        for (int h = 0; h < 4; ++h) {
            const int row = h * 8 + er, ml = wm0 + row, nl = wn0 + ec;
            f32x4 x = *reinterpret_cast<const f32x4*>(&ep[row * EPS + ec]);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                x[e] += bv[e];
                if (p.act == ACT_RELU) x[e] = relu_f(x[e]);
            }
            __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, x), rs_out,
                                                   (m0 + ml < p.M && nl < p.N) ? (unsigned)(ml * (int)p.omap.S1 + nl) * 4u : OOB, 0, 0);
        }
        __syncthreads();
    }
#endif
}

template <int KS>
__global__ __launch_bounds__(256, 2) void igemm_f32_stem_stream_kernel(GemmArgs p, int ntiles) {
    igemm_f32_stem_stream_body<KS, false>(p, ntiles, nullptr);
}
template <int KS>
__global__ __launch_bounds__(256, 2) void igemm_f32_stem_stream_u8_kernel(GemmArgs p, int ntiles, U8Input in) {
    igemm_f32_stem_stream_body<KS, true>(p, ntiles, &in);
}

// =====================================================================================================
// Small-Cin stem (Cin = 3, k = 3 or 7) under compute_dtype = bf16: the fp32 image is gathered element-wise (K order
// (kh, kw, c), like the fp32 igemm_f32_smallc kernel whose packed fp32 weights it shares), rounded to bf16 on the way into
// a padded LDS tile, and multiplied on v_mfma_f32_32x32x16_bf16: 1/8 of the matrix cycles of the fp32 stem, which was
// 1.1 ms of CPN's 9.7 ms at batch 128 (384x288) -- the gather is what remains.  Output bf16 NHWC.
// =====================================================================================================
[[maybe_unused]] static constexpr int SPITCH = 40;          // halves per LDS row: 32 k-values + 8 pad (80 B: 16-byte aligned fragment reads)

// U8 (all three stem kernels below): the uint8 forms -- the image is the BGR crop itself, see igemm_f32_smallc_body above for the
// scheme: a per-block value table filled with pixel_rule(), one byte load per tap with its own validity, the same tile / K order / MFMA
// sequence as the float form, the descriptor as an extra argument of the *_u8_kernel entry points.
template <class F, bool U8>
__device__ __forceinline__ void igemm_bf16_smallc_body(const GemmArgs& p, const U8Input* u8) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int BM = 128, BN = 64, WM = 64, WN = 32, SBK = 32;
    constexpr int WAVES_N = BN / WN, TM = WM / 32, TN = WN / 32, RA = BM / 32, RB = BN / 32;
    __shared__ __attribute__((aligned(16))) unsigned short lds[(BM + BN) * SPITCH + (U8 ? 2 * U8_TAB : 0)];
    unsigned short* As = lds;
    unsigned short* Bs = lds + BM * SPITCH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* tab = reinterpret_cast<const float*>(lds + (BM + BN) * SPITCH);
    if (U8) {
        u8_fill_table(reinterpret_cast<float*>(lds + (BM + BN) * SPITCH), *u8, tid, 256);
        __syncthreads();
    }
    const int nbn = (p.N + BN - 1) / BN;
    const int bid = xcd_remap_b(blockIdx.x, gridDim.x);
    const int tile_m = bid / nbn, tile_n = bid - tile_m * nbn;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const int srow = tid >> 3, kq = (tid & 7) * 4;

    long a_base[RA];
    int a_h0[RA], a_w0[RA], a_f[RA];                  // (a_f: the frame, read by the U8 form alone)
#pragma unroll
    for (int i = 0; i < RA; ++i) {
        const int m = m0 + srow + 32 * i;
        a_base[i] = 0; a_h0[i] = -(1 << 20); a_w0[i] = 0; a_f[i] = 0;
        if (m < p.M) {
            const int b = fast_div_b(m, p.fd_hw), rem = m - b * p.Ho * p.Wo;
            const int ho = fast_div_b(rem, p.fd_wo), wo = rem - ho * p.Wo;
            a_f[i] = b;
            a_base[i] = (long)b * p.H * p.W * p.Cin;
            a_h0[i] = ho * p.stride - p.pad;
            a_w0[i] = wo * p.stride - p.pad;
        }
    }
    float a_reg[RA][4];
    f32x4 b_reg[RB];
    auto load_chunk = [&](int c) {
        int dh[4], dw[4], doff[4], dc[4];
        bool kok[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {          // the (kh, kw, c) of this thread's four k-values: the same for every row
            const int ke = c * SBK + kq + e;
            const int t = ke / p.Cin, c1 = ke - t * p.Cin;
            dh[e] = t / p.ks;
            dw[e] = t - dh[e] * p.ks;
            doff[e] = (dh[e] * p.W + dw[e]) * p.Cin + c1;
            kok[e] = ke < p.K;
            dc[e] = kok[e] ? c1 : 0;
        }
#pragma unroll
        for (int i = 0; i < RA; ++i) {
            const long row = a_base[i] + ((long)a_h0[i] * p.W + a_w0[i]) * p.Cin;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int hi = a_h0[i] + dh[e], wi = a_w0[i] + dw[e];
                const bool ok = kok[e] && (unsigned)hi < (unsigned)p.H && (unsigned)wi < (unsigned)p.W;
                if (U8) a_reg[i][e] = u8_value(tab, ok, u8_load(*u8, ok, u8_pixel(*u8, a_f[i], hi, wi, p.H, p.W), dc[e]), dc[e]);
                else a_reg[i][e] = ok ? p.A[row + doff[e]] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < RB; ++i) {
            const int n = n0 + srow + 32 * i;
            b_reg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (n < p.N) b_reg[i] = *reinterpret_cast<const f32x4*>(p.Wp + (long)n * p.Kpad + c * SBK + kq);
        }
    };
    f32x16 acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;
    const int wm0 = (wave / WAVES_N) * WM, wn0 = (wave % WAVES_N) * WN;
    const int frow = lane & 31, fhalf = lane >> 5;
    const int nchunks = p.Kpad / SBK;          // the fp32 pack pads K to a multiple of 32
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
    load_chunk(0);
    for (int c = 0; c < nchunks; ++c) {
#pragma unroll
        for (int i = 0; i < RA; ++i)
            *reinterpret_cast<u32x2*>(&As[(srow + 32 * i) * SPITCH + kq]) =
                u32x2{F::pack2(a_reg[i][0], a_reg[i][1]), F::pack2(a_reg[i][2], a_reg[i][3])};
#pragma unroll
        for (int i = 0; i < RB; ++i)
            *reinterpret_cast<u32x2*>(&Bs[(srow + 32 * i) * SPITCH + kq]) =
                u32x2{F::pack2(b_reg[i][0], b_reg[i][1]), F::pack2(b_reg[i][2], b_reg[i][3])};
        __syncthreads();
        if (c + 1 < nchunks) load_chunk(c + 1);
#pragma unroll
        for (int step = 0; step < SBK / 16; ++step) {
            typename F::x8 af[TM], bfr[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i)
                af[i] = __builtin_bit_cast(typename F::x8, *reinterpret_cast<const f32x4*>(&As[(wm0 + i * 32 + frow) * SPITCH + step * 16 + fhalf * 8]));
#pragma unroll
            for (int j = 0; j < TN; ++j)
                bfr[j] = __builtin_bit_cast(typename F::x8, *reinterpret_cast<const f32x4*>(&Bs[(wn0 + j * 32 + frow) * SPITCH + step * 16 + fhalf * 8]));
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = F::mfma(bfr[j], af[i], acc[i][j]);
        }
        __syncthreads();
    }
    // transposed accumulator (lane = row m, register group g = channels 8 g + 4 (lane >> 5) .. + 3): 8-byte stores
    unsigned short* Out = reinterpret_cast<unsigned short*>(p.out);
#pragma unroll
    for (int i = 0; i < TM; ++i) {
        const int m = m0 + wm0 + i * 32 + frow;
        if (m >= p.M) continue;
        const long o_row = (long)m * p.omap.S1 + p.omap.off;
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const int n = n0 + wn0 + j * 32 + 4 * fhalf + 8 * g;
                if (n >= p.N) continue;
                u16x4 v;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float t = acc[i][j][4 * g + e] + (p.bias ? p.bias[n + e] : 0.f);
                    if (p.act == ACT_RELU) t = relu_f(t);
                    v[e] = F::narrow(t);
                }
                *reinterpret_cast<u16x4*>(Out + o_row + n) = v;
            }
    }
#endif
}

template <class F>
__global__ __launch_bounds__(256) void igemm_bf16_smallc_kernel(GemmArgs p) { igemm_bf16_smallc_body<F, false>(p, nullptr); }
template <class F>
__global__ __launch_bounds__(256) void igemm_bf16_smallc_u8_kernel(GemmArgs p, U8Input in) { igemm_bf16_smallc_body<F, true>(p, &in); }

// Stem, second version (Cin = 3, k = 7 or 3): for a fixed (output pixel, kh) the 3 k input values are CONTIGUOUS in the NHWC
// image (and in the (kh, kw, c)-ordered weights), so a thread fetches one such run with 16-byte loads (dword-aligned
// addresses) instead of 21 / 9 scalar gathers, zeroes what lies outside the image, and writes it as bf16 into an LDS tile
// whose K axis is (kh, 24 | 16): the whole K of a 128 x 64 tile is staged once (no chunk loop), then 11 / 3 MFMA k-steps.
template <int KS, int BM, class F, bool U8>
__device__ __forceinline__ void igemm_bf16_stem_body(const GemmArgs& p, const U8Input* u8) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int BN = 64, WM = BM / 2, WN = 32, TM = WM / 32;
    constexpr int RUN = KS * 3;                      // contiguous floats per (pixel, kh)
    constexpr int NX4 = (RUN + 3) / 4;               // 16-byte loads per run
    constexpr int PKH = (RUN + 7) / 8 * 8;           // halves per kh in LDS (24 / 16)
    constexpr int KP = (KS * PKH + 15) / 16 * 16;    // staged K (176 / 48)
    constexpr int PITCH = KP + 8;                    // halves per LDS row: 16-byte aligned, conflict-free b128 reads
    __shared__ __attribute__((aligned(16))) unsigned short lds[(BM + BN) * PITCH + (U8 ? 2 * U8_TAB : 0)];
    unsigned short* As = lds;
    unsigned short* Bs = lds + BM * PITCH;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int nbn = (p.N + BN - 1) / BN;
    const int bid = xcd_remap_b(blockIdx.x, gridDim.x);
    const int tile_m = bid / nbn, tile_n = bid - tile_m * nbn;
    const int m0 = tile_m * BM, n0 = tile_n * BN;
    const long total = (long)(p.M / (p.Ho * p.Wo)) * p.H * p.W * 3;
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const float* tab = reinterpret_cast<const float*>(lds + (BM + BN) * PITCH);
    if (U8) {
        u8_fill_table(reinterpret_cast<float*>(lds + (BM + BN) * PITCH), *u8, tid, 256);
        __syncthreads();
    }

    auto put_run = [&](unsigned short* dst, const float (&v)[NX4 * 4], int kh) {     // RUN values (+ zero padding) -> LDS as bf16
        unsigned pk[PKH / 2];
#pragma unroll
        for (int e = 0; e < PKH / 2; ++e)
            pk[e] = F::pack2(2 * e < NX4 * 4 ? v[2 * e] : 0.f, 2 * e + 1 < NX4 * 4 ? v[2 * e + 1] : 0.f);
#pragma unroll
        for (int q = 0; q < PKH / 8; ++q)
            *reinterpret_cast<u32x4*>(dst + kh * PKH + q * 8) = u32x4{pk[4 * q], pk[4 * q + 1], pk[4 * q + 2], pk[4 * q + 3]};
        if (KP > KS * PKH && kh == KS - 1)                                         // the tail of the last k-step
            *reinterpret_cast<u32x4*>(dst + KS * PKH) = u32x4{0u, 0u, 0u, 0u};
    };
    for (int t = tid; t < BM * KS; t += 256) {               // activation runs: consecutive lanes = consecutive pixels
        const int kh = t / BM, row = t - kh * BM;
        const int m = m0 + row;
        float v[NX4 * 4];
#pragma unroll
        for (int e = 0; e < NX4 * 4; ++e) v[e] = 0.f;
        if (m < p.M) {
            const int b = fast_div_b(m, p.fd_hw), rem = m - b * p.Ho * p.Wo;
            const int ho = fast_div_b(rem, p.fd_wo), wo = rem - ho * p.Wo;
            const int hi = ho * p.stride - p.pad + kh, wi0 = wo * p.stride - p.pad;
            if (U8 && (unsigned)hi < (unsigned)p.H) {
#pragma unroll
                for (int kw = 0; kw < KS; ++kw) {
                    const bool ok = (unsigned)(wi0 + kw) < (unsigned)p.W;
                    const long px = u8_pixel(*u8, b, hi, wi0 + kw, p.H, p.W);
#pragma unroll
                    for (int c = 0; c < 3; ++c) v[3 * kw + c] = u8_value(tab, ok, u8_load(*u8, ok, px, c), c);
                }
            } else if ((unsigned)hi < (unsigned)p.H) {
                const long src = (((long)b * p.H + hi) * p.W + wi0) * 3;
#pragma unroll
                for (int x = 0; x < NX4; ++x) {
                    const long o = src + 4 * x;
                    if (o >= 0 && o + 4 <= total) {
                        __builtin_memcpy(&v[4 * x], p.A + o, 16);
                    } else {
#pragma unroll
                        for (int e = 0; e < 4; ++e)
                            if (o + e >= 0 && o + e < total) v[4 * x + e] = p.A[o + e];
                    }
                }
#pragma unroll
                for (int e = 0; e < NX4 * 4; ++e)
                    if (e >= RUN || (unsigned)(wi0 + e / 3) >= (unsigned)p.W) v[e] = 0.f;
            }
        }
        put_run(As + row * PITCH, v, kh);
    }
    for (int t = tid; t < BN * KS; t += 256) {               // weight runs from the fp32 pack [N][Kpad], K order (kh, kw, c)
        const int kh = t / BN, n = t - kh * BN;
        float v[NX4 * 4];
#pragma unroll
        for (int e = 0; e < NX4 * 4; ++e) v[e] = 0.f;
        if (n0 + n < p.N) {
            const float* src = p.Wp + (long)(n0 + n) * p.Kpad + kh * RUN;          // (kh * RUN + 4 NX4 <= Kpad: launcher checks)
#pragma unroll
            for (int x = 0; x < NX4; ++x) __builtin_memcpy(&v[4 * x], src + 4 * x, 16);
#pragma unroll
            for (int e = RUN; e < NX4 * 4; ++e) v[e] = 0.f;
        }
        put_run(Bs + n * PITCH, v, kh);
    }
    __syncthreads();

    f32x16 acc[TM];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
    const int wm0 = (wave >> 1) * WM, wn0 = (wave & 1) * WN;
    const int frow = lane & 31, fhalf = lane >> 5;
#pragma unroll
    for (int step = 0; step < KP / 16; ++step) {
        const typename F::x8 bfr = __builtin_bit_cast(typename F::x8, *reinterpret_cast<const f32x4*>(&Bs[(wn0 + frow) * PITCH + step * 16 + fhalf * 8]));
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const typename F::x8 af = __builtin_bit_cast(typename F::x8, *reinterpret_cast<const f32x4*>(&As[(wm0 + i * 32 + frow) * PITCH + step * 16 + fhalf * 8]));
            acc[i] = F::mfma(bfr, af, acc[i]);
        }
    }
    // transposed accumulator (lane = row m, register group g = channels 8 g + 4 fhalf .. + 3): 8-byte stores
    unsigned short* Out = reinterpret_cast<unsigned short*>(p.out);
    typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const int n = n0 + wn0 + 4 * fhalf + 8 * g;
        if (n >= p.N) continue;
        f32x4 bv = {0.f, 0.f, 0.f, 0.f};
        if (p.bias) bv = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const int m = m0 + wm0 + i * 32 + frow;
            if (m >= p.M) continue;
            float t[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                t[e] = acc[i][4 * g + e] + bv[e];
                if (p.act == ACT_RELU) t[e] = relu_f(t[e]);
            }
            *reinterpret_cast<u32x2*>(Out + (long)m * p.omap.S1 + p.omap.off + n) = u32x2{F::pack2(t[0], t[1]), F::pack2(t[2], t[3])};
        }
    }
#endif
}

template <int KS, int BM, class F>
__global__ __launch_bounds__(256) void igemm_bf16_stem_kernel(GemmArgs p) { igemm_bf16_stem_body<KS, BM, F, false>(p, nullptr); }
template <int KS, int BM, class F>
__global__ __launch_bounds__(256) void igemm_bf16_stem_u8_kernel(GemmArgs p, U8Input in) { igemm_bf16_stem_body<KS, BM, F, true>(p, &in); }

// Stem, third version: PERSISTENT blocks with the weights staged once and the next tile's runs in flight while the current
// tile is multiplied and stored.  The second version above is one latency chain per block -- gather (6 x 16-byte loads per run
// behind per-quad branches, i.e. one L2 round trip after the other), LDS, 11 MFMAs, 8-byte strided stores -- with only two
// 70 KiB blocks per CU to hide it: 488 us for CPN's 7x7 at batch 128 (1.3 TB/s; 453 MB out + 170 MB in would take 125 us at
// 5 TB/s).  Here: 64-pixel tiles (47 KiB of operands + 18 KiB of epilogue scratch: two blocks per CU), every run fetched with
// raw buffer loads on ONE descriptor over the whole image tensor (a quad outside it, or of a row above / below the image,
// gets an out-of-range offset; a quad only PARTLY beyond the tensor's end returns its in-range dwords -- range checking is
// per dword, tools/buffer_oob.hip), so all of a thread's 12 / 3 loads are in flight at once and stay in flight across the
// MFMAs and the stores of the previous tile; the epilogue transposes through LDS and stores 16 bytes per lane, 64 B
// contiguous per row.  XCD-aware tile order: each XCD walks its own contiguous eighth of the tiles, so the 7 / 3 input rows
// that vertically adjacent tiles share are fetched into ONE L2.  Only the handful of runs at the very start of the tensor (negative
// offsets cannot be expressed) are patched element-wise by the blocks that own those pixels.
// U8: issue() requests the runs' 21 / 9 bytes one by one -- in flight across the previous tile's MFMAs and stores like the float form's
// loads -- and the table turns them into the float run just before put_run.  Every byte carries its own validity, so the patch of the runs
// that start before the tensor has nothing to do in that form.
template <int KS, class F, bool U8>
__device__ __forceinline__ void igemm_bf16_stem_stream_body(const GemmArgs& p, const int ntiles, const U8Input* u8) {
#if defined(__HIP_DEVICE_COMPILE__)
    constexpr int BM = 64, BN = 64;
    constexpr int RUN = KS * 3;                      // contiguous floats per (pixel, kh)
    constexpr int NX4 = RUN / 4;                     // 16-byte loads per run (5 / 2) ...
    static_assert(RUN % 4 == 1, "... plus ONE dword: a 16-byte load whose upper dwords nobody reads leaves dead destination "
                                "registers that the allocator reuses -- and a vmcnt(0) in front of that reuse");
    constexpr int PKH = (RUN + 7) / 8 * 8;           // halves per kh in LDS (24 / 16)
    constexpr int KP = (KS * PKH + 15) / 16 * 16;    // staged K (176 / 48)
    constexpr int PITCH = KP + 8;                    // halves per LDS row: 16-byte aligned, conflict-free b128 reads
    constexpr int NT = (BM * KS + 255) / 256;        // runs per thread and tile (2 / 1)
    constexpr int EPS = 36;
    constexpr unsigned OOB = 0x80000000u;
    __shared__ __attribute__((aligned(16))) unsigned short lds[(BM + BN) * PITCH + 4 * 32 * EPS * 2 + (U8 ? 2 * U8_TAB : 0)];
    unsigned short* As = lds;
    unsigned short* Bs = lds + BM * PITCH;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* ep = reinterpret_cast<float*>(lds + (BM + BN) * PITCH) + wave * (32 * EPS);
    const float* tab = reinterpret_cast<const float*>(lds + (BM + BN) * PITCH + 4 * 32 * EPS * 2);
    if (U8) u8_fill_table(reinterpret_cast<float*>(lds + (BM + BN) * PITCH + 4 * 32 * EPS * 2), *u8, tid, 256);   // (its barrier: in front of the tile loop)
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    unsigned short* Out = reinterpret_cast<unsigned short*>(p.out);
    const long total = (long)(p.M / (p.Ho * p.Wo)) * p.H * p.W * 3;              // floats of the image tensor (< 2^29: launcher)
    const rsrc_t rs_in = __builtin_amdgcn_make_buffer_rsrc(U8 ? (void*)Out : (void*)p.A, 0, U8 ? 0u : (unsigned)(total * 4), 0x00020000);
    const rsrc_t rs_bias = __builtin_amdgcn_make_buffer_rsrc(p.bias ? (void*)p.bias : (void*)Out, 0,
                                                             p.bias ? (unsigned)p.N * 4u : 0u, 0x00020000);

    auto put_run = [&](unsigned short* dst, const f32x4 (&q)[NX4], float last, unsigned mask, int kh) {   // RUN values (+ zeros) -> LDS
        auto val = [&](int e) { return e < NX4 * 4 ? q[e >> 2][e & 3] : (e == NX4 * 4 ? last : 0.f); };
        unsigned pk[PKH / 2];
        if (mask == (1u << RUN) - 1u) {              // interior pixel (all but ~1 run in 70): no per-element selects
#pragma unroll
            for (int e = 0; e < PKH / 2; ++e) pk[e] = F::pack2(2 * e < RUN ? val(2 * e) : 0.f, 2 * e + 1 < RUN ? val(2 * e + 1) : 0.f);
        } else {
#pragma unroll
            for (int e = 0; e < PKH / 2; ++e) {
                const float a = 2 * e < RUN && ((mask >> (2 * e)) & 1u) ? val(2 * e) : 0.f;
                const float b = 2 * e + 1 < RUN && ((mask >> (2 * e + 1)) & 1u) ? val(2 * e + 1) : 0.f;
                pk[e] = F::pack2(a, b);
            }
        }
#pragma unroll
        for (int g = 0; g < PKH / 8; ++g)
            *reinterpret_cast<u32x4*>(dst + kh * PKH + g * 8) = u32x4{pk[4 * g], pk[4 * g + 1], pk[4 * g + 2], pk[4 * g + 3]};
        if (KP > KS * PKH && kh == KS - 1)                                         // the tail of the last k-step
            *reinterpret_cast<u32x4*>(dst + KS * PKH) = u32x4{0u, 0u, 0u, 0u};
    };

    // ---- weights, once per block: runs of the fp32 pack [N][Kpad], K order (kh, kw, c)
    {
        const rsrc_t rs_w = __builtin_amdgcn_make_buffer_rsrc((void*)p.Wp, 0, (unsigned)p.N * (unsigned)p.Kpad * 4u, 0x00020000);
        for (int t = tid; t < BN * KS; t += 256) {
            const int kh = t / BN, n = t - kh * BN;
            f32x4 q[NX4];
            const unsigned wo = n < p.N ? (unsigned)(n * p.Kpad + kh * RUN) * 4u : OOB;
#pragma unroll
            for (int x = 0; x < NX4; ++x)
                q[x] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_w, n < p.N ? wo + 16u * x : OOB, 0, 0));
            const float last = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rs_w, n < p.N ? wo + 16u * NX4 : OOB, 0, 0));
            put_run(Bs + n * PITCH, q, last, (1u << RUN) - 1u, kh);
        }
    }
    // XCD-aware persistent walk: XCD x owns tiles [x * per_xcd, (x + 1) * per_xcd); its blocks take them round-robin
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, nslots = gridDim.x >> 3;        // (gridDim.x % 8 == 0: launcher)
    const int per_xcd = (ntiles + 7) >> 3;
    const int t_end = min(ntiles, (xcd + 1) * per_xcd);
    int tile = xcd * per_xcd + slot;

    f32x4 q[NT][NX4];
    float qlast[NT];
    unsigned mask[NT];
    unsigned raw[NT][RUN];                           // U8: the runs' bytes, (kw, c) order like the float runs
    // run i of this thread; a thread without an i-th run repeats another one (same loads, the same LDS bytes written twice) --
    // a branch around put_run would leave "maybe pending" loads behind it and cost a vmcnt(0) in front of the next requests
    auto run_of = [&](int i) { return (tid + 256 * i) % (BM * KS); };
    auto issue = [&](int tl) {                       // request the runs of tile tl (tl >= t_end: every offset out of range)
        const int m0 = tl * BM;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int t = run_of(i);
            const int kh = t / BM, row = t - kh * BM;
            const int m = m0 + row;
            bool ok = tl < t_end && m < p.M;
            const int mm = ok ? m : 0;
            const int b = fast_div_b(mm, p.fd_hw), rem = mm - b * p.Ho * p.Wo;
            const int ho = fast_div_b(rem, p.fd_wo), wo = rem - ho * p.Wo;
            const int hi = ho * p.stride - p.pad + kh, wi0 = wo * p.stride - p.pad;
            ok = ok && (unsigned)hi < (unsigned)p.H;
            const int o = ((b * p.H + hi) * p.W + wi0) * 3;                      // floats from the tensor start (may be < 0 at its start)
            // elements 3 lo .. 3 hn - 1 of the run lie inside the image row
            const int lo = max(0, -wi0), hn = max(lo, min(KS, p.W - wi0));
            const unsigned mk = ((1u << (3 * hn)) - 1u) & ~((1u << (3 * lo)) - 1u);
            mask[i] = ok ? mk : 0u;
            if (U8) {
#pragma unroll
                for (int kw = 0; kw < KS; ++kw) {
                    const bool v = (mask[i] >> (3 * kw)) & 1u;
                    const long px = u8_pixel(*u8, b, hi, wi0 + kw, p.H, p.W);
#pragma unroll
                    for (int c = 0; c < 3; ++c) raw[i][3 * kw + c] = u8_load(*u8, v, px, c);
                }
                continue;
            }
#pragma unroll
            for (int x = 0; x < NX4; ++x)
                q[i][x] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(
                                                        rs_in, (ok && o + 4 * x >= 0) ? (unsigned)(o + 4 * x) * 4u : OOB, 0, 0));
            qlast[i] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(
                                                     rs_in, (ok && o + 4 * NX4 >= 0) ? (unsigned)(o + 4 * NX4) * 4u : OOB, 0, 0));
        }
    };
    const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
    const int frow = lane & 31, fhalf = lane >> 5;
    const int er = lane >> 2, ec = (lane & 3) * 8;
    const f32x4 b0 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_bias, (unsigned)(wn0 + ec) * 4u, 0, 0));
    const f32x4 b1 = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_bias, (unsigned)(wn0 + ec + 4) * 4u, 0, 0));

    issue(tile);
    {   // two dropped stores: the loop is entered with the same "loads, then two stores" in flight as its back edge leaves, so the
        // wait in front of the LDS writes is a counted vmcnt(2) -- not a vmcnt(0) that would sit out the previous tile's stores
        const rsrc_t rs_none = __builtin_amdgcn_make_buffer_rsrc((void*)Out, 0, 0u, 0x00020000);
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{0u, 0u, 0u, 0u}, rs_none, OOB, 0, 0);
        __builtin_amdgcn_raw_buffer_store_b128(u32x4{0u, 0u, 0u, 0u}, rs_none, OOB + 16u, 0, 0);   // (distinct: identical stores are merged)
    }
    if (U8) __syncthreads();                          // the value table is complete
    for (; tile < t_end; tile += nslots) {
        const int m0 = tile * BM;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int t = run_of(i);
            const int kh = t / BM, row = t - kh * BM;
            if (U8) {                                  // bytes -> the float run (masked elements are zeroed by put_run)
#pragma unroll
                for (int e = 0; e < RUN; ++e) {
                    const float v = tab[(e % 3) * 256 + raw[i][e]];
                    if (e < NX4 * 4) q[i][e >> 2][e & 3] = v; else qlast[i] = v;
                }
            }
            put_run(As + row * PITCH, q[i], qlast[i], mask[i], kh);
        }
        const int ho_max = p.pad / p.stride;           // output rows (of frame 0) with a window row on input row 0
        if (!U8 && m0 < (ho_max + 1) * p.Wo) {
            // Frame 0, input row 0, window starting left of the image: the run begins at a NEGATIVE offset from the tensor start,
            // which a buffer offset cannot express -- its first quads were requested out of range above.  The few such runs
            // (output rows ho = (pad - kh) / stride, columns wo * stride < pad) are rewritten here element by element.
            __syncthreads();
            const int nw = min(p.Wo, (p.pad + p.stride - 1) / p.stride);
            for (int idx = tid; idx < (ho_max + 1) * nw * PKH; idx += 256) {
                const int e = idx % PKH, r = idx / PKH, wo = r % nw, ho = r / nw;
                const int kh = p.pad - ho * p.stride, m = ho * p.Wo + wo;
                if (kh >= 0 && kh < KS && m >= m0 && m < m0 + BM) {
                    const int wi = wo * p.stride - p.pad + e / 3;
                    float v = 0.f;
                    if (e < RUN && (unsigned)wi < (unsigned)p.W) v = p.A[wi * 3 + e % 3];
                    As[(m - m0) * PITCH + kh * PKH + e] = F::narrow(v);
                }
            }
        }
        __syncthreads();
        issue(tile + nslots);                         // in flight across this tile's MFMAs and stores

        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
        for (int step = 0; step < KP / 16; ++step) {
            const typename F::x8 bfr = __builtin_bit_cast(typename F::x8, *reinterpret_cast<const f32x4*>(&Bs[(wn0 + frow) * PITCH + step * 16 + fhalf * 8]));
            const typename F::x8 af = __builtin_bit_cast(typename F::x8, *reinterpret_cast<const f32x4*>(&As[(wm0 + frow) * PITCH + step * 16 + fhalf * 8]));
            acc = F::mfma(bfr, af, acc);
        }
        // transposed accumulator (lane = row, register group g = channels 8 g + 4 fhalf ..) -> LDS -> 8 channels of a row per lane
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<f32x4*>(&ep[frow * EPS + 8 * g + 4 * fhalf]) = f32x4{acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
        __builtin_amdgcn_wave_barrier();
        const rsrc_t rs_out = __builtin_amdgcn_make_buffer_rsrc((void*)(Out + (long)m0 * p.omap.S1 + p.omap.off), 0, 0x7FFFFF00u, 0x00020000);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int row = h * 16 + er, ml = wm0 + row, nl = wn0 + ec;
            const f32x4 x0 = *reinterpret_cast<const f32x4*>(&ep[row * EPS + ec]);
            const f32x4 x1 = *reinterpret_cast<const f32x4*>(&ep[row * EPS + ec + 4]);
            float t[8];
#pragma unroll
            for (int e = 0; e < 4; ++e) { t[e] = x0[e] + b0[e]; t[4 + e] = x1[e] + b1[e]; }
            if (p.act == ACT_RELU) {
#pragma unroll
                for (int e = 0; e < 8; ++e) t[e] = relu_f(t[e]);
            }
            const u32x4 o = u32x4{F::pack2(t[0], t[1]), F::pack2(t[2], t[3]), F::pack2(t[4], t[5]), F::pack2(t[6], t[7])};
            __builtin_amdgcn_raw_buffer_store_b128(o, rs_out, (m0 + ml < p.M && nl < p.N) ? (unsigned)(ml * (int)p.omap.S1 + nl) * 2u : OOB, 0, 0);
        }
        __syncthreads();                              // every wave has read As: the next tile's runs may overwrite it
    }
#endif
}

template <int KS, class F>
__global__ __launch_bounds__(256, 2) void igemm_bf16_stem_stream_kernel(GemmArgs p, int ntiles) {
    igemm_bf16_stem_stream_body<KS, F, false>(p, ntiles, nullptr);
}
template <int KS, class F>
__global__ __launch_bounds__(256, 2) void igemm_bf16_stem_stream_u8_kernel(GemmArgs p, int ntiles, U8Input in) {
    igemm_bf16_stem_stream_body<KS, F, true>(p, ntiles, &in);
}

// =====================================================================================================
// host side: one route, one prepared problem, one launch site per kernel
// =====================================================================================================
// what the three 16-bit kernels take: fp32 NHWC image (Cin % 4 != 0), fp32 packed weights [N][Kpad32], bf16 / fp16 NHWC result; no residual.
static bool gemm_bf16_smallc_ok(const GemmArgs& a) {
    return a.conv && a.out_bf16 && !a.res && a.omap.G == 1 && a.N % 4 == 0 && a.omap.S1 % 4 == 0 && a.omap.off % 4 == 0 &&
           a.Kpad % 32 == 0 && a.act != ACT_GELU;
}

// compute_dtype = bf16 / fp16 (the op writes 16-bit activations): the stem runs on the 16-bit MFMA too; CAPF_STEM_BF16=0 keeps it fp32
static bool stem_on_bf16(const GemmArgs& a) {
    static const int on = [] { const char* e = diag_env("CAPF_STEM_BF16"); return e ? atoi(e) : 1; }();
    return on && gemm_bf16_smallc_ok(a);
}

static int stem_runs_ks(const GemmArgs& a) {     // 7 / 3: the run-based stem kernel applies; 0: the element-wise gather kernel
    static const int v2 = [] { const char* e = diag_env("CAPF_STEM_V2"); return e ? atoi(e) : 1; }();     // A/B runs only
    if (!v2 || a.Cin != 3 || a.pad != a.ks / 2 || a.K != a.ks * a.ks * 3) return 0;
    if (a.ks == 7 && a.Kpad >= 6 * 21 + 24) return 7;
    if (a.ks == 3 && a.Kpad >= 2 * 9 + 12) return 3;
    return 0;
}

static bool stem_stream_on() {
    static const int on = [] { const char* e = diag_env("CAPF_STEM_STREAM"); return e ? atoi(e) : 1; }();        // A/B runs only
    return on;
}
// the persistent streaming stems: one 64-column tile, 8- (16-bit) / 4-channel (fp32) vector stores, 32-bit float offsets into the image tensor
static bool stem_stream_ok(const GemmArgs& a) {
    const long total = (long)(a.M / (a.Ho * a.Wo)) * a.H * a.W * 3;
    return stem_stream_on() && a.N <= 64 && a.N % 8 == 0 && a.omap.S1 % 8 == 0 && a.omap.off % 8 == 0 && total < (1L << 29) && a.Wo >= 4;
}
static bool stem_stream_f32_ok(const GemmArgs& a) {
    const long total = (long)(a.M / (a.Ho * a.Wo)) * a.H * a.W * 3;
    return stem_stream_on() && a.conv && a.Cin == 3 && a.ks == 3 && a.pad == 1 && a.K == 27 && a.Kpad >= 2 * 9 + 12 && !a.res && !a.out_bf16 &&
           !a.rscale && a.act != ACT_GELU && a.omap.G == 1 && a.rmap.G <= 1 && a.N <= 64 && a.N % 4 == 0 && a.omap.S1 % 4 == 0 &&
           a.omap.off % 4 == 0 && total < (1L << 29) && a.Wo >= 4;
}

StemRoute gemm_stem_route(const GemmArgs& a) {
    if (stem_on_bf16(a)) {
        const int ks = stem_runs_ks(a);
        if (!ks) return {StemKernel::B16_SMALLC, 0};
        return {stem_stream_ok(a) ? StemKernel::B16_STREAM : StemKernel::B16_RUNS, ks};
    }
    if (stem_stream_f32_ok(a)) return {StemKernel::F32_STREAM, 3};
    return {StemKernel::F32_SMALLC, 0};
}

const char* gemm_stem_kernel_name(const GemmArgs& a, bool u8) {
    struct Names { char s[5][2][48]; };
    static const Names names = [] {
        static const char* const base[5] = {"igemm_f32_smallc<w4,128x64", "igemm_f32_stem_stream<w4,64x64", "igemm_bf16_smallc<w4,128x64",
                                            "igemm_bf16_stem<w4,128x64", "igemm_bf16_stem_stream<w4,64x64"};     // in StemKernel's order
        Names n;
        for (int k = 0; k < 5; ++k)
            for (int u = 0; u < 2; ++u) snprintf(n.s[k][u], sizeof(n.s[k][u]), "%s%s>", base[k], u ? ",u8" : "");
        return n;
    }();
    const StemKernel k = gemm_stem_route(a).kernel;
    const char* name = names.s[(int)k][u8 ? 1 : 0];
    return stem_is_16bit(k) ? fmt_kernel_name(name, a.f16) : name;
}

// Anything but a conv these kernels address -- and, from a uint8 crop, but a Cin = 3 conv whose frame count matches the descriptor's mode -- is
// an error, never another kernel
bool gemm_stem_ok(const GemmArgs& a, const U8Input* in) {
    if (!a.conv || a.M <= 0 || a.N <= 0 || a.Kpad % BK != 0 || a.splits > 1 || a.act == ACT_GELU) return false;
    // the epilogues' fast paths address out / res with 32-bit element offsets from their bases
    if (a.omap.G == 1 && (double)a.M * (double)a.omap.S1 >= 4.0e9) return false;
    if (a.res && a.rmap.G == 1 && (double)a.M * (double)a.rmap.S1 >= 4.0e9) return false;
    if (in) {
        if (a.Cin != 3 || a.Ho <= 0 || a.Wo <= 0 || a.M % (a.Ho * a.Wo) != 0) return false;
        if (!in->img || in->Bsrc <= 0 || in->mode < 0 || in->mode > 2) return false;
        if (a.M / (a.Ho * a.Wo) != (in->mode == 2 ? 2 * in->Bsrc : in->Bsrc)) return false;
    }
    // a 16-bit result that the 16-bit kernels refuse falls to igemm_f32_smallc, whose 16-bit store is bf16 whatever GemmArgs::f16 says: not for fp16
    return !(a.out_bf16 && a.f16 && !stem_is_16bit(gemm_stem_route(a).kernel));
}

// the problem as the kernels read it
static GemmArgs stem_args(const GemmArgs& a_in, bool u8) {
    GemmArgs a = a_in;
    if (u8) a.A = nullptr;
    a.split_ws = nullptr; a.split_cnt = nullptr;
    a.splits = 1; a.cps = a.Kpad / BK; a.split_stride = 0;
    if (a.rs_div <= 0) a.rs_div = 1;
    a.fd_hw = make_fastdiv((unsigned)(a.Ho * a.Wo));
    a.fd_wo = make_fastdiv((unsigned)a.Wo);
    a.spread = 0ull;
    for (int kh = 0; kh < a.ks && kh * a.ks < 64; ++kh) a.spread |= 1ull << (kh * a.ks);
    return a;
}

// grid of the persistent streaming kernels over `ntiles` 64-pixel tiles: two blocks per CU, halved while every block still gets a tile (always
// a multiple of 8: the kernels' per-XCD walk) ...
static dim3 stem_stream_grid(int ntiles) {
    int blocks = 512;
    while (blocks > 8 && blocks / 2 >= ntiles) blocks /= 2;
    return dim3(blocks);
}
// ... and of the 128 x 64 tile kernels (64-pixel tiles -- 47 KiB, three blocks per CU for the 7x7 -- measured slower: 0.50 -> 0.59 ms for CPN,
// 0.30 -> 0.35 for HRNet)
static dim3 stem_tile_grid(const GemmArgs& a) { return dim3(((a.M + 127) / 128) * ((a.N + 63) / 64)); }

// one kernel's launch site: its float entry point, or -- from a uint8 crop -- its U8 one with the descriptor behind the float form's arguments
template <class KF, class KU, class... Extra>
static void launch_form(KF float_kernel, KU u8_kernel, dim3 grid, hipStream_t s, const U8Input* in, const GemmArgs& a, Extra... extra) {
    if (in) hipLaunchKernelGGL(u8_kernel, grid, dim3(256), 0, s, a, extra..., *in);
    else hipLaunchKernelGGL(float_kernel, grid, dim3(256), 0, s, a, extra...);
}
template <class Fn>
static void with_stem_ks(int ks, Fn&& fn) {      // the run-based kernels' KS (7 / 3: stem_runs_ks) as a constant
    if (ks == 7) fn(std::integral_constant<int, 7>{});
    else fn(std::integral_constant<int, 3>{});
}

hipError_t launch_gemm_stem(const GemmArgs& a_in, const U8Input* in, hipStream_t s) {
    if (!gemm_stem_ok(a_in, in)) return hipErrorInvalidValue;
    const StemRoute r = gemm_stem_route(a_in);
    const GemmArgs a = stem_args(a_in, in != nullptr);
    const int ntiles = (a.M + 63) / 64;
    const dim3 stream = stem_stream_grid(ntiles), tiles = stem_tile_grid(a);
    if (r.kernel == StemKernel::F32_SMALLC)
        launch_form(igemm_f32_smallc_kernel<128, 64, 64, 32>, igemm_f32_smallc_u8_kernel<128, 64, 64, 32>, tiles, s, in, a);
    else if (r.kernel == StemKernel::F32_STREAM)
        launch_form(igemm_f32_stem_stream_kernel<3>, igemm_f32_stem_stream_u8_kernel<3>, stream, s, in, a, ntiles);
    else
        with_fmt(a.f16, [&](auto f) {
            using F = decltype(f);
            if (r.kernel == StemKernel::B16_SMALLC) launch_form(igemm_bf16_smallc_kernel<F>, igemm_bf16_smallc_u8_kernel<F>, tiles, s, in, a);
            else with_stem_ks(r.ks, [&](auto k) {
                constexpr int KS = decltype(k)::value;
                if (r.kernel == StemKernel::B16_RUNS) launch_form(igemm_bf16_stem_kernel<KS, 128, F>, igemm_bf16_stem_u8_kernel<KS, 128, F>, tiles, s, in, a);
                else launch_form(igemm_bf16_stem_stream_kernel<KS, F>, igemm_bf16_stem_stream_u8_kernel<KS, F>, stream, s, in, a, ntiles);
            });
            return 0;
        });
    return hipGetLastError();
}

}  // namespace capf
