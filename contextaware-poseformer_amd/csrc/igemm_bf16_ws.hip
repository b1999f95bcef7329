// bf16 3x3 / stride-1 / pad-1 convolution on the "2-D halo" tile (igemm_bf16_ws_tile.h): launchers, grouped kernel, weight pack.
// Replaces, for launches that fill the chip, the row-halo tile of igemm_bf16.hip for the BasicBlock convs of HRNet
// (pose_hrnet.py:66-95) and the 3x3 convs of the ResNet-50 / refine bottlenecks (networks/resnet.py:58-93, refineNet.py:3-45).
// Measured alone at batch 256 (tools/bf16_ws.hip; row-halo tile in brackets): 96 ch 32^2 979 TFLOP/s (546), 192 ch 16^2 1107 (671),
// 384 ch 8^2 1108 (776), 48 ch 64^2 605 (411).
#include "igemm_bf16_ws_tile.h"
#include "kernels.h"

namespace capf {

static int ws_ns(int N) { return N % 96 == 0 ? 96 : (N <= 32 ? 32 : 64); }

long bf16_ws_pack_elems(int Cout, int Cin) {
    const int NS = ws_ns(Cout);
    return (long)((Cout + NS - 1) / NS) * (Cin / 16) * 9 * NS * 16;
}

// GemmArgs -> tile geometry; false = not a problem this tile takes
static bool ws_from_args(const GemmArgs& a, WsProblem* p) {
    if (!ws_args_ok(a, 7, a.f32s ? 4.0 : 2.0, a.M)) return false;      // (bf16 rows; fp32 stream: fp32 residual / result.  out_bf16 is not looked at)
    if (!ws_plan(a.M / (a.H * a.W), a.H, a.W, a.Cin, a.N, p)) return false;
    p->x = reinterpret_cast<const unsigned short*>(a.A);
    p->wp = reinterpret_cast<const unsigned short*>(a.Wp3);
    p->bias = a.bias;
    p->res = a.res ? reinterpret_cast<const unsigned short*>(a.res) + a.rmap.off : nullptr;
    p->y = reinterpret_cast<unsigned short*>(a.out) + a.omap.off;
    p->res32 = nullptr;
    p->y32 = nullptr;
    if (a.f32s) {
        p->res = nullptr;
        p->res32 = a.res ? a.res + a.rmap.off : nullptr;
        if (a.out_f32) {
            p->y32 = a.out + a.omap.off;
            p->y = a.out_sh ? static_cast<unsigned short*>(a.out_sh) + a.omap.off : nullptr;
        }
    }
    p->ldy = (int)a.omap.S1;
    p->ldr = a.res ? (int)a.rmap.S1 : (int)a.omap.S1;
    p->relu = a.act == ACT_RELU;
    return true;
}

bool gemm_bf16_ws_ok(const GemmArgs& a) {
    WsProblem p;
    return ws_from_args(a, &p);
}

// Which kernel a conv runs on is a function of the conv ALONE (its shape and batch), never of what else shares its launch: the
// engine's schedules (one chain, two chains, program order) group a level's convs differently and promise identical bits
// (capf.h, tests/test_gpu_ops.py::test_two_chain_schedule_is_bit_identical_to_one_chain).  The HRNet branches of a level have equal
// FLOPs and very different tile counts (1024 ... 64 at batch 64), so the rule is on the problem's work: the tile takes a conv from
// 1 GFLOP up -- below that (HRNet-32 under batch ~14, HRNet-48 under ~6) a level is a handful of 256-pixel tiles and the ring
// kernel's 64 x 64 tiles fill the chip better.  (diag builds: CAPF_BF16_WS_MIN_MFLOP, CAPF_BF16_WS_MIN_BATCH)
// Round 6 (tools/sweep_thresholds.py, tools/ws_sweep.py -> profiles/r06_threshold_sweep.txt): the FLOP rule alone let the tile in far too
// early -- HRNet-48 at batch 8 / 16 ran 21 % / 10 % SLOWER with it than on the row-halo / ring kernels, CPN at batch 4 - 16 5 %; the three
// backbones cross over between batch 16 and 32, where a launch's 256-pixel tiles start to fill the chip's 512 slots.  So: 1 GFLOP AND batch 24.
// The engine's plan applies the rule, once per conv (Engine::tile_takes); the launcher runs what it is handed
bool bf16_tile_big_enough(int B, int H, int W, int Cin, int Cout) {
    static const double min_flop = [] { const char* e = diag_env("CAPF_BF16_WS_MIN_MFLOP"); return (e ? atof(e) : 1000.0) * 1e6; }();
    static const long min_batch = [] { const char* e = diag_env("CAPF_BF16_WS_MIN_BATCH"); return e ? atol(e) : 24L; }();
    return B >= min_batch && 2.0 * (double)B * H * W * Cout * 9.0 * Cin >= min_flop;
}

// The grid: kernels.h "Grouped launch" (what was measured against it on this kernel stands there).
struct WsGroupArgs {
    WsProblem g[MAXG];
    GroupLayout lay;
    int n;
};
static_assert(sizeof(WsGroupArgs) == MAXG * sizeof(WsProblem) + (2 * MAXG + 2) * sizeof(int), "kernel argument layout");

template <bool F32S, class F>
__device__ __forceinline__ void ws_group_body(const WsGroupArgs& ga, unsigned char* ws_lds) {
#if defined(__HIP_DEVICE_COMPILE__)
    const GroupSlot t = group_slot(ga.lay, ga.n, blockIdx.x);
    if (!t.live) return;
    const WsProblem& p = ga.g[t.pi];
    switch (p.NS) {
        case 96: igemm_bf16_ws_tile<3, F32S, F>(p, t.bid, ws_lds); break;
        case 64: igemm_bf16_ws_tile<2, F32S, F>(p, t.bid, ws_lds); break;
        default: igemm_bf16_ws_tile<1, F32S, F>(p, t.bid, ws_lds); break;
    }
#endif
}

__global__ __launch_bounds__(256, 2) void igemm_bf16_group_ws_kernel(WsGroupArgs ga) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) unsigned char ws_lds[];
    ws_group_body<false, Bf16Fmt>(ga, ws_lds);
#endif
}

// ... on fp16 elements (GemmArgs::f16)
__global__ __launch_bounds__(256, 2) void igemm_f16_group_ws_kernel(WsGroupArgs ga) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) unsigned char ws_lds[];
    ws_group_body<false, F16Fmt>(ga, ws_lds);
#endif
}

// ... with the fp32-stream epilogue (every problem of the launch has GemmArgs::f32s)
__global__ __launch_bounds__(256, 2) void igemm_bf16_group_ws_stream_kernel(WsGroupArgs ga) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) unsigned char ws_lds[];
    ws_group_body<true, Bf16Fmt>(ga, ws_lds);
#endif
}

hipError_t launch_gemm_bf16_ws_group(const GemmArgs* list, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n > MAXG) return hipErrorInvalidValue;
    WsProblem p[MAXG];
    int tiles[MAXG], order[MAXG], max_ns = 32;
    double cost[MAXG];
    const bool stream = list[0].f32s != 0;
    const int f16 = list[0].f16;                                   // (one element format per launch; the fp32-stream epilogue is bf16 plans' only)
    if (stream && f16) return hipErrorInvalidValue;
    for (int i = 0; i < n; ++i) {
        if (!list[i].Wp3 || !ws_from_args(list[i], &p[i]) || (list[i].f32s != 0) != stream || list[i].f16 != f16) return hipErrorInvalidValue;
        tiles[i] = p[i].tiles_m * p[i].NSL;
        cost[i] = (double)(p[i].C / 16) * p[i].NS;               // a tile's K loop
        if (p[i].NS > max_ns) max_ns = p[i].NS;
    }
    WsGroupArgs ga{};
    ga.n = n;
    const int start = group_layout(ga.lay, n, tiles, cost, order);
    for (int i = 0; i < n; ++i) ga.g[i] = p[order[i]];
    const size_t lds_bytes = 2 * (size_t)ws_stage_bytes(max_ns);
    static DynLdsAttr attr_once, attr_f16, attr_stream;
    if (stream) {
        const hipError_t attr = attr_stream.ensure(reinterpret_cast<const void*>(&igemm_bf16_group_ws_stream_kernel), 2 * ws_stage_bytes(96));
        if (attr != hipSuccess) return attr;
        hipLaunchKernelGGL(igemm_bf16_group_ws_stream_kernel, dim3(start), dim3(256), lds_bytes, s, ga);
        return hipGetLastError();
    }
    if (f16) {
        const hipError_t attr = attr_f16.ensure(reinterpret_cast<const void*>(&igemm_f16_group_ws_kernel), 2 * ws_stage_bytes(96));
        if (attr != hipSuccess) return attr;
        hipLaunchKernelGGL(igemm_f16_group_ws_kernel, dim3(start), dim3(256), lds_bytes, s, ga);
        return hipGetLastError();
    }
    const hipError_t attr = attr_once.ensure(reinterpret_cast<const void*>(&igemm_bf16_group_ws_kernel), 2 * ws_stage_bytes(96));
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(igemm_bf16_group_ws_kernel, dim3(start), dim3(256), lds_bytes, s, ga);
    return hipGetLastError();
}

// Measured and not adopted (commit 899a361 "persistent weight-resident form", profiles/r04_pmc_bf16_ws_level.txt): a persistent block per CU
// for the narrow branch (Cin 48: whole filter staged once, the next tile's pixels in flight under the current tile, one barrier per
// tile) -- bit-identical, 92 -> 83 us alone, but nothing end to end (cfg2 14.23k vs 14.19k frames/s): with one wave per SIMD its K
// loop, its VALU-heavy epilogue and its waits are strictly serial.

const char* gemm_bf16_ws_kernel_name(const GemmArgs& a) {
    const int ns = ws_ns(a.N);
    return fmt_kernel_name(ns == 96 ? "igemm_bf16_ws<w4,256x96,conv>" : (ns == 64 ? "igemm_bf16_ws<w4,256x64,conv>" : "igemm_bf16_ws<w4,256x32,conv>"), a.f16);
}

// BN fold + re-layout for the tile: Wp[slice][Cin / 16][tap][n][quad position][8] (ws_pack_decode) = bf16 of the folded fp32 weight
// (bn_fold_w3x3: rows beyond Cout zero; bias as launch_pack_conv)
template <class F>
__global__ void pack_conv_bf16_ws_kernel(const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta,
                                         const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                         unsigned short* __restrict__ Wp, float* __restrict__ bias, int Cout, int Cin, int NS, long total) {
    const int ncc = Cin / 16;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const WsPackIdx d = ws_pack_decode(i, NS, ncc);
        Wp[i] = F::narrow(bn_fold_w3x3(w, gamma, beta, mean, var, eps, bias, Cout, Cin, d.ng, d.c, d.tap, d.first));
    }
}

hipError_t launch_pack_conv_bf16_ws(const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                                    float eps, void* Wp_bf16, float* bias, int Cout, int Cin, hipStream_t s, int f16) {
    if (Cin % 16 != 0 || Cout <= 0) return hipErrorInvalidValue;
    const long total = bf16_ws_pack_elems(Cout, Cin);
    with_fmt(f16, [&](auto f) {
        hipLaunchKernelGGL(pack_conv_bf16_ws_kernel<decltype(f)>, dim3(grid_1d(total)), dim3(256), 0, s, w, gamma, beta, mean, var, eps,
                           static_cast<unsigned short*>(Wp_bf16), bias, Cout, Cin, ws_ns(Cout), total);
        return 0;
    });
    return hipGetLastError();
}

}  // namespace capf
