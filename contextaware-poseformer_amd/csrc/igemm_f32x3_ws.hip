// fp32 3x3 / stride-1 / pad-1 convolution on the bf16 matrix pipe, operands split into three bf16 pieces (igemm_f32x3_ws_tile.h):
// launcher, grouped kernel, weight pack.  Under CAPF_PLAN_F32X3_EXACT the engine (Engine::gemm_family) runs the BasicBlock convs of HRNet
// under compute_dtype = fp32 (pose_hrnet.py:66-95) here wherever a launch fills the chip; the default plan runs them on the two-fp16-piece
// tile of igemm_f32h2_ws.hip instead.  fp32 tensors in and out, results to fp32 accumulation order (tools/f32x3_ws.hip: 2.6e-7 of the sum
// of |terms| at worst against an fp64 evaluation, rms 1.4e-8; the F(4,3) Winograd kernel: 1e-5).
// Measured alone (tools/f32x3_ws.hip; F(4,3) kernel in brackets), batch 64: 32 ch 64^2 37.6 us (43.6), 64 ch 32^2 31.6 (38.0),
// 128 ch 16^2 30.6 (48.5), 256 ch 8^2 50.8 (81.3); batch 512: 352 (341), 271 (281), 236 (243), 229 (248).
#include "igemm_f32x3_ws_tile.h"
#include "kernels.h"

namespace capf {

static constexpr int X3_NS = 32;               // output channels per tile: two blocks per CU (67.6 KiB of LDS each)

long f32x3_pack_elems(int Cout, int Cin) { return x3_pack_elems(Cout, Cin, X3_NS); }

// GemmArgs -> tile geometry; false = not a problem this tile takes
static bool x3_from_args(const GemmArgs& a, X3Problem* q) {
    if (a.out_bf16 || !ws_args_ok(a, 3, 4.0, a.M)) return false;       // (fp32 rows, fp32 out only)
    if (!x3_plan(a.M / (a.H * a.W), a.H, a.W, a.Cin, a.N, X3_NS, q)) return false;
    q->x = a.A;
    q->g.wp = reinterpret_cast<const unsigned short*>(a.Wp3);
    q->g.bias = a.bias;
    q->res = a.res ? a.res + a.rmap.off : nullptr;
    q->y = a.out + a.omap.off;
    q->g.ldy = (int)a.omap.S1;
    q->g.ldr = a.res ? (int)a.rmap.S1 : (int)a.omap.S1;
    q->g.relu = a.act == ACT_RELU;
    return true;
}

bool gemm_f32x3_ok(const GemmArgs& a) {
    X3Problem q;
    return x3_from_args(a, &q);
}

// As for the bf16 tile (igemm_bf16_ws.hip): which kernel a conv runs on is a function of the conv ALONE, so that every schedule of
// the engine produces the same bits.  From 370 MFLOP and batch 5 up (the HRNet-32 branch convs -- 75.5 MFLOP per frame -- from batch 5:
// round 5's sweep with the two-piece tile, ms per forward at batch 4 / 5 / 6 / 7 / 8: 2.89 (direct kernels) / 2.79 / 2.85 / 2.96 / 3.01; the rule
// of rounds 4-5, 400 MFLOP and batch 6, left batch 5 on the direct kernels at 3.62.  Round 4's numbers for the three-piece tile, ms per forward
// against the direct kernel with split-K / the Winograd kernels: batch 6 3.67 / 3.80 / -, 8 3.76 / 3.90 / 5.47, 16 4.27 / 4.75 / 5.86,
// 24 4.90 / 6.08 / 6.37; below, the direct kernel wins: batch 4 3.49 / 2.92).  (diag builds: CAPF_F32X3_MIN_MFLOP)
bool f32_tile_big_enough(int B, int H, int W, int Cin, int Cout) {
    static const double min_flop = [] { const char* e = diag_env("CAPF_F32X3_MIN_MFLOP"); return (e ? atof(e) : 370.0) * 1e6; }();
    return B >= 5 && 2.0 * (double)B * H * W * Cout * 9.0 * Cin >= min_flop;
}

struct X3GroupArgs {
    X3Problem g[MAXG];
    GroupLayout lay;
    int n;
};
static_assert(sizeof(X3GroupArgs) == MAXG * sizeof(X3Problem) + (2 * MAXG + 2) * sizeof(int), "kernel argument layout");

__global__ __launch_bounds__(256, 2) void igemm_f32x3_group_ws_kernel(X3GroupArgs ga) {
#if defined(__HIP_DEVICE_COMPILE__)
    extern __shared__ __attribute__((aligned(16))) unsigned char x3_lds[];
    const GroupSlot t = group_slot(ga.lay, ga.n, blockIdx.x);
    if (!t.live) return;
    igemm_f32x3_ws_tile<X3_NS / 32>(ga.g[t.pi], t.bid, x3_lds);
#endif
}

hipError_t launch_gemm_f32x3_group(const GemmArgs* list, int n, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n > MAXG) return hipErrorInvalidValue;
    X3Problem q[MAXG];
    int tiles[MAXG], order[MAXG];
    double cost[MAXG];
    for (int i = 0; i < n; ++i) {
        if (!list[i].Wp3 || list[i].x3_h2 || !x3_from_args(list[i], &q[i])) return hipErrorInvalidValue;
        tiles[i] = q[i].g.tiles_m * q[i].g.NSL;
        cost[i] = q[i].g.C;                                 // a tile's K loop
    }
    X3GroupArgs ga{};
    ga.n = n;
    const int start = group_layout(ga.lay, n, tiles, cost, order);
    for (int i = 0; i < n; ++i) ga.g[i] = q[order[i]];
    static DynLdsAttr attr_once;
    const hipError_t attr = attr_once.ensure(reinterpret_cast<const void*>(&igemm_f32x3_group_ws_kernel), x3_lds_bytes(X3_NS));
    if (attr != hipSuccess) return attr;
    hipLaunchKernelGGL(igemm_f32x3_group_ws_kernel, dim3(start), dim3(256), x3_lds_bytes(X3_NS), s, ga);
    return hipGetLastError();
}

const char* gemm_f32x3_kernel_name() { return "igemm_f32x3_group_ws"; }

// BN fold + three-way split + re-layout for the tile: with v the folded fp32 weight (bn_fold_w3x3: the value launch_pack_conv folds, rows
// beyond Cout zero, bias as launch_pack_conv), piece 0 = bf16(v), piece 1 = bf16(v - piece 0), piece 2 = bf16(v - piece 0 - piece 1) -- exact
// remainders, v = piece 0 + piece 1 + piece 2 -- at Wp[slice][Cin / 16][piece][tap][n][quad position][8] (ws_pack_decode)
__global__ void pack_conv_f32x3_kernel(const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta,
                                       const float* __restrict__ mean, const float* __restrict__ var, float eps,
                                       unsigned short* __restrict__ Wp, float* __restrict__ bias, int Cout, int Cin, int NS, long total) {
    const int ncc = Cin / 16;
    for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {   // i: one weight, its three pieces
        const WsPackIdx d = ws_pack_decode(i, NS, ncc);
        float v = bn_fold_w3x3(w, gamma, beta, mean, var, eps, bias, Cout, Cin, d.ng, d.c, d.tap, d.first);
        const long piece = 9L * NS * 16;
        const long base = ((long)(d.sl * ncc + d.cc) * 3) * piece + ((long)d.tap * NS + d.n) * 16 + d.qp * 8 + d.e;
#pragma unroll
        for (int pc = 0; pc < 3; ++pc) {
            const unsigned short b = to_bf16(v);
            Wp[base + pc * piece] = b;
            v -= __uint_as_float((unsigned)b << 16);
        }
    }
}

hipError_t launch_pack_conv_f32x3(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                                  void* Wp_bf16, float* bias, int Cout, int Cin, hipStream_t s) {
    if (Cin % 16 != 0 || Cout <= 0) return hipErrorInvalidValue;
    const long total = f32x3_pack_elems(Cout, Cin) / 3;
    hipLaunchKernelGGL(pack_conv_f32x3_kernel, dim3(grid_1d(total)), dim3(256), 0, s, w, gamma, beta, mean, var, eps,
                       static_cast<unsigned short*>(Wp_bf16), bias, Cout, Cin, X3_NS, total);
    return hipGetLastError();
}

}  // namespace capf
