// Launcher declarations for the gfx950 kernels (internal; the public ABI is include/capf.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <stdlib.h>

#include "relu.h"
#include "fmt16.h"    // the 16-bit element formats (bf16 / fp16) of the 16-bit kernel families
#include "pixel_rule.h"   // the input normalisation rule and the uint8 image descriptor of the stem kernels' U8 forms
#include "capf.h"      // capf_optim_report: the record the guarded AdamW kernel writes is the public one

namespace capf {

// A/B and tuning switches read the environment ONLY in the diagnostic build (make DIAG=1 -> tools/ab/libcapf_diag.so,
// -DCAPF_DIAG, loaded through CAPF_LIB by the tools); the product library ignores them, so an exported variable can never
// change a production plan or its numerics.  What tests need to steer is an explicit field: capf_config::plan_flags.
inline const char* diag_env(const char* name) {
#ifdef CAPF_DIAG
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// Bilinear corner of F.grid_sample(mode='bilinear', align_corners=True) at normalised coordinates (gx, gy): the integer NW
// corner and the fractional weights of the +1 corners, exactly as ATen computes them (GridSampler.h:27-36, 58-60, 143-171:
// ((g + 1) / 2) * (size - 1); padding 'border' clips the COORDINATE to [0, size - 1] before floor, 'zeros' keeps it).  The
// result feeds an index gather that must be bit-exact, so every translation unit that instantiates this is built with
// -ffp-contract=off (csrc/Makefile: lifter.hip, lifter_fused.hip) -- no FMA contraction, IEEE division.  The function also switches
// contraction off for itself: train_kernels.hip is built without that flag, and there x - floor(x) of a product became an fma in one
// kernel and not in another (the two summation forms of the map gradient must get the same weights, the forward's).
struct BilinearCorner {
    int x0, y0;
    float wx1, wy1;
};
#if defined(__HIPCC__)
template <bool BORDER>
__device__ __forceinline__ BilinearCorner bilinear_corner(float gx, float gy, int H, int W) {
#pragma clang fp contract(off)
    float x = ((gx + 1.0f) / 2.0f) * (float)(W - 1);
    float y = ((gy + 1.0f) / 2.0f) * (float)(H - 1);
    if (BORDER) {   // clip_coordinates: min(size - 1, max(x, 0)) before floor
        x = fminf((float)(W - 1), fmaxf(x, 0.0f));
        y = fminf((float)(H - 1), fmaxf(y, 0.0f));
    }
    const float xf = floorf(x), yf = floorf(y);
    BilinearCorner c;
    c.x0 = (int)xf;
    c.y0 = (int)yf;
    c.wx1 = x - xf;
    c.wy1 = y - yf;
    return c;
}
#endif

// addr(m) = (m / G) * S1 + (m % G) * S2 + off   (elements).  G == 1 -> plain leading dimension S1.
struct RowMap {
    int G;
    long S1, S2, off;
};
inline RowMap row_ld(long ld, long off = 0) { return RowMap{1, ld, 0, off}; }

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2 };

// n / d for 0 <= n < 2^31:  q = (umulhi(n, mul) + n) >> shift   (host: make_fastdiv)
struct FastDiv {
    unsigned mul, shift;
};
FastDiv make_fastdiv(unsigned d);

// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE property of a kernel: launchers that need more than the 64 KiB default of
// dynamic LDS keep one of these per kernel (a function-local static) and call ensure() before every launch -- one hipGetDevice, and the
// attribute call the first time a device is seen (a handle per device in one process: capf_create takes a device index)
struct DynLdsAttr {
    unsigned long long seen = 0;     // bit d: set on device d (a benign race: setting the attribute twice is harmless)
    hipError_t ensure(const void* kernel, int bytes) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        if (dev >= 0 && dev < 64 && ((seen >> dev) & 1ull)) return hipSuccess;
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e == hipSuccess && dev >= 0 && dev < 64) seen |= 1ull << dev;
        return e;
    }
};

// One implicit-GEMM problem:  out[m, n] = act( sum_k A[m, k] * Wp[n, k] + bias[n] + res[m, n] )
//   conv mode: A[m, k] gathered from an NHWC tensor, m = (b, ho, wo), k = (kh, kw, ci)
//   rows mode: A[m, k] = A[amap(m) + k]
struct GemmArgs {
    const float* A;
    const float* Wp;    // packed weights [N][Kpad], K-contiguous, zero padded to Kpad (multiple of 32)
    const float* Wp2;   // bf16 3x3 stride-1 convs: the same weights in the row-halo layout ([N][9 * Cin], igemm_bf16.hip), or
                        // nullptr; launch_gemm_bf16 / _group switch to that kernel for launches of >= 2048 tiles
    const float* Wp3;   // bf16 3x3 stride-1 convs: the same weights in the 2-D halo tile's layout (igemm_bf16_ws.hip), or nullptr.
                        // fp32 3x3 stride-1 convs: the weights as the split-fp32 tile's pieces, or nullptr -- three bf16 pieces
                        // (igemm_f32x3_ws.hip, launch_pack_conv_f32x3) or, with x3_h2 set, two block-scaled fp16 pieces (igemm_f32h2_ws.hip,
                        // launch_pack_conv_f32h2).  Read by the tile launchers alone; who calls them decides (Engine::gemm_family)
    int x3_h2;          // which pieces Wp3 holds: each tile launcher refuses the other's pack.  (GemmArgs is the fp32 / bf16 / Winograd kernels'
                        // argument: a member in front of the ones they read cannot leave without moving those and changing their code)
    const float* Wh2;   // the same weights as the two-fp16-piece pack of igemm_f32h2.hip (launch_pack_f32h2_gemm: Wp's [N][Kpad] geometry, then [N]
                        // inverse channel scales), or nullptr: launch_gemm_f32 / _group run the problem on that kernel where gemm_f32h2g_ok()
                        // accepts it (the HBM-bound pointwise kernels keep theirs)
    const float* bias;  // [N] or nullptr
    const float* res;   // residual, addressed by rmap, or nullptr
    float* out;         // addressed by omap
    int M, N, K, Kpad;
    int conv;           // 1 = conv mode
    int Cin, H, W, Ho, Wo, ks, stride, pad;
    RowMap amap, omap, rmap;
    int act;
    FastDiv fd_hw, fd_wo;   // filled by launch_gemm_f32 (conv mode): division by Ho*Wo and by Wo
    unsigned long long spread;   // conv mode: bits kh*ks set for kh < ks (tap-mask construction)
    const float* rscale;    // optional per-row scale of (acc + bias): rscale[m / rs_div] (DropPath), or nullptr
    int rs_div;
    int splits, cps;        // split-K (rows mode): grid.y slices of `cps` chunks, slab s at out + s*split_stride
    long split_stride;
    int out_bf16;           // small-Cin stem kernel only: fp32 image in, bf16 activations out
    int f16;                // 16-bit kernels: the element format of every 16-bit tensor and weight pack of the problem -- 0 bf16, 1 fp16 (Bf16Fmt /
                            // F16Fmt above; every problem of a grouped launch carries the same one).  The fp32 kernels do not look at it
    // conv-mode split-K with an in-kernel, deterministic reduction (small batches: a long-K conv with a handful of tiles):
    // slice ky writes its raw partial tile to split_ws + ky * split_stride ([M][N]); the LAST slice to finish a tile (a
    // device-scope counter per tile, self-resetting) sums the slices in order 0..splits-1 and runs the epilogue
    float* split_ws;
    int* split_cnt;
    long split_ws_elems;    // capacity of the scratch the caller lends (floats / counters); the launchers carve it up
    int split_cnt_elems;
    const float* ln_g;      // rows mode: LayerNorm the A rows over their K columns on the fly (gamma, beta [K]); nullptr = off
    const float* ln_b;
    float ln_eps;
    // bf16 conv mode: out = act(acc + bias (+ res)) + bilinear_upsample(up) -- a map [B][up_H][up_W][N] (bf16, dense) resized to the conv's
    // Ho x Wo with align_corners = True and added AFTER the activation (CPN globalNet.py:66: lateral + upsampled path), in the epilogue of
    // igemm_bf16_kernel<..., UPADD>; nullptr = off.  up_sh / up_sw = (up_H - 1) / (Ho - 1), (up_W - 1) / (Wo - 1) as launch_bilinear_resize has them
    const void* up;
    int up_H, up_W;
    float up_sh, up_sw;
    // the two-fp16-piece conv tile only (igemm_f32h2_ws_tile.h, PLANES): A holds the producer's fp16 planes and h2_ein their [tile][chunk]
    // scale exponents / out is written as planes and h2_eout receives the exponents.  nullptr = plain fp32 tensors
    const int* h2_ein;
    int* h2_eout;
    const unsigned* h2_utab;     // ... and the map geometry's unit table (f32h2_unit_table; nullptr: the prologue computes its addresses)
    // bf16 convs of a CAPF_PLAN_BF16_F32_STREAM plan (the *_stream kernels of igemm_bf16.hip / igemm_bf16_ws.hip; every problem of a launch or none):
    // res, if any, is fp32; out_f32 = 1: out is fp32 and out_sh (may be nullptr) receives its bf16 rounding (RNE, the operand the next conv reads);
    // out_f32 = 0: out is bf16 as usual.  A and the weights stay bf16: the main loops are the default ones, only the epilogue differs
    int f32s;
    int out_f32;
    void* out_sh;
};

// all res blocks of the lifter as one launch (lifter_chain.hip): per block LayerNorm weights, the two-fp16-piece packs of the four projections
// (launch_pack_f32h2_gemm_rows' [N][K floats] of {piece 0 | piece 1} chunks + [N] inverse scales, through launch_res_chain_repack) and their fp32 biases
struct ResBlockW {
    const float *ln1_g, *ln1_b, *wqkv, *bqkv, *wproj, *bproj, *ln2_g, *ln2_b, *wfc1, *bfc1, *wfc2, *bfc2;
};
bool res_chain_ok(int dim, int tokens, int heads, int nblk);
// a projection's two-piece pack re-laid out in MFMA fragment order (same bits; what ResBlockW's w* point at)
hipError_t launch_res_chain_repack(const float* h2g_pack, float* chain_pack, int N, int K, hipStream_t s);
hipError_t launch_res_chain(float* X, int rows, int tokens, int heads, float eps, const ResBlockW* blk, int nblk, hipStream_t s);
hipError_t launch_mlp_chain(float* X, RowMap rows_map, int rows, float eps, const ResBlockW& blk, hipStream_t s);     // the MLP half alone, on mapped rows

// 1-D grid of a grid-stride kernel with 256-thread blocks: one thread per element up to `cap` blocks
inline int grid_1d(long total, int cap = 4096) {
    const long want = (total + 255) / 256;
    return (int)(want < cap ? want : cap);
}

// Eval-mode BatchNorm folded into a conv (pose_hrnet.py:72-75 etc.): y = (conv(x) - mean) / sqrt(var + eps) * gamma + beta ==
// conv_{w * sc}(x) + (beta - mean * sc); gamma == nullptr: no BatchNorm (scale 1, bias 0).  Every weight pack folds through these two,
// so that all layouts of one conv hold the same fp32 values (tests/test_gpu_ops.py checks the packs bit for bit against host folds;
// the expressions are inlined whole, so -ffp-contract sees beta - mean * sc as it always did)
#if defined(__HIPCC__)
__device__ __forceinline__ float bn_scale(const float* __restrict__ gamma, const float* __restrict__ var, float eps, int n) {
    return gamma ? gamma[n] / sqrtf(var[n] + eps) : 1.f;
}
__device__ __forceinline__ float bn_bias(const float* __restrict__ gamma, const float* __restrict__ beta, const float* __restrict__ mean, float sc, int n) {
    return gamma ? beta[n] - mean[n] * sc : 0.f;
}
// one folded weight of a 3x3 filter w [Cout][Cin][3][3] for the 2-D halo tiles' packs (igemm_bf16_ws_tile.h ws_pack_decode: output channel
// ng, input channel c, tap = kh * 3 + kw); rows beyond Cout are zero.  The thread that holds a channel's first element also writes its bias
__device__ __forceinline__ float bn_fold_w3x3(const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta,
                                              const float* __restrict__ mean, const float* __restrict__ var, float eps, float* __restrict__ bias,
                                              int Cout, int Cin, int ng, int c, int tap, bool first) {
    if (ng >= Cout) return 0.f;
    const float sc = bn_scale(gamma, var, eps, ng);
    if (bias && first) bias[ng] = bn_bias(gamma, beta, mean, sc, ng);
    return w[(((long)ng * Cin + c) * 3 + tap / 3) * 3 + tap % 3] * sc;
}
#endif

hipError_t launch_gemm_f32(const GemmArgs& a, hipStream_t s);
// several independent fp32 convs in one grid (see "Grouped launch" below); n <= MAXG, every problem
// must satisfy gemm_f32_groupable()
static constexpr int MAXG = 8;

// =====================================================================================================
// Grouped launch: up to MAXG independent convolutions (the branches of an HRNet module at the same depth,
// the 1x1 / stride-2 convs of a fuse layer) share ONE grid.  A kernel per conv leaves the chip idle while
// its last tiles drain and the next kernel's first tiles wait for their first loads (5-10 us out of ~50),
// and separate streams overlap almost nothing because each kernel fills every CU; inside one grid the
// block scheduler back-fills every freed slot at once and the problems' prologue / epilogue bursts
// interleave.  Every conv family lays its grid out the same way, through the three functions below:
// problems one after the other, longest K loop first (the 256-channel 8x8 branch has 8x the K loop of the
// 32-channel 64x64 one), so that the launch does not end on them; each problem's range padded to a multiple
// of 8 blocks, so that block b of a problem runs on XCD b % 8 and walks that XCD's contiguous eighth of the
// tiles (neighbouring tiles share halo rows and, for several channel slices, the pixel tile in L2) -- the
// XCD-contiguous tile order of the single-problem kernels, per problem.  The order and the padding are a
// function of the problems alone: part of the promise that every schedule computes the same bits (capf.h).
// Measured and rejected (igemm_bf16_group_ws_kernel): dealing the grid out in rounds, every problem in
// proportion to its size, so that memory-bound (48-channel) and matrix-bound (384-channel) tiles are co-resident throughout:
// HRNet-48 level at batch 256 224 -> 247 us, cfg2 14.39k -> 13.9k frames/s.
// Also measured and rejected: two streams -- the matrix-bound problems longest first, the memory-bound 48-channel one dealt evenly
// between them so that a CU's two slots hold one tile of each kind: 226 -> 228 us.  The tiles are bound by their own serial issue /
// wait chains (SQ_WAIT_INST_ANY 35-40 %, SQ_WAIT_ANY 30-36 % of the wave-cycles with two waves per SIMD), not by a shared roof.
// A family's kernel argument is {problems g[MAXG]; GroupLayout; its own per-problem fields; int n}.
struct GroupLayout {
    int start[MAXG + 1];   // first physical block of problem i (multiples of 8); start[n] = the grid size
    int tiles[MAXG];       // real tiles of problem i; blocks beyond them are padding
};
// launch order: order[i] = list index of the i-th problem.  Stable insertion sort by cost, descending (ties keep list order)
inline void group_order(int n, const double* cost, int* order) {
    for (int i = 0; i < n; ++i) {
        int j = i;
        for (; j > 0 && cost[i] > cost[order[j - 1]]; --j) order[j] = order[j - 1];
        order[j] = i;
    }
}
// tiles[i] = tile count of the i-th problem IN LAUNCH ORDER; returns the grid size.  The unused slots n .. MAXG - 1 are empty
// ranges at the end of the grid (no block looks at them: pi < n); a family's own fields there stay as value-initialisation left them
inline int group_fill(GroupLayout& lay, int n, const int* tiles) {
    int start = 0;
    for (int i = 0; i < MAXG; ++i) {
        lay.start[i] = start;
        lay.tiles[i] = i < n ? tiles[i] : 0;
        start += (lay.tiles[i] + 7) & ~7;
    }
    lay.start[MAXG] = start;
    return start;
}
// ... both at once, for families whose tile counts do not depend on the order (tiles[], cost[] by list index)
inline int group_layout(GroupLayout& lay, int n, const int* tiles, const double* cost, int* order) {
    group_order(n, cost, order);
    int sorted[MAXG];
    for (int i = 0; i < n; ++i) sorted[i] = tiles[order[i]];
    return group_fill(lay, n, sorted);
}
#if defined(__HIPCC__)
// physical block b -> problem pi and its tile bid; live = false: a padding block.  (Takes the layout inside the kernel argument by
// reference: the loads stay scalar kernarg loads)
struct GroupSlot { int pi, bid; bool live; };
__device__ __forceinline__ GroupSlot group_slot(const GroupLayout& lay, int n, int b) {
    int pi = 0;
    while (pi + 1 < n && b >= lay.start[pi + 1]) ++pi;                 // block-uniform
    const int l = b - lay.start[pi];
    const int per_xcd = (lay.start[pi + 1] - lay.start[pi]) >> 3;
    const int bid = (l & 7) * per_xcd + (l >> 3);                      // XCD-contiguous tile order inside the problem
    return GroupSlot{pi, bid, bid < lay.tiles[pi]};
}
#endif

// What the three 2-D halo tiles (igemm_bf16_ws.hip, igemm_f32x3_ws.hip, igemm_f32h2_ws.hip) ask of a GemmArgs alike: a 3x3 / stride-1 /
// pad-1 conv with plain row maps, no GELU, no row scale, output / residual rows in 16-byte pieces (align_mask: 7 bf16 or 3 fp32 elements)
// and byte offsets below 2 GB over `rows` rows of elem_bytes elements (the whole tensor, or one tile's rows where the tile addresses
// from per-tile bases).  Whether out_bf16 matters is the caller's: the fp32 tiles reject it, the bf16 tile does not look at it
inline bool ws_args_ok(const GemmArgs& a, int align_mask, double elem_bytes, long rows) {
    if (!a.conv || a.ks != 3 || a.stride != 1 || a.pad != 1 || a.Ho != a.H || a.Wo != a.W || a.act == ACT_GELU || a.rscale ||
        a.omap.G != 1 || (a.res && a.rmap.G != 1) || a.M <= 0 || a.H <= 0 || a.W <= 0 || a.M % (a.H * a.W) != 0)
        return false;
    if ((a.omap.S1 & align_mask) || (a.omap.off & align_mask) || (a.res && ((a.rmap.S1 & align_mask) || (a.rmap.off & align_mask)))) return false;
    return (double)rows * (double)a.omap.S1 * elem_bytes < 2.0e9 && (!a.res || (double)rows * (double)a.rmap.S1 * elem_bytes < 2.0e9);
}
bool gemm_f32_groupable(const GemmArgs& a);
bool gemm_f32_rows_splitk(const GemmArgs& a);        // rows-mode GEMM that launch_gemm_f32 splits along K (few tiles, long K, scratch lent)
hipError_t launch_gemm_f32_group(const GemmArgs* list, int n, hipStream_t s);
// The path launch_gemm_f32 takes for a problem, in its order: the pointwise kernel, the two-fp16-piece GEMM (igemm_f32h2.hip), a lone conv
// split along K on the grouped kernel, a rows-mode GEMM split along K, the Cin = 3 stem (gemm_stem_route below picks its kernel), the tile
// kernel (tile = its configuration).  One decision: the launcher switches on it, gemm_f32_kernel_name names it, the engine counts by it
enum class F32Path { PW, H2G, SPLITK_GROUP, ROWS_SPLITK, STEM, TILE };
struct F32Route { F32Path path; int tile; };
F32Route gemm_f32_route(const GemmArgs& a);
const char* gemm_f32_kernel_name(const GemmArgs& a);   // what rocprofv3 calls the launch of launch_gemm_f32
// fp32 pointwise (1x1 / stride 1) conv for the HBM-bound bottleneck convs of layer1 (igemm_f32_pw.hip): ping-pong schedule,
// coalesced epilogue with prefetched residual; launch_gemm_f32 routes eligible problems (>= 2048 tiles) to it
bool gemm_f32_pw_ok(const GemmArgs& a);
hipError_t launch_gemm_f32_pw(const GemmArgs& a, hipStream_t s);
const char* gemm_f32_pw_kernel_name();
// two pointwise convs back to back (64 -> 256 + residual + ReLU, then 256 -> 64 + ReLU on its output) as ONE launch: the first conv's
// accumulators are the second conv's A operand (igemm_f32_pwchain.hip); bit-identical to the two launches
bool gemm_f32_pwchain_ok(const GemmArgs& a, const GemmArgs& b);
hipError_t launch_gemm_f32_pwchain(const GemmArgs& a, const GemmArgs& b, hipStream_t s);
const char* gemm_f32_pwchain_kernel_name();
// the first bottleneck of a layer1 under compute_dtype = bf16 as one persistent kernel (bneck_bf16.hip): conv1 -> conv2 -> conv3 + downsample
// shortcut + ReLU, intermediates on chip; tap = also store conv1's, conv2's and the downsample's outputs where the unfused ops write them
bool bneck0_bf16_ok(const GemmArgs& c1, const GemmArgs& c2, const GemmArgs& ds, const GemmArgs& c3);
hipError_t launch_bneck0_bf16(const GemmArgs& c1, const GemmArgs& c2, const GemmArgs& ds, const GemmArgs& c3, bool tap, hipStream_t s);
const char* bneck0_bf16_kernel_name(int f16 = 0);
// ... and an identity bottleneck (256 -> 64 -> 64 -> 256, y = relu(conv3 + x)) the same way
bool bneck1_bf16_ok(const GemmArgs& c1, const GemmArgs& c2, const GemmArgs& c3);
hipError_t launch_bneck1_bf16(const GemmArgs& c1, const GemmArgs& c2, const GemmArgs& c3, bool tap, hipStream_t s);
const char* bneck1_bf16_kernel_name(int f16 = 0);
// the bf16 twin (igemm_bf16_pwchain.hip): CPN's / HRNet's layer1 pairs under compute_dtype = bf16
bool gemm_bf16_pwchain_ok(const GemmArgs& a, const GemmArgs& b);
hipError_t launch_gemm_bf16_pwchain(const GemmArgs& a, const GemmArgs& b, hipStream_t s);
const char* gemm_bf16_pwchain_kernel_name(int f16 = 0);

// Winograd-along-W variants of the 3x3 / stride-1 / pad-1 fp32 conv (igemm_wino.hip): same GemmArgs as the direct conv, Wp = weights packed
// by launch_pack_conv_wino -- [N][12 * Cin]: F(2,3), even W; [N][18 * Cin]: F(4,3), W % 4 == 0 (the variant rides in Kpad); needs
// Cin % 32 == 0, N % 4 == 0.  An F(4,3) problem, alone or in a list, runs the F(4,3) group kernel, an F(2,3) one the single-problem or the
// grouped F(2,3) kernel; a problem that is neither is an error
bool gemm_wino_ok(const GemmArgs& a);
hipError_t launch_gemm_wino(const GemmArgs& a, hipStream_t s);
hipError_t launch_gemm_wino_group(const GemmArgs* list, int n, hipStream_t s);
const char* gemm_wino_kernel_name(const GemmArgs& a);
hipError_t launch_pack_conv_wino(const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                                 float eps, float* Wp, float* bias, int Cout, int Cin, hipStream_t s, int variant = 23);

// conv weight fold + pack:  Wp[n][(kh*ks+kw)*Cin+ci] = w[n][ci][kh][kw] * gamma[n]/sqrt(var[n]+eps)
//                            bias[n] = beta[n] - mean[n]*gamma[n]/sqrt(var[n]+eps)
hipError_t launch_pack_conv(const float* w, const float* gamma, const float* beta, const float* mean,
                            const float* var, float eps, float* Wp, float* bias, int Cout, int Cin,
                            int ks, int Kpad, hipStream_t s);
// linear pack: Wp[n][k] = w[n][k] (zero padded to Kpad); rows [n0, n0+N) of the destination
hipError_t launch_pack_conv_bf16(const float* w, const float* gamma, const float* beta, const float* mean,
                                 const float* var, float eps, void* Wp_bf16, float* bias, int Cout, int Cin, int ks,
                                 int Kpad, hipStream_t s, int f16 = 0);
// bf16 conv (igemm_bf16.hip): A / res / out bf16 NHWC, Wp bf16 [N][Kpad], Kpad % 64 == 0, bias fp32
hipError_t launch_gemm_bf16(const GemmArgs& a, hipStream_t s);
int f32h2_tiles_m(int B, int H, int W, int* tile_pixels = nullptr);            // pixel tiles of the two-fp16-piece conv tile (rows of a planes tensor's exponent table); 0: not eligible
bool gemm_bf16_groupable(const GemmArgs& a);
bool gemm_bf16_upadd_ok(const GemmArgs& a);      // a.up (post-activation upsampled add) can run in igemm_bf16_kernel<.., UPADD>
// bf16 twin of launch_gemm_f32_group; *variant (optional) = the device kernel it chose: 0 ring (igemm_bf16_group_kernel),
// 1 ping-pong (igemm_bf16_group_pp_kernel), 2 ping-pong with row-halo tiles (igemm_bf16_group_rh_kernel), -1 single launch.  (3 is the
// 2-D halo tile's number in the engine's launch log: a launch of launch_gemm_bf16_ws_group, which who routes the convs calls itself)
hipError_t launch_gemm_bf16_group(const GemmArgs* list, int n, hipStream_t s, int* variant = nullptr);
// the path launch_gemm_bf16 takes: the row-halo tile, or one of the four tile shapes of igemm_bf16_kernel; pp: a launch of >= 2048
// tiles (ping-pong schedule, the row-halo tile's condition)
enum class Bf16Path { RH, T128x32, T128x64, T64x64, T128x128 };
struct Bf16Route { Bf16Path path; bool pp; };
Bf16Route gemm_bf16_route(const GemmArgs& a);
const char* gemm_bf16_kernel_name(const GemmArgs& a);
// row-halo variant of the 3x3 / stride-1 bf16 conv (one staged A tile serves the three kw taps): chunk width 64 / 48 / 32 or
// 0 = not eligible; weights packed by launch_pack_conv_bf16_rh ([N][9 * Cin], K order (kh, Cin / CW, kw, CW))
int bf16_rh_width(int Cin);
int gemm_bf16_rh_cw(const GemmArgs& a);
hipError_t launch_gemm_bf16_rh(const GemmArgs& a, hipStream_t s);
hipError_t launch_pack_conv_bf16_rh(const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                                    float eps, void* Wp_bf16, float* bias, int Cout, int Cin, int CW, hipStream_t s, int f16 = 0);
// "2-D halo" tile of the 3x3 / stride-1 bf16 conv (igemm_bf16_ws.hip, igemm_bf16_ws_tile.h): 256 pixels x 32 / 64 / 96 channels per
// block with the accumulators resident for the whole K, 16-channel chunks staged once for all nine taps; weights packed by
// launch_pack_conv_bf16_ws (bf16_ws_pack_elems(Cout, Cin) bf16 elements), passed as GemmArgs::Wp3
// (_ok: what the launcher accepts, Wp3 aside; it refuses every other problem -- an error, never another kernel)
bool gemm_bf16_ws_ok(const GemmArgs& a);
// the size from which the tile pays: 1 GFLOP per conv and batch 24.  The engine's plan applies it (Engine::tile_takes); the launcher runs
// what it is handed
bool bf16_tile_big_enough(int B, int H, int W, int Cin, int Cout);
long bf16_ws_pack_elems(int Cout, int Cin);
hipError_t launch_gemm_bf16_ws_group(const GemmArgs* list, int n, hipStream_t s);
const char* gemm_bf16_ws_kernel_name(const GemmArgs& a);
hipError_t launch_pack_conv_bf16_ws(const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                                    float eps, void* Wp_bf16, float* bias, int Cout, int Cin, hipStream_t s, int f16 = 0);

// fp32 3x3 / stride-1 conv on the bf16 matrix pipe (igemm_f32x3_ws.hip, igemm_f32x3_ws_tile.h): fp32 tensors in and out, every operand split
// losslessly into three bf16 pieces, the six piece products of weight >= 2^-18 accumulated in fp32 -- results to fp32 accumulation
// order.  Any width up to 256, Cin % 16 == 0, Cout % 4 == 0; weights packed by launch_pack_conv_f32x3 (f32x3_pack_elems(Cout, Cin)
// bf16 elements), passed as GemmArgs::Wp3
// (_ok: what the launcher accepts, Wp3 aside -- a test of the geometry, the row maps and whether there is a residual; no pointer is read through)
bool gemm_f32x3_ok(const GemmArgs& a);
// the size from which either split-fp32 tile pays: 370 MFLOP per conv and batch 5.  The engine's plan applies it (Engine::tile_takes); the
// launchers run what they are handed
bool f32_tile_big_enough(int B, int H, int W, int Cin, int Cout);
long f32x3_pack_elems(int Cout, int Cin);
hipError_t launch_gemm_f32x3_group(const GemmArgs* list, int n, hipStream_t s);
const char* gemm_f32x3_kernel_name();
hipError_t launch_pack_conv_f32x3(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                                  void* Wp_bf16, float* bias, int Cout, int Cin, hipStream_t s);
// the same convs with HALF the MFMAs (igemm_f32h2_ws.hip, igemm_f32h2_ws_tile.h): every operand as two fp16 pieces under an exact power-of-two
// block scale (per output channel for the weights, per block and 16-channel chunk for the pixels, found in the kernel), three piece products
// per fp32 MAC, fp32 accumulation; operands to 2^-23, one product to 2^-21 -- below the fp32 accumulation error of the dot product it
// belongs to.  The plan's default tile (Engine::plan.x3_h2); tensors of any size (it addresses from per-tile bases).  Weights packed by
// launch_pack_conv_f32h2 (f32h2_pack_elems(Cout, Cin) 16-bit elements), passed as GemmArgs::Wp3 with GemmArgs::x3_h2 set
long f32h2_pack_elems(int Cout, int Cin);
hipError_t launch_gemm_f32h2_group(const GemmArgs* list, int n, hipStream_t s);
bool gemm_f32h2_ok(const GemmArgs& a);
static constexpr int F32H2_UNIT_TABLE_WORDS = 7 * 256;
bool f32h2_unit_table(int H, int W, int Cin, unsigned* out);     // the tile's unit table of a map geometry (igemm_f32h2_ws_tile.h); false: none, the kernel computes
const char* gemm_f32h2_kernel_name();
hipError_t launch_pack_conv_f32h2(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                                  void* Wp_f16, float* bias, int Cout, int Cin, hipStream_t s);
// ... and everything else that is fp32 and MFMA-shaped -- 1x1 / stride-2 / lone convs, the lifter's linears -- on the same two-piece arithmetic
// (igemm_f32h2.hip): the A tile is staged as fp32 exactly as igemm_f32.hip stages it and split by the wave that consumes it (scale per wave,
// 32 rows and 32-deep chunk); weights packed by launch_pack_f32h2_gemm over the fp32 pack's geometry (GemmArgs::Wh2)
long f32h2_gemm_pack_elems(int N, int Kpad);            // floats
// the power-of-two channel scales of both two-piece packs: winv[n] = 1 / t with max_k |w[n][k] * bn_scale| t in [2^14, 2^15) for the rows
// n < N of w [N][K], 1 for the rows N <= n < rows (one launch, one block per row)
hipError_t launch_f32h2_wscale(const float* w, const float* gamma, const float* var, float eps, float* winv, int rows, int N, int K, hipStream_t s);
bool gemm_f32h2g_ok(const GemmArgs& a);
hipError_t launch_gemm_f32h2g(const GemmArgs& a, hipStream_t s);
hipError_t launch_gemm_f32h2g_group(const GemmArgs* list, int n, hipStream_t s);     // convs with plain row maps, one grid
const char* gemm_f32h2g_kernel_name(const GemmArgs& a, bool grouped);
hipError_t launch_pack_f32h2_gemm(const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                                  float* Wp, float* bias, int N, int Cin, int ks, int K, int Kpad, hipStream_t s);   // ks = 0: linear [N][K]
// rows [n0, n0 + n) of an [Ntot][Kpad] pack from one nn.Linear weight [n][K] (several linears concatenated along N share a pack)
hipError_t launch_pack_f32h2_gemm_rows(const float* w, float* Wp, int n0, int n, int Ntot, int K, int Kpad, hipStream_t s);
// One matrix of the training step's weight table: W [N][K] (row pitch ld) -> its two-piece pack at base + fwd_off (Kpad = K rounded up to 32)
// and the pack of W^T [K][N] at base + bwd_off (Kpad = N rounded up to 32); either offset may be -1 (not wanted).  tile_start: first block of
// this matrix in the launch (ceil(N / 32) * ceil(K / 32) blocks each); max_off: its N row + K column maxima in the scratch
struct H2TrainW {
    const float* w;
    long fwd_off, bwd_off;
    int N, K, ld, tile_start, max_off, pad_;
};
hipError_t launch_pack_f32h2_train(const H2TrainW* tab_dev, int n, int tiles, float* base, int* maxima, long maxima_elems, hipStream_t s);
// The small-Cin stem conv (igemm_stem.hip; what gemm_f32_route calls F32Path::STEM: a conv with Cin % 4 != 0, and capf_op_conv_16's
// Cin % 8 != 0 branch): fp32 image and fp32 pack in, fp32 or -- out_bf16 -- 16-bit result.  One decision, a function of the problem alone:
// the 16-bit kernels where they take the problem (element-wise gather / one run per (pixel, kh) / the persistent streaming form of that),
// else the fp32 ones (streaming / element-wise gather).  ks: 7 / 3 for the run-based kernels
enum class StemKernel { F32_SMALLC, F32_STREAM, B16_SMALLC, B16_RUNS, B16_STREAM };
inline bool stem_is_16bit(StemKernel k) { return k >= StemKernel::B16_SMALLC; }
struct StemRoute { StemKernel kernel; int ks; };
StemRoute gemm_stem_route(const GemmArgs& a);
// in == nullptr: the fp32 image at GemmArgs::A.  Otherwise the uint8 BGR crop itself (pixel_rule.h U8Input; GemmArgs::A is not read): the same
// route, the same grid, the U8 form of the same kernel -- bit-identical to the float form on launch_preprocess's output; its name is the float
// kernel's with a ",u8" tag
bool gemm_stem_ok(const GemmArgs& a, const U8Input* in);
hipError_t launch_gemm_stem(const GemmArgs& a, const U8Input* in, hipStream_t s);
const char* gemm_stem_kernel_name(const GemmArgs& a, bool u8);
hipError_t launch_pack_linear(const float* w, float* Wp, int N, int K, int Kpad, hipStream_t s);
// quad-interleaved pack for the fused lifter kernels: Wq[(k / 4) * Ntot + n0 + n][k % 4] = w[n][k]  (K % 4 == 0): lane n of a
// wave reads the 16-byte quad next to lane n - 1's instead of a row K floats away
hipError_t launch_pack_linear_quad(const float* w, float* Wq, int N, int K, int n0, int Ntot, hipStream_t s);
// lifter projections on the bf16 MFMA path (igemm_bf16.hip): A bf16 [M][K], W bf16 [N][Kpad]; gelu_bf16_out = 0: fp32 out
// (+ fp32 residual) through the row maps; 1: GELU then bf16 out [M][N]
hipError_t launch_gemm_bf16_rows(const void* A_bf16, const void* W_bf16, const float* bias, int M, int N, int K, int Kpad,
                                 float* out, RowMap omap, const float* res, RowMap rmap, int gelu_bf16_out, hipStream_t s, int f16 = 0);
const char* gemm_bf16_rows_kernel_name(int M, int N, int f16 = 0);

// out = relu( sum_i up_{s_i}(in_i) ), NHWC, s_i = nearest-upsample factor (1 = same resolution)
struct FuseSumArgs {
    const float* in[4];
    int shift[4];  // log2 of the upsample factor
    int n_in;
    int f16;       // 16-bit tensors (bf16 below): their element format, 0 bf16 / 1 fp16
    float* out;
    int B, H, W, C;
    int relu;
    int bf16;      // tensors are 16-bit (arithmetic stays fp32)
    void* out_sh;  // fp32 sums only (bf16 = 0): bf16 shadow of out (RNE, [B,H,W,C]) written in the same pass, or nullptr
};
hipError_t launch_fuse_sum(const FuseSumArgs& a, hipStream_t s);
// up to 4 independent sums (the outputs of one HRNet fuse module) as ONE launch; same arithmetic per element as launch_fuse_sum
hipError_t launch_fuse_sum_group(const FuseSumArgs* a, int n, hipStream_t s);

// Training-mode BatchNorm2d of a raw conv output x [rows = B * H * W][C] fp32 (bn_train.hip): batch statistics without atomics -- slab
// partials (fp64 mean / M2 per slab and channel, bn_scratch_elems floats at `part`, 8-byte aligned), combined by a second launch in one fixed
// order -- into scale = gamma / sqrt(var + eps), shift = beta - mean * scale and the running statistics (updated in place; nullptr: none);
// then y = act(x * scale[c] + shift[c] + res).  C % 4 == 0, C <= 1024, rows >= 2 for the statistics.  The launchers fill slab_rows / nslab
static constexpr int BN_MAX_SLABS = 1024;
struct BnStatsArgs {
    const float* x;
    const float *gamma, *beta;
    float *rmean, *rvar;
    double* part;
    float *scale, *shift;
    long rows;
    int C, slab_rows, nslab;
    float eps, momentum;
};
struct BnApplyArgs {
    const float* x;
    const float* res;      // [rows][C] or nullptr
    float* y;              // may be x
    const float *scale, *shift;
    long rows;
    int C, act;            // act: 0 none, 1 ReLU (relu_f)
};
int bn_slab_rows(long rows, int C);
int bn_num_slabs(long rows, int C);
size_t bn_scratch_elems(long rows, int C);     // 0: a shape the kernels do not take
// up to 4 independent BatchNorms (the branches of an HRNet level) per launch: statistics = two launches, apply = one
hipError_t launch_bn_stats_group(const BnStatsArgs* a, int n, hipStream_t s);
hipError_t launch_bn_apply_group(const BnApplyArgs* a, int n, hipStream_t s);

// 3x3 s2 p1 max-pool NHWC (resnet.py:140), bilinear align_corners=True resize NHWC (+ optional add)
hipError_t launch_maxpool3x3s2(const float* in, float* out, int B, int H, int W, int C, int Ho, int Wo,
                               hipStream_t s, int bf16 = 0, int f16 = 0);      // bf16: 16-bit tensors, of format f16 (0 bf16, 1 fp16)
hipError_t launch_bilinear_resize(const float* in, float* out, int B, int H, int W, int C, int Ho, int Wo,
                                  hipStream_t s, int bf16 = 0, const float* add = nullptr, int f16 = 0);   // out = resize(in) (+ add, same shape as out)

// n small float copies in one launch; the table ({src, dst, n} per segment) is in device memory
struct CopySegment {
    const float* src;
    float* dst;
    int n, pad;
};
hipError_t launch_copy_segments(const CopySegment* table_dev, int n, hipStream_t s);

// ---- lifter -----------------------------------------------------------------------------------
// kcrop -> ref in place (conpose.py:34-35);  X[b,p,0,:] = coord_embed(k2d[b,p]) + pos[0,p,:]
hipError_t launch_prep_embed(float* kcrop, const float* k2d, const float* w, const float* bias,
                             const float* pos, float* X, int B, int J, int L1, int C, hipStream_t s);
// reference-point sampling, padding zeros (pose_dformer.py:216-218): S[b,p,:] = bilinear(feat, ref[b,p])
hipError_t launch_sample_ref(const float* feat, const float* ref, float* S, int* idx, int B, int J, int H,
                             int W, int C, hipStream_t s, int feat_bf16 = 0);
// LayerNorm over rows: out[r,:] = LN(in[imap(r)] (+ add[amap(r)]))   width C
hipError_t launch_layernorm(const float* in, RowMap imap, const float* add, RowMap amap, const float* g,
                            const float* b, float eps, float* out, int rows, int C, hipStream_t s, int out_bf16 = 0);   // out_bf16: 16-bit rows out, 1 bf16 / 2 fp16
// deformable sampling (pose_dformer.py:122-135 minus the embed_proj GEMM):
//   AO [rows=(b,p,l), NH*NS + 2*NH*NS] = [attention logits | offset pre-activations]
//   U_l[(b,p,h), :] = sum_s softmax_s(logit[h,s]) * bilinear_border(feat_l, tanh(off[h,s]) + ref[b,p])
struct DeformArgs {
    const float* feat[4];
    int H[4], W[4], C[4];
    float* U[4];
    const float* AO;
    const float* ref;
    int B, J, L, NH, NS;
    int feat_bf16;           // storage format of the context maps: 0 fp32, 1 bf16, 2 fp16 (the same code in launch_sample_ref / EmbedArgs / CtxAttnArgs)
    int ld_ao;               // row pitch of AO (0 = 3*NH*NS, the inference layout; 64 in training)
    const float* dU[4];      // backward only: gradient w.r.t. U[l]
    float* cpos;             // optional taps (capf_set_debug): sampling positions pos = tanh(off) + ref, [B*J, L, NH*NS, 2] ...
    int* cidx;               // ... and the NW corner (x0, y0) of each, border mode (bit-exact check against the oracle)
};
hipError_t launch_deform_sample(const DeformArgs& a, hipStream_t s);
// the corner arithmetic of both sampling sites on caller-supplied coordinates (op-level parity test): grid [n, 2] normalised
// (x, y) -> idx [n, 2] = (x0, y0), frac [n, 2] = (wx1, wy1); border = 1: padding_mode='border' (pose_dformer.py:128), 0: zeros (:217)
hipError_t launch_bilinear_corners(const float* grid, int n, int H, int W, int border, int* idx, float* frac, hipStream_t s);
// ---- fused front half of the lifter (lifter_fused.hip) -----------------------------------------------------------
// crop-keypoint normalisation (in place) + coord_embed + reference-point sampling (padding zeros) + feat_embed + pos
struct EmbedArgs {
    float* kcrop;                // [BJ, 2] in: crop pixels, out: ref
    const float* k2d;            // [BJ, 2]
    const float* cw; const float* cb;       // coord_embed weight [C, 2], bias [C]
    const float* pos;            // Spatial_pos_embed [1, L1, J, C]
    const float* feat[4]; int H[4], W[4], Cl[4];
    const float* fw[4]; const float* fb[4]; // feat_embed[l] weight [C, Cl], bias [C]
    float* sampled[4];           // optional taps: sampled rows [BJ, Cl]
    int* idx[4];                 // optional taps: NW corner (x0, y0) per (b, p)
    float* X;                    // tokens [B, J, L1, C]
    int BJ, J, L, L1, C;
    int feat_bf16;
};
hipError_t launch_embed(const EmbedArgs& a, hipStream_t s);
// DeformableBlock attention half (LayerNorm + logits / offsets + sampling + embed_proj + residual), see lifter_fused.hip
struct CtxAttnArgs {
    const float* feat[4]; int H[4], W[4], Cl[4];
    const float* Wp[4]; const float* bp[4]; // embed_proj[l] weight [C/NH, Cl], bias [C/NH]
    const float* Wao; const float* bao;     // [attention_weights | sampling_offsets] quad-interleaved: Wq[C / 4][3*NH*NS][4]; bias
    int ldw;
    const float* ln_g; const float* ln_b; float eps;
    const float* ref;            // [BJ, 2]
    float* X;                    // tokens [B, J, L1, C], updated in place (tokens 1..L)
    int BJ, J, L, L1, C, NH, NS;
    int feat_bf16;
    int woff[4];                 // per-wave LDS section offsets (floats), filled by the launcher
    float* cpos;                 // optional taps (capf_set_debug): sampling positions [BJ, L, NH*NS, 2] and their NW corners
    int* cidx;
    float* U[4];                 // optional: per level [BJ * NH][Cl] scratch -- the per-head weighted sample sums leave the kernel and embed_proj +
                                 // residual run as ONE fp32-MFMA launch over all levels behind it (ctx_proj_kernel); null: inside the kernel
};
hipError_t launch_ctx_attn(const CtxAttnArgs& a, hipStream_t s);
// tiny multi-head attention: QKV [G*N, 3*heads*d] -> O [G*N, heads*d]; N tokens per group
hipError_t launch_attention(const float* qkv, float* out, int groups, int N, int heads, int d, hipStream_t s, int out_bf16 = 0);
// the token counts and head dimensions launch_attention takes: 1 <= N <= ATTENTION_MAX_TOKENS, d a positive multiple of 4
static constexpr int ATTENTION_MAX_TOKENS = 17;
bool attention_ok(int N, int d);
// head (pose_dformer.py:240): out[r, 0..2] = Linear(LN(X[r,:]))
hipError_t launch_head(const float* X, const float* g, const float* b, float eps, const float* w,
                       const float* wb, float* out, int rows, int C, int NO, hipStream_t s);

// ---- training step (train_kernels.hip) ----------------------------------------------------------------
hipError_t launch_layernorm_train(const float* in, RowMap imap, const float* add, RowMap amap, const float* g,
                                  const float* b, float eps, float* out, float* xhat, float* rstd, int rows, int C,
                                  hipStream_t s);
hipError_t launch_layernorm_bwd(const float* dy, const float* xhat, const float* rstd, const float* gamma, float* dX,
                                RowMap omap, float* second, RowMap smap, int rows, int GRP, int C, hipStream_t s);
// dst[c*dst_stride] (+)= sum_r A[amap(r)+c] * B(r,c); bmode 0 none, 1 B[bmap(r)+c], 2 B[bmap(r)]; scratch >= 64*C floats
// `defer` (optional): the second stage is NOT launched but appended to the batch (launch_colreduce_final_batch runs every waiting one in a
// single launch; the scratch must stay untouched until then)
static constexpr int COL_BATCH_MAX = 40;
struct ColFinalBatch {
    const float* partial[COL_BATCH_MAX];
    const float* partial2[COL_BATCH_MAX];
    float* dst[COL_BATCH_MAX];
    float* dst2[COL_BATCH_MAX];
    int chunks[COL_BATCH_MAX], C[COL_BATCH_MAX], dst_stride[COL_BATCH_MAX];
    int blk_end[COL_BATCH_MAX];       // running block count (64 columns per block)
    int count;
};
int colreduce_chunks(int rows, int C, int nout, size_t scratch_elems, int* rows_per_chunk = nullptr);   // row chunks of the first stage: scratch = nout * chunks * C floats
hipError_t launch_colreduce(const float* A, RowMap amap, const float* Bm, RowMap bmap, int bmode, int rows, int C,
                            float* dst, long dst_stride, int accumulate, float* scratch, hipStream_t s,
                            float* dst2 = nullptr, size_t scratch_elems = 0, ColFinalBatch* defer = nullptr);   // dst2: plain column sums of A as well
hipError_t launch_colreduce_final_batch(const ColFinalBatch& b, hipStream_t s);
hipError_t launch_slab_sum(const float* slabs, int nslab, long n, float* dst, hipStream_t s);
// the same sums for up to SLAB_BATCH_MAX weight gradients in ONE launch (the backward defers them: Engine::t_slab_flush).  Every job: n % 4 == 0,
// 16-byte aligned slabs; slabs summed in order k = 0, 1, ... per element exactly as slab_sum_kernel does (same bits)
static constexpr int SLAB_BATCH_MAX = 48;
struct SlabBatch {
    const float* src[SLAB_BATCH_MAX];
    float* dst[SLAB_BATCH_MAX];
    int n[SLAB_BATCH_MAX];            // elements per slab
    int nslab[SLAB_BATCH_MAX];
    int blk_end[SLAB_BATCH_MAX];      // running block count: job j owns blocks [blk_end[j - 1], blk_end[j]), 1024 elements each
    int count;
};
hipError_t launch_slab_sum_batch(const SlabBatch& b, hipStream_t s);
// dW[n][k] = sum_m dY[m][n] X[m][k] (+ db[n] = sum_m dY[m][n] behind it) from row-major operands, no transposes (train_kernels.hip);
// N % 4 == 0, K % 4 == 0; slice s of `splits` row ranges writes N * K (+ N) floats at out + s * slab.  h2: both operands as two fp16
// pieces split in the kernel, three piece products on the 16-bit matrix pipe, 128 x 128 tiles (N % 128 == 0, K % 128 == 0)
hipError_t launch_wgrad_tn(const float* dY, long ldy, const float* X, long ldx, int M, int N, int K, float* out, long slab, int splits,
                           int want_bias, hipStream_t s, bool h2 = false);
hipError_t launch_gelu_fwd(const float* x, float* y, long n, hipStream_t s);
hipError_t launch_gelu_bwd(const float* x, const float* dy, float* dx, long n, hipStream_t s);
hipError_t launch_transpose_pad(const float* in, RowMap imap, int M, int C, float* out, int Mp, hipStream_t s);
hipError_t launch_attention_bwd(const float* qkv, const float* dO, float* dqkv, int groups, int N, int heads, int d,
                                hipStream_t s);
// what launch_attention_bwd takes: attention_ok(N, d) and its instance's dynamic LDS (attention_bwd_lds_bytes: q, k, v, dO [NMAX][d + 1]
// and P, dS [NMAX][NMAX + 1] floats, NMAX = 5 up to 5 tokens, else 17) within ATTENTION_BWD_MAX_LDS
static constexpr size_t ATTENTION_BWD_MAX_LDS = 64 * 1024;
size_t attention_bwd_lds_bytes(int N, int d);
bool attention_bwd_ok(int N, int d);
// dref (optional, capf_backward_points; fp32 maps only): [B*J, 2], the block's position gradients are added to it -- the kernel's PTS form
hipError_t launch_deform_bwd(const DeformArgs& a, float* dAO, int ldd, hipStream_t s, float* dref = nullptr);
// ---- gradient w.r.t. the keypoints (capf_backward_points).  dref [B*J, 2] is dL/d(normalised crop keypoints): zeroed by the caller, then
//     dref = ((((0 + c[Lv-1]) + c[Lv-2]) + ...) + c[0]) + r_ref
// with c[i] added by context block i's launch_deform_bwd (the order Engine::backward visits them) and r_ref by launch_points_grad: every
// term a fixed fp32 expression (train_kernels.hip), every add a plain load and store by the one block that owns (b, p).  Bit-reproducible.
struct PointsGradArgs {
    const float* feat[4];    // fp32 NHWC context maps
    int H[4], W[4], C[4];
    const float* dS[4];      // input gradient of feat_embed[l], [B*J, C_l]
    const float* ref;        // [B*J, 2] normalised crop keypoints
    const float* dX;         // token gradient; row (b, p) at dX + (b * J + p) * ldx, token 0 = its first Ce floats
    long ldx;
    const float* cw;         // coord_embed.weight [Ce, 2]
    int Ce;
    float* dref;             // [B*J, 2] or null: dref += r_ref
    float* dk2d;             // [B*J, 2] or null: dk2d = dX[:, 0, :] coord_embed.weight
    int B, J, L;
};
hipError_t launch_points_grad(const PointsGradArgs& a, hipStream_t s);
// ---- gradient w.r.t. the context maps (capf_backward_maps): the backward of both bilinear samplers w.r.t. the SAMPLED tensor.  g[l] holds
// the gradient of every sampled vector; each is added to its (up to) four corners of dfeat[l] (fp32 NHWC [B, H, W, C], zeroed first by
// launch_zero_maps), lanes over contiguous channels.  Two summation forms of the same sources into the same destinations:
//   atomic  (launch_deform_scatter / launch_ref_scatter): fp32 atomic adds; the order of the adds is not fixed: dfeat is not bit-reproducible
//   ordered (launch_deform_scatter_ordered / launch_ref_scatter_ordered): no atomics, a fixed expression -- see below
struct MapGradArgs {
    float* dfeat[4];
    const float* g[4];       // deform: dU[l] [(b,p,h), C_l];  ref: dS_l [(b,p), C_l]
    int H[4], W[4], C[4];
    const float* AO;         // deform only: [attention logits | offset pre-activations] of the block, rows (b,p,l), pitch ld_ao
    const float* ref;        // [B*J, 2] normalised crop keypoints
    int B, J, L, NH, NS, ld_ao;
};
// pose_dformer.py:128 (padding border): dfeat[corner of sample s of head h] += softmax_s(logit[h,s]) * bilinear weight * dU[(b,p,h)]
hipError_t launch_deform_scatter(const MapGradArgs& a, hipStream_t s);
// pose_dformer.py:217 (padding zeros): dfeat[corner of ref[b,p]] += bilinear weight * dS[(b,p)], corners outside the map dropped
hipError_t launch_ref_scatter(const MapGradArgs& a, hipStream_t s);
// The ordered form.  An ITEM is one corner of one sample: it = ((p * NH + h) * NS + s) * 4 + dy * 2 + dx (deformable, source row dU[(b,p,h)],
// weight softmax_s * wx * wy) or it = p * 4 + dy * 2 + dx (reference point, source row dS[(b,p)], weight wx * wy); cells, weights and the
// inside test are the atomic form's, from one device function.  One launch adds, to every pixel that any of its items falls into,
//     S[pixel][c] = sum over that pixel's items, IN ASCENDING it, in fp32 without contraction, of weight_it * row_it[c]
// by a plain load and a plain store: dfeat[pixel][c] = dfeat[pixel][c] + S[pixel][c].  Inside a launch every pixel has exactly one owner
// (a workgroup owns a frame, a level and 64 channels; it sorts the frame's (pixel, it) keys in LDS), so with the stream-ordered launches
// of Engine::backward the whole gradient is ONE fixed expression,
//     dfeat = ((((0 + S_ctx[Lv-1]) + S_ctx[Lv-2]) + ...) + S_ctx[0]) + S_ref,
// bit-identical from run to run; pixels that no item falls into keep launch_zero_maps' 0.  No global scratch.
// Limits: launch_deform_scatter's (NS == 4, NH * NS <= 16, L <= 4, C_l % 4 == 0), J * NH * NS * 4 <= MAPGRAD_ORDERED_MAX_ITEMS items per
// (frame, level) in the deformable pass (J <= 32 at NH * NS = 16) and J <= MAPGRAD_ORDERED_MAX_JOINTS in the reference pass,
// H_l * W_l <= 2^20, dfeat 16-byte aligned; anything else: hipErrorInvalidValue.
constexpr int MAPGRAD_ORDERED_MAX_ITEMS = 2048;
constexpr int MAPGRAD_ORDERED_MAX_JOINTS = 64;
hipError_t launch_deform_scatter_ordered(const MapGradArgs& a, hipStream_t s);
hipError_t launch_ref_scatter_ordered(const MapGradArgs& a, hipStream_t s);
// p[l][0 .. n[l]) = 0 for `count` <= 4 maps in one launch (n[l] % 4 == 0, 16-byte aligned pointers; the launcher fills blk_end)
struct ZeroMaps {
    float* p[4];
    long n[4];
    int blk_end[4];          // running block count: map l owns blocks [blk_end[l - 1], blk_end[l]), 4096 elements each
    int count;
};
hipError_t launch_zero_maps(ZeroMaps z, hipStream_t s);
hipError_t launch_mpjpe(const float* pred, const float* gt, int rows, float* loss, float* dpred, float gscale,
                        hipStream_t s);
hipError_t launch_mpjpe_nd(const float* pred, const float* gt, int rows, int D, float* loss, float* dpred, float gscale,
                           hipStream_t s);
hipError_t launch_adamw(float* p, const float* g, float* m, float* v, long n, float lr, float b1, float b2, float eps,
                        float wd, int step, hipStream_t s, float gscale = 1.0f);
// guarded AdamW (train.py:194-201, run_3dhp.py:260-277): launch_grad_sumsq leaves OPTIM_PARTIALS block sums of (gscale * g[i])^2 (fp64) and
// non-finite flags in the control block; launch_adamw_guarded adds them in a fixed order in every block, clips by the global norm, skips
// the whole update when the gradient is not finite, and otherwise runs launch_adamw's arithmetic with lr / weight decay per segment and
// the bias corrections of the DEVICE's step count (slot[attempt & 1] is written, slot[~attempt & 1] read: no word is read and written
// within one launch).  The report comes first so that a caller copies sizeof(capf_optim_report) bytes from the block's start.
constexpr int OPTIM_PARTIALS = 512;          // fixed: the grid of launch_grad_sumsq, whatever the device
constexpr int ADAMW_MAX_SEGMENTS = 64;
struct OptimCtrl {
    capf_optim_report report;
    capf_optim_report slot[2];
    double partial[OPTIM_PARTIALS];
    unsigned nonfinite[OPTIM_PARTIALS];
};
struct AdamwSegments {                       // sorted, disjoint, covering [0, n): segment k is [end[k - 1], end[k]) (end[-1] = 0)
    long end[ADAMW_MAX_SEGMENTS];
    float lr[ADAMW_MAX_SEGMENTS], wd[ADAMW_MAX_SEGMENTS];
    int count;
};
hipError_t launch_optim_ctrl_init(OptimCtrl* ctrl, long long steps_taken, hipStream_t s);
hipError_t launch_grad_sumsq(const float* g, long n, float gscale, OptimCtrl* ctrl, hipStream_t s);
hipError_t launch_adamw_guarded(float* p, const float* g, float* m, float* v, long n, const AdamwSegments& segs, float b1, float b2,
                                float eps, float gscale, float max_norm, long long attempt, const float* loss, int rows,
                                OptimCtrl* ctrl, hipStream_t s);
// dst[r, :] = src[smap(r), :] * scale[r / div]   (DropPath mask on a gradient), width C
hipError_t launch_scale_rows(const float* src, RowMap smap, const float* scale, int div, float* dst, int rows, int C,
                             hipStream_t s);
// head backward pieces: dY[r, c] = sum_o dOut[r, o] * W[o, c]  (NO <= 4)
hipError_t launch_head_dgrad(const float* dOut, const float* W, float* dY, int rows, int C, int NO, hipStream_t s);
// dpos[l, p, c] = sum_b dX[b, p, l, c]
hipError_t launch_pos_grad(const float* dX, float* dpos, int B, int J, int L1, int C, hipStream_t s);

// ---- neighbours of the path (preprocess.hip): N1 input preprocessing, N2 flip-test fusion ---------------
// mode 0: as is; 1: train-time horizontal flip of the whole batch; 2: flip-test (outputs hold [orig | mirrored])
hipError_t launch_preprocess(const unsigned char* images_bgr, int B, int H, int W, const float mean[3], const float* stdv,
                             int mode, float* images_out, const float* gt_in, float* gt_out, const float* k2d_in,
                             float* k2d_out, const float* kc_in, float* kc_out, hipStream_t s);
// ... its keypoint / ground-truth half alone (one launch; what launch_preprocess runs behind the image kernel)
hipError_t launch_preprocess_points(int B, int mode, const float* gt_in, float* gt_out, const float* k2d_in, float* k2d_out,
                                    const float* kc_in, float* kc_out, hipStream_t s);
hipError_t launch_fliptest_fuse(const float* pred2, int B, float* out, hipStream_t s);     // the H36M table (kSwap)
// A mirror's joint exchange for any skeleton of J <= MAX_JOINTS joints: swap[j] = the joint of the mirror that lands on joint j.  The table
// travels in the kernel arguments (no per-call device allocation).  It is a permutation that is its own inverse (left <-> right pairs, the
// rest fixed) -- the ONE statement of that rule: the C ABI entries that take a table judge it with this, and the three launchers that put a
// table into kernel arguments call it again before a kernel indexes by it.
constexpr int MAX_JOINTS = 32;
struct SwapTable { int j[MAX_JOINTS]; };
inline bool swap_table_ok(const int* swap, int J) {
    if (!swap || J < 1 || J > MAX_JOINTS) return false;
    for (int j = 0; j < J; ++j)
        if (swap[j] < 0 || swap[j] >= J || swap[swap[j]] != j) return false;
    return true;
}
hipError_t launch_fliptest_fuse_swap(const float* pred2, int B, int J, const int* swap, float* out, hipStream_t s);
// N3 (preprocess.hip): get_affine_transform (host) and cv2.warpAffine INTER_LINEAR for 8-bit BGR frames
bool affine_from_center_scale(const double center[2], const double scale[2], int out_w, int out_h, double M[6]);
hipError_t launch_warp_affine_u8(const unsigned char* const* frames, const int* dims, const double* M, unsigned char* out,
                                 int B, int out_h, int out_w, hipStream_t s);
// N1 (erase.hip): erase_image (mvn/utils/img.py:179-198) for a batch of uint8 crops -- P <= MAX_JOINTS patches a frame, a frame of at most
// 2^31 - 1 bytes, scratch = ERASE_PATCH_BYTES per (frame, patch), 16-byte aligned; out == images or disjoint from it
constexpr int ERASE_PATCH_BYTES = 32;
hipError_t launch_erase_patches(const unsigned char* images, int B, int H, int W, const float* centers, const unsigned char* mask, int P,
                                int size, int use_mean, unsigned char* out, void* scratch, hipStream_t s);

// ---- evaluation metrics (metrics.hip): N2 -------------------------------------------------------------------
hipError_t launch_pose_errors(const float* pred, const float* gt, int n, int J, const int* prev, float* err, hipStream_t s);
hipError_t launch_segment_sums(const float* err, const int* seg, const int* prev, int n, int n_seg, double* sums, int* counts,
                               hipStream_t s);
// MPI-INF-3DHP PCK / AUC / MPJPE counts: counts [n_seg][J][PCK_THRESHOLDS] int32, sums [n_seg][J] fp64, frames [n_seg] int32
constexpr int PCK_THRESHOLDS = 31;
hipError_t launch_pck_counts(const float* pred, const float* gt, int n, int J, int root, double to_mm, const int* seg, int n_seg,
                             int* counts, double* sums, int* frames, hipStream_t s);
// 2-D PCKh counts: counts [n_seg][K][J] int32, valid [n_seg][J] int32, sums [n_seg][J] fp64; thresholds: K host doubles, carried to the
// kernel in its arguments
constexpr int PCK2D_MAX_THRESHOLDS = 32;
struct Pck2dThresholds { double v[PCK2D_MAX_THRESHOLDS]; };
hipError_t launch_pck2d_counts(const float* pred, const float* gt, int n, int J, const float* norm, const float* weight,
                               const double* thresholds, int K, int strict, const int* seg, int n_seg, int* counts, int* valid, double* sums,
                               hipStream_t s);
hipError_t launch_keypoints_loss(const float* pred, const float* gt, const float* validity, int rows, int D, int mode, float thr,
                                 float* loss, float* dpred, hipStream_t s);
// ---- the remaining pose losses of ContextPose/mvn/models/loss.py (pose_losses.hip) ---------------------------------------------------
// KeypointsL2Loss (loss.py:140-147): one block; dpred (or nullptr) = gscale * dloss/dpred, exactly 0 where the row's square root is 0
hipError_t launch_keypoints_l2_loss(const float* pred, const float* gt, const float* validity, int rows, int D, float* loss, float* dpred,
                                    float gscale, hipStream_t s);
// LimbLengthError (loss.py:181-201): err [n][L] fp32 per pose and limb; dpred (or nullptr) [n][J][3] = gscale * d(sum_l err[i][l])/dpred.
// The limb table (L <= LIMB_MAX pairs of joints in [0, J), checked by the caller) travels in the kernel's arguments.
constexpr int LIMB_MAX = 64;
struct LimbTable { unsigned char a[LIMB_MAX], b[LIMB_MAX]; };
hipError_t launch_limb_length_errors(const float* pred, const float* gt, int n, int J, const LimbTable& limbs, int L, float* err, float* dpred,
                                     float gscale, hipStream_t s);
// sums [n_seg][L] fp64 in a fixed order, counts [n_seg] int64
hipError_t launch_limb_length_sums(const float* err, const int* seg, int n, int L, int n_seg, double* sums, long long* counts, hipStream_t s);
// UNCERTAINTY (loss.py:7-13): K <= UNCERTAINTY_MAX_SIGMAS sigma tensors of width D or 1; one block
constexpr int UNCERTAINTY_MAX_SIGMAS = 8;
struct UncertaintySigmas {
    const float* sigma[UNCERTAINTY_MAX_SIGMAS];
    float* dsigma[UNCERTAINTY_MAX_SIGMAS];           // nullptr: not wanted
    int width[UNCERTAINTY_MAX_SIGMAS];               // D or 1
};
hipError_t launch_uncertainty_loss(const float* pred, const float* gt, int rows, int D, const UncertaintySigmas& sg, int K, float* loss,
                                   float* dpred, float gscale, hipStream_t s);

// ---- 2-D keypoint head (kp_head.hip): final_layer (1x1 conv) on feat0 + heatmap decode, one pass over the map ------------------------
constexpr int KP_MAX_CHANNELS = 512;
constexpr int KP_MAX_SLABS = 64;             // forward: slabs of 256-pixel tiles per frame (a function of H * W alone)
constexpr int KP_BW_SLABS = 8;               // backward: blocks per frame, each leaves one partial of dW
// the ONE statement of the shapes the head takes (kp_geom, and the C ABI entries through engine.cpp's kp_shape_check)
inline bool kp_shape_ok(int B, int H, int W, int C, int J) {
    return B >= 1 && H >= 1 && W >= 1 && J >= 1 && J <= MAX_JOINTS && C >= 4 && C % 4 == 0 && C <= KP_MAX_CHANNELS;
}
struct KpGeom {                              // kp_geom: how a shape is cut; ok = false: a shape the kernels do not take
    int ntiles, slab_tiles, nslab, bw_tiles, nbw;
    size_t fwd_elems, stat_elems, bw_elems;  // floats of scratch: slab records | (max, sum, x, y) per (frame, joint) | dW partials
    bool ok;
};
KpGeom kp_geom(int B, int H, int W, int C, int J);
struct KpHeadArgs {
    const void* x;           // [B, H, W, C] NHWC, dtype 0 fp32 / 1 bf16 / 2 fp16 (capf_dtype)
    int dtype;
    const float* wt;         // [J, C]
    const float* bias;       // [J] or NULL
    const float* to_image;   // [B, 2, 3] or NULL
    float* kcrop;            // [B, J, 2]
    float* k2d;              // [B, J, 2] or NULL
    float* score;            // [B, J] or NULL
    float* heat;             // [B, J, H, W] or NULL
    float* part;             // scratch (fwd_elems floats; the backward: + stat_elems + bw_elems)
    int B, H, W, C, J, mode; // mode 0 argmax, 1 integral
    float beta;
    float dec[4];            // sx, ox, sy, oy
    // backward (mode 1, fp32 map)
    const float* dkcrop;     // [B, J, 2] or NULL
    const float* dk2d;       // [B, J, 2] or NULL (needs to_image)
    float* dW;               // [J, C]
    float* dbias;            // [J] or NULL: zeros
    float* dmap;             // [B, H, W, C] or NULL
    int accumulate;
    // filled by the launchers
    KpGeom g;
    float* stats;
    float* bw_part;
};
hipError_t launch_kp_head_forward(KpHeadArgs a, hipStream_t s);
hipError_t launch_kp_head_backward(KpHeadArgs a, hipStream_t s);
// the flip-test pair (capf_kp_head_forward_pair): x holds [2 B, H, W, C], frame B + b the mirror of source frame b; B counts SOURCE frames
// (grids, scratch and to_image [B, 2, 3] are the single entry's at B); kcrop / k2d are the stacks [2, B, J, 2], score [B, J], heat
// [B, J, H, W] the fused logits.  Forward only.
struct KpPairArgs : KpHeadArgs {
    SwapTable swap;
    int shift;               // 1: HRNet's SHIFT_HEATMAP (the flipped-back heatmap moved one column to the right, column 0 kept)
    float mirror_w;          // kcrop2[1].x = (mirror_w - x) - 1
};
hipError_t launch_kp_head_forward_pair(KpPairArgs a, hipStream_t s);
// heatmap supervision (capf_kp_heatmap_loss): the head's logits against analytic Gaussian targets, loss and parameter gradients in one entry
constexpr int KP_LOSS_MAX_RADIUS = 64;
struct KpLossGeom {                          // kp_loss_geom: floats of scratch, in this order; ok = false: a shape the kernels do not take
    KpGeom g;
    size_t sq_elems, item_elems, frame_elems, bw_elems;      // block sums of (z - t)^2 | g_bj (OHKM only) | frame sums | dW and dbias partials
    bool ok;
};
KpLossGeom kp_loss_geom(int B, int H, int W, int C, int J);
struct KpLossArgs {
    const void* x;           // [B, H, W, C] NHWC, dtype 0 fp32 / 1 bf16 / 2 fp16 (capf_dtype)
    int dtype;
    const float* wt;         // [J, C]
    const float* bias;       // [J] or NULL
    const float* gt;         // [B, J, 2] crop pixels
    const float* tw;         // [B, J] or NULL: 1
    int B, H, W, C, J;
    float dec[4];            // sx, ox, sy, oy
    float sigma;
    int radius;              // ceil(3 sigma)
    int reduction, topk;     // 0 mean, 1 OHKM
    float scale;
    float* loss;             // [1]
    float* joint_loss;       // [B, J] or NULL
    float* dW;               // [J, C] or NULL
    float* dbias;            // [J] or NULL
    float* dmap;             // [B, H, W, C] or NULL (fp32 map)
    int accumulate;
    float* scratch;
    // filled by the launcher
    KpLossGeom lg;
    float *sq_part, *gsel, *frame, *bw_part;
};
hipError_t launch_kp_heatmap_loss(KpLossArgs a, hipStream_t s);

// ---- CPN's detector head (CAPF_PLAN_CPN_PREDICT) ---------------------------------------------------------------------------------------
// elementwise.hip: out[p][i * row_bytes ..] = in[i][p][0 .. row_bytes) for the `pixels` NHWC pixels of n <= 4 maps of one channel count
// (row_bytes = channels x element size, a multiple of 16; 16 bytes per lane)
hipError_t launch_concat_channels(const float* const in[4], int n, float* out, long pixels, int row_bytes, hipStream_t s);
// cpn_decode.hip: CPN's two-peak heatmap decode (cpn/test.py:79-108; include/capf.h capf_cpn_decode has the rules), one workgroup per
// (frame, joint), the normalised plane (fp32) and the row pass of the blur (fp64) in LDS
constexpr int CPN_BORDER = 10, CPN_TAPS = 2 * CPN_BORDER + 1;
constexpr size_t CPN_LDS_LIMIT = 160 * 1024;
struct CpnDecodeArgs {
    const void* heat;        // [B, H, W, C] NHWC, dtype 0 fp32 / 1 bf16 / 2 fp16 (capf_dtype); joint j is channel j
    int dtype;
    int B, H, W, C, J;
    float dec[4];            // sx, ox, sy, oy
    const float* to_image;   // [B, 2, 3] or NULL
    float* kcrop;            // [B, J, 2]
    float* k2d;              // [B, J, 2] or NULL
    float* score;            // [B, J] or NULL
    double* blurred;         // [B, J, H + 20, W + 20] or NULL
    double g[CPN_TAPS];      // the Gaussian taps (cpn_decode_taps), filled by the launcher
};
void cpn_decode_taps(double g[CPN_TAPS]);
size_t cpn_decode_lds_bytes(int H, int W);       // what one workgroup needs (the launcher refuses more than CPN_LDS_LIMIT)
hipError_t launch_cpn_decode(CpnDecodeArgs a, hipStream_t s);
// CPN's test-time flip (capf_cpn_decode_pair; cpn/test.py:62-70): heat holds [2 B, H, W, C], frame B + b the mirror of source frame b; B counts
// SOURCE frames (the grid and to_image [B, 2, 3] are the single entry's at B).  The fold zf = 0.5 (zo + zm) happens in the load, the decode of zf
// is the single form's; kcrop / k2d are the stacks [2, B, J, 2], score [B, J], blurred [B, J, H + 20, W + 20].
struct CpnPairArgs : CpnDecodeArgs {
    SwapTable swap;
    float mirror_w;          // kcrop2[1].x = (mirror_w - x) - 1
    float* fused;            // [B, J, H, W] or NULL: zf, as the decode used it
};
hipError_t launch_cpn_decode_pair(CpnPairArgs a, hipStream_t s);

}  // namespace capf
