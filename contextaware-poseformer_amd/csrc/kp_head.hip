// 2-D keypoint head on the highest-resolution context map (gfx950): HRNet's final_layer (a 1x1 conv, pose_hrnet.py:497-501) and the decode
// of its heatmaps in one pass over the map, plus the two backwards (integral decode, heatmap loss).  include/capf.h (capf_kp_head_forward) has the rules.
//
// Map X [B, H, W, C] NHWC (fp32 / bf16 / fp16, widened on load), Wt [J, C] fp32, bias [J] fp32 or NULL; J <= 32, C % 4 == 0, C <= 512.
// A logit is ONE fp32 expression, plain FMAs on the vector pipe (no matrix pipe: block scales shared across pixels would tie a frame's argmax
// to its neighbours in the batch):
//     z = bias[j];  for c = 0 .. C-1 ascending:  z = fmaf(X[b, y, x, c], Wt[j, c], z)
// kp_logits (all joints of a pixel) and kp_logit1 (one joint, the argmax's four neighbours) are that chain, so they agree bit for bit.
//
// Forward, two launches, no atomics, no hand-off between blocks inside a launch:
//   slab     a block owns one frame's slab of `slab_tiles` consecutive 256-pixel tiles (row-major pixel index; the tiling depends on H * W
//            alone, never on the batch).  Per tile: thread t computes the J logits of pixel t into LDS (and into `heat` when asked); then 8 lanes
//            per joint walk the tile, lane l taking pixels l, l + 8, ... ascending, and keep the running best (argmax) or the online
//            max / sum / sum * col / sum * row of exp(beta z - max) (integral).  The 8 lanes are combined in ascending l; one record per
//            (frame, slab, joint) goes to the scratch.  The heatmaps never reach memory.
//   combine  one thread per (frame, joint) folds the slabs in ascending order, decodes, and writes kcrop / k2d / score.  The argmax's quarter
//            shift recomputes the winner's four neighbours from the map (4 C values per joint; the only second read).
// Flip-test pair (capf_kp_head_forward_pair), the PAIR instantiations of the same two kernels: the map holds [2 B] frames, frame B + b the mirror of
//   frame b.  slab: after its own pixel's logits, thread t computes those of the mirror frame's pixel that flip_back + SHIFT_HEATMAP put on pixel t
//   (same row, column kp_mirror_col; 256-pixel tiles are not row-aligned, so it lies in another tile and is read from memory) and folds them into its
//   OWN LDS column at swap[j]: zf = 0.5 (zo + zm).  No extra barrier, no runtime-indexed registers; the walk, the merges and the records are the
//   single form's.  combine: the quarter shift's neighbours are fused logits recomputed from both frames; both sets of the [2, B, J, 2] stacks.
// Gradients, ONE kernel body and ONE reduce for every producer of dz = dL/dz -- the section at the end:
//   kp_grad_kernel<L, Rule>  a block owns a frame's eighth of the tiles.  Per tile it recomputes the logits, asks the rule for the value of each
//            (pixel, joint) -- what goes to the LDS tile and the dz that multiplies Wt --, writes dmap[pixel, c] = sum_j dz Wt[j, c] (every element by
//            one thread) and adds per-block partials of dW = sum dz X (pixels ascending inside a tile, tiles ascending inside a block).
//   kp_reduce_kernel         sums the partials: part q of 16 takes blocks q, q + 16, ... ascending, the parts ascending.
//   A rule is the per-block LDS state beside the tile, the set-up in front of the first barrier, the value of one (pixel, joint), and two
//   policies (a tile's sum scaled per joint; J bias columns):
//     KpIntegralRule  the backward of the integral decode (capf_kp_head_backward; fp32 map), four launches: slab + combine as above leave
//                     (max, sum, x, y) per (frame, joint) in the scratch, the rule forms dz from them; the reduce writes dbias = 0.
//     KpGaussRule     heatmap supervision (capf_kp_heatmap_loss): d = z - t against analytic Gaussian targets, dz = g_bj d; the same body also
//                     adds the d^2 of the loss (LOSS), and the reduce's extra last block sums the frames.
#include <math.h>

#include "kernels.h"
#include "pair_stacks.h"

namespace capf {

typedef fmt_f32x4 f32x4;

static constexpr int KP_THREADS = 256;            // = pixels of a tile
static constexpr int KP_ZS = KP_THREADS + 8;      // LDS pitch of a joint's tile of logits: the 8 joints x 8 lanes of a wave hit 64 banks
static constexpr int KP_REC = 8;                  // floats per (frame, slab, joint) record: m, sum, sum_x, sum_y, zmax, nan, idx, -
static constexpr int KP_RED_PARTS = 16;

KpGeom kp_geom(int B, int H, int W, int C, int J) {
    KpGeom g{};
    if (!kp_shape_ok(B, H, W, C, J)) return g;
    const long HW = (long)H * W;
    if (HW > (1L << 24)) return g;                                  // (a pixel index and its row / column are exact in fp32)
    g.ntiles = (int)((HW + KP_THREADS - 1) / KP_THREADS);
    g.slab_tiles = (g.ntiles + KP_MAX_SLABS - 1) / KP_MAX_SLABS;
    g.nslab = (g.ntiles + g.slab_tiles - 1) / g.slab_tiles;
    g.bw_tiles = (g.ntiles + KP_BW_SLABS - 1) / KP_BW_SLABS;
    g.nbw = (g.ntiles + g.bw_tiles - 1) / g.bw_tiles;
    if ((long)B * g.nslab >= (1L << 31) || (long)B * J >= (1L << 31)) return KpGeom{};      // (grid sizes; addresses are 64-bit)
    g.fwd_elems = (size_t)B * g.nslab * J * KP_REC;
    g.stat_elems = (size_t)B * J * 4;
    g.bw_elems = (size_t)B * g.nbw * J * C;
    g.ok = true;
    return g;
}

// the J logits of one pixel: acc[j] = bias[j], then one fmaf per channel, ascending
template <class L>
__device__ __forceinline__ void kp_logits(const typename L::T* __restrict__ xp, const float* __restrict__ wt, const float* __restrict__ bias,
                                          const int C, const int J, float (&acc)[MAX_JOINTS]) {
#pragma unroll
    for (int j = 0; j < MAX_JOINTS; ++j) acc[j] = bias ? bias[j < J ? j : J - 1] : 0.f;
    for (int c = 0; c < C; c += 4) {                                // (loads grouped 16 channels ahead of their FMAs measured no faster: R24.1)
        const f32x4 v = L::ld4(xp + c);
#pragma unroll
        for (int jg = 0; jg < MAX_JOINTS / 4; ++jg) {
            if (jg * 4 < J) {                                       // (uniform; the joints of a group beyond J compute a copy of joint J - 1)
#pragma unroll
                for (int jj = 0; jj < 4; ++jj) {
                    const int j = jg * 4 + jj;
                    const float* __restrict__ w = wt + (size_t)(j < J ? j : J - 1) * C + c;
                    float z = acc[j];
                    z = fmaf(v[0], w[0], z);
                    z = fmaf(v[1], w[1], z);
                    z = fmaf(v[2], w[2], z);
                    z = fmaf(v[3], w[3], z);
                    acc[j] = z;
                }
            }
        }
    }
}

template <class L>
__device__ __forceinline__ float kp_logit1(const typename L::T* __restrict__ xp, const float* __restrict__ w, const float b, const int C) {
    float z = b;
    for (int c = 0; c < C; c += 4) {
        const f32x4 v = L::ld4(xp + c);
        z = fmaf(v[0], w[c], z);
        z = fmaf(v[1], w[c + 1], z);
        z = fmaf(v[2], w[c + 2], z);
        z = fmaf(v[3], w[c + 3], z);
    }
    return z;
}

struct KpRun {           // a lane's / slab's / frame's running decode state of one joint
    float m, s, sx, sy;  // integral: max of beta z, sums of e = exp(beta z - m), e col, e row
    float zm;            // max logit
    int idx;             // argmax: where zm was first seen
    int nan;
};
__device__ __forceinline__ KpRun kp_run_init() { return KpRun{-INFINITY, 0.f, 0.f, 0.f, -INFINITY, 0, 0}; }

// `o` holds pixels that all come AFTER r's in row-major order, or (lanes of a tile) interleave with them: the index breaks a tie
template <int MODE>
__device__ __forceinline__ void kp_run_merge(KpRun& r, const KpRun& o) {
    r.nan |= o.nan;
    if (MODE == 0) {
        if (o.zm > r.zm || (o.zm == r.zm && o.idx < r.idx)) { r.zm = o.zm; r.idx = o.idx; }
    } else {
        const float M = o.m > r.m ? o.m : r.m;
        const float e1 = r.m == M ? 1.f : expf(r.m - M), e2 = o.m == M ? 1.f : expf(o.m - M);
        r.s = r.s * e1 + o.s * e2;
        r.sx = r.sx * e1 + o.sx * e2;
        r.sy = r.sy * e1 + o.sy * e2;
        r.m = M;
        if (o.zm > r.zm) r.zm = o.zm;
    }
}

// the column of the mirror frame whose logit the flip test puts on column x: flip_back mirrors in x, SHIFT_HEATMAP then moves the flipped-back
// heatmap one column to the right (column 0 keeps its own value)
__device__ __forceinline__ int kp_mirror_col(const int x, const int W, const int shift) { return W - 1 - (shift && x >= 1 ? x - 1 : x); }

template <bool PAIR> struct KpArgsOf { typedef KpHeadArgs type; };
template <> struct KpArgsOf<true> { typedef KpPairArgs type; };

// PAIR: the tile holds the FUSED logits of source frame b, zf = 0.5 (zo + zm) -- thread t adds, into its own LDS column, the logits of the
// pixel of frame B + b that the flip test puts on pixel t (joint js of the mirror lands on joint swap[js]); nobody else touches that column,
// so the fold needs no barrier.  Everything after it is the single decode.
template <class L, int MODE, bool PAIR>
__global__ void __launch_bounds__(KP_THREADS) kp_fwd_slab_kernel(const typename KpArgsOf<PAIR>::type a) {
    __shared__ float zs[MAX_JOINTS * KP_ZS];
    const int tid = threadIdx.x;
    const int b = (int)blockIdx.x / a.g.nslab, s = (int)blockIdx.x - b * a.g.nslab;
    const int HW = a.H * a.W, J = a.J;
    const typename L::T* __restrict__ xb = static_cast<const typename L::T*>(a.x) + (size_t)b * HW * a.C;
    const typename L::T* __restrict__ xm = xb + (size_t)a.B * HW * a.C;        // (PAIR) frame B + b
    const int jl = tid >> 3, l = tid & 7;
    KpRun r = kp_run_init();
    const int t0 = s * a.g.slab_tiles;
    const int t1 = t0 + a.g.slab_tiles < a.g.ntiles ? t0 + a.g.slab_tiles : a.g.ntiles;
    for (int t = t0; t < t1; ++t) {
        const int pix = t * KP_THREADS + tid;
        if (pix < HW) {
            float acc[MAX_JOINTS];
            kp_logits<L>(xb + (size_t)pix * a.C, a.wt, a.bias, a.C, J, acc);
#pragma unroll
            for (int j = 0; j < MAX_JOINTS; ++j) {
                if (j < J) {
                    zs[j * KP_ZS + tid] = acc[j];
                    if (!PAIR && a.heat) a.heat[((size_t)b * J + j) * HW + pix] = acc[j];
                }
            }
            if constexpr (PAIR) {
                const int row = pix / a.W, col = pix - row * a.W;
                kp_logits<L>(xm + ((size_t)row * a.W + kp_mirror_col(col, a.W, a.shift)) * a.C, a.wt, a.bias, a.C, J, acc);
#pragma unroll
                for (int js = 0; js < MAX_JOINTS; ++js) {
                    if (js < J) {
                        float* z = zs + a.swap.j[js] * KP_ZS + tid;
                        *z = __fmul_rn(0.5f, __fadd_rn(*z, acc[js]));  // the fp32 sum rounded once, then halved
                    }
                }
                if (a.heat)
                    for (int j = 0; j < J; ++j) a.heat[((size_t)b * J + j) * HW + pix] = zs[j * KP_ZS + tid];
            }
        }
        __syncthreads();
        if (jl < J) {
            const int base = t * KP_THREADS;
            const int n = HW - base < KP_THREADS ? HW - base : KP_THREADS;
            for (int p = l; p < n; p += 8) {
                const float z = zs[jl * KP_ZS + p];
                const int pp = base + p;
                if (z != z) r.nan = 1;
                if (MODE == 0) {
                    if (z > r.zm) { r.zm = z; r.idx = pp; }
                } else {
                    const int row = pp / a.W, col = pp - row * a.W;
                    const float tz = a.beta * z;
                    if (tz > r.m) {
                        const float e = expf(r.m - tz);             // (first pixel: exp(-inf) = 0 on zero sums)
                        r.s *= e; r.sx *= e; r.sy *= e;
                        r.m = tz;
                    }
                    const float w = expf(tz - r.m);
                    r.s += w;
                    r.sx = fmaf(w, (float)col, r.sx);
                    r.sy = fmaf(w, (float)row, r.sy);
                    if (z > r.zm) r.zm = z;
                }
            }
        }
        __syncthreads();
    }
    if constexpr (PAIR) {
        // with the shift no pixel reads the mirror's column 0, and its logits still count for the NaN rule: the joint's lanes recompute
        // those of the rows that start inside this slab
        if (a.shift && a.W > 1 && jl < J) {
            const int js = a.swap.j[jl];
            const float* w = a.wt + (size_t)js * a.C;
            const float bj = a.bias ? a.bias[js] : 0.f;
            const int p1 = t1 * KP_THREADS < HW ? t1 * KP_THREADS : HW;
            for (int row = (t0 * KP_THREADS + a.W - 1) / a.W + l; row * a.W < p1; row += 8) {
                const float z = kp_logit1<L>(xm + (size_t)row * a.W * a.C, w, bj, a.C);
                if (z != z) r.nan = 1;
            }
        }
    }
    // the 8 lanes of a joint, ascending (every thread takes part in the shuffles)
    KpRun tot = r;
    for (int q = 1; q < 8; ++q) {
        KpRun o;
        o.m = __shfl(r.m, q, 8); o.s = __shfl(r.s, q, 8); o.sx = __shfl(r.sx, q, 8); o.sy = __shfl(r.sy, q, 8);
        o.zm = __shfl(r.zm, q, 8); o.idx = __shfl(r.idx, q, 8); o.nan = __shfl(r.nan, q, 8);
        kp_run_merge<MODE>(tot, o);
    }
    if (l == 0 && jl < J) {
        float* rec = a.part + ((size_t)blockIdx.x * J + jl) * KP_REC;
        rec[0] = tot.m; rec[1] = tot.s; rec[2] = tot.sx; rec[3] = tot.sy;
        rec[4] = tot.zm; rec[5] = tot.nan ? 1.f : 0.f; rec[6] = __int_as_float(tot.idx); rec[7] = 0.f;
    }
}

// one fused logit of the pair, from the map: the expression of the slab kernel's fold
template <class L>
__device__ __forceinline__ float kp_pair_logit1(const KpPairArgs& a, const int b, const int j, const int py, const int px) {
    const typename L::T* x = static_cast<const typename L::T*>(a.x);
    const size_t HW = (size_t)a.H * a.W;
    const int js = a.swap.j[j];
    const float zo = kp_logit1<L>(x + ((size_t)b * HW + (size_t)py * a.W + px) * a.C, a.wt + (size_t)j * a.C, a.bias ? a.bias[j] : 0.f, a.C);
    const float zm = kp_logit1<L>(x + ((size_t)(a.B + b) * HW + (size_t)py * a.W + kp_mirror_col(px, a.W, a.shift)) * a.C,
                                  a.wt + (size_t)js * a.C, a.bias ? a.bias[js] : 0.f, a.C);
    return __fmul_rn(0.5f, __fadd_rn(zo, zm));
}

// The pair's outputs from the decoded heatmap coordinates (x, y) of (b, j): write_pair_stacks' (pair_stacks.h).  Every operation is rounded on
// its own, as capf.h writes the expressions: __fmul_rn / __fadd_rn are plain operators to this compiler, which contracts A00 kx + A01 ky of the
// single form below into an fma (that form keeps the code it always had); here contraction is off, for the decode scale as in the writer.
__device__ __forceinline__ void kp_pair_outputs(const KpPairArgs& a, const int b, const int j, const float x, const float y, const float score) {
#pragma clang fp contract(off)
    const size_t o = (size_t)b * a.J + j, om = (size_t)(a.B + b) * a.J + a.swap.j[j];       // (B <= 2^30: B + b is an int)
    write_pair_stacks(a.kcrop, a.k2d, a.score, o, om, a.to_image && a.k2d ? a.to_image + (size_t)b * 6 : nullptr, a.mirror_w,
                      a.dec[0] * x + a.dec[1], a.dec[2] * y + a.dec[3], score);
}

// PAIR: the neighbours of the quarter shift are fused logits; the outputs are kp_pair_outputs'
template <class L, int MODE, bool PAIR>
__global__ void __launch_bounds__(KP_THREADS) kp_fwd_combine_kernel(const typename KpArgsOf<PAIR>::type a) {
    const int i = (int)blockIdx.x * KP_THREADS + threadIdx.x;
    if (i >= a.B * a.J) return;
    const int b = i / a.J, j = i - b * a.J, J = a.J, H = a.H, W = a.W;
    KpRun r = kp_run_init();
    r.idx = 0x7fffffff;
    for (int s = 0; s < a.g.nslab; ++s) {                           // slabs ascending
        const float* rec = a.part + (((size_t)b * a.g.nslab + s) * J + j) * KP_REC;
        KpRun o{rec[0], rec[1], rec[2], rec[3], rec[4], __float_as_int(rec[6]), rec[5] != 0.f};
        kp_run_merge<MODE>(r, o);
    }
    float x, y, score = r.zm;
    if (MODE == 0) {
        if (r.idx == 0x7fffffff) r.idx = 0;
        const int py = r.idx / W, px = r.idx - py * W;
        x = (float)px;
        y = (float)py;
        if constexpr (PAIR) {
            if (!r.nan && 1 < px && px < W - 1 && 1 < py && py < H - 1) {
                const float dx = kp_pair_logit1<L>(a, b, j, py, px + 1) - kp_pair_logit1<L>(a, b, j, py, px - 1);
                const float dy = kp_pair_logit1<L>(a, b, j, py + 1, px) - kp_pair_logit1<L>(a, b, j, py - 1, px);
                x += dx > 0.f ? 0.25f : dx < 0.f ? -0.25f : 0.f;
                y += dy > 0.f ? 0.25f : dy < 0.f ? -0.25f : 0.f;
            }
        } else if (!r.nan && 1 < px && px < W - 1 && 1 < py && py < H - 1) {
            const typename L::T* xp = static_cast<const typename L::T*>(a.x) + ((size_t)b * H * W + r.idx) * a.C;
            const float* w = a.wt + (size_t)j * a.C;
            const float bj = a.bias ? a.bias[j] : 0.f;
            const float dx = kp_logit1<L>(xp + a.C, w, bj, a.C) - kp_logit1<L>(xp - a.C, w, bj, a.C);
            const float dy = kp_logit1<L>(xp + (size_t)W * a.C, w, bj, a.C) - kp_logit1<L>(xp - (size_t)W * a.C, w, bj, a.C);
            x += dx > 0.f ? 0.25f : dx < 0.f ? -0.25f : 0.f;
            y += dy > 0.f ? 0.25f : dy < 0.f ? -0.25f : 0.f;
        }
        if (score <= 0.f) x = y = 0.f;
    } else {
        x = r.sx / r.s;
        y = r.sy / r.s;
    }
    if (r.nan) x = y = score = __builtin_nanf("");
    if constexpr (PAIR) {
        kp_pair_outputs(a, b, j, x, y, score);
        return;
    }
    if (a.stats) {
        float* st = a.stats + (size_t)i * 4;
        st[0] = r.m; st[1] = r.s; st[2] = x; st[3] = y;
    }
    if (!a.kcrop) return;
    const float kx = __fadd_rn(__fmul_rn(a.dec[0], x), a.dec[1]), ky = __fadd_rn(__fmul_rn(a.dec[2], y), a.dec[3]);
    a.kcrop[(size_t)i * 2] = kx;
    a.kcrop[(size_t)i * 2 + 1] = ky;
    if (a.score) a.score[i] = score;
    if (a.to_image && a.k2d) {
        const float* A = a.to_image + (size_t)b * 6;
        a.k2d[(size_t)i * 2] = __fadd_rn(__fadd_rn(__fmul_rn(A[0], kx), __fmul_rn(A[1], ky)), A[2]);
        a.k2d[(size_t)i * 2 + 1] = __fadd_rn(__fadd_rn(__fmul_rn(A[3], kx), __fmul_rn(A[4], ky)), A[5]);
    }
}

template <class L, bool PAIR = false>
static void kp_forward_launches(const typename KpArgsOf<PAIR>::type& a, hipStream_t s) {
    const dim3 g1((unsigned)(a.B * a.g.nslab)), g2((unsigned)((a.B * a.J + KP_THREADS - 1) / KP_THREADS));
    if (a.mode == 0) {
        hipLaunchKernelGGL((kp_fwd_slab_kernel<L, 0, PAIR>), g1, dim3(KP_THREADS), 0, s, a);
        hipLaunchKernelGGL((kp_fwd_combine_kernel<L, 0, PAIR>), g2, dim3(KP_THREADS), 0, s, a);
    } else {
        hipLaunchKernelGGL((kp_fwd_slab_kernel<L, 1, PAIR>), g1, dim3(KP_THREADS), 0, s, a);
        hipLaunchKernelGGL((kp_fwd_combine_kernel<L, 1, PAIR>), g2, dim3(KP_THREADS), 0, s, a);
    }
}

static bool kp_args_ok(const KpHeadArgs& a) {
    return a.g.ok && a.x && a.wt && a.part && (a.mode == 0 || a.mode == 1) && a.beta > 0.f && a.dtype >= 0 && a.dtype <= 2;
}

hipError_t launch_kp_head_forward(KpHeadArgs a, hipStream_t s) {
    a.g = kp_geom(a.B, a.H, a.W, a.C, a.J);
    if (!kp_args_ok(a) || !a.kcrop) return hipErrorInvalidValue;
    a.stats = nullptr;
    with_map_loader(a.dtype, [&](auto l) { kp_forward_launches<decltype(l)>(a, s); });
    return hipGetLastError();
}

hipError_t launch_kp_head_forward_pair(KpPairArgs a, hipStream_t s) {
    a.g = kp_geom(a.B, a.H, a.W, a.C, a.J);
    if (!kp_args_ok(a) || !a.kcrop || a.B > (1 << 30) || (a.shift != 0 && a.shift != 1) || !swap_table_ok(a.swap.j, a.J)) return hipErrorInvalidValue;
    a.stats = nullptr;
    with_map_loader(a.dtype, [&](auto l) { kp_forward_launches<decltype(l), true>(a, s); });
    return hipGetLastError();
}

// ---- gradients: one kernel body, one reduce; a rule per producer of dz ----------------------------------------------------------------
// Heatmap supervision (capf_kp_heatmap_loss; include/capf.h has the rules): d = z - t per (pixel, joint) in the LDS tile, z being kp_logits'
// chain and t the analytic Gaussian target (a product of two entries of a per-block fp64 table; the difference is formed in fp64 and rounded
// once); neither reaches memory.
//   kp_grad_kernel<KpGaussRule, LOSS>  8 lanes per joint add d^2 (lane l: pixels l, l + 8, ... of each tile, tiles ascending; lanes ascending):
//                                      one sum per (block, joint)
//   kp_loss_items_kernel               one thread per (frame, joint): blocks ascending -> l_bj; the OHKM rank and g_bj; the frame's sum, joints ascending
//   kp_grad_kernel<KpGaussRule, GRAD>  dz = g_bj d in registers -> dmap; per block partials of sum d X and sum d, scaled by g_bj per tile
//   kp_reduce_kernel                   the partials -> dweight, dbias; its last block the frames' sums -> loss
// reduction 0 knows g_bj up front: <LOSS, GRAD> is one pass over the map.  OHKM: <LOSS>, items, <GRAD> (the logits recomputed).
KpLossGeom kp_loss_geom(int B, int H, int W, int C, int J) {
    KpLossGeom lg{};
    lg.g = kp_geom(B, H, W, C, J);
    if (!lg.g.ok) return lg;
    lg.sq_elems = (size_t)B * lg.g.nbw * J;
    lg.item_elems = (size_t)B * J;
    lg.frame_elems = (size_t)B;
    lg.bw_elems = (size_t)B * lg.g.nbw * ((size_t)J * C + J);
    lg.ok = true;
    return lg;
}

struct KpLossItem { int mux, muy; float w; };   // the target's centre and the effective weight of one (frame, joint)
static constexpr int KP_LOSS_NOWHERE = -(1 << 25);   // a centre whose window holds no pixel (columns and rows are below 2^24)

__device__ __forceinline__ KpLossItem kp_loss_item(const KpLossArgs& a, const size_t i) {
    const float cx = __fdiv_rn(__fsub_rn(a.gt[i * 2], a.dec[1]), a.dec[0]);
    const float cy = __fdiv_rn(__fsub_rn(a.gt[i * 2 + 1], a.dec[3]), a.dec[2]);
    KpLossItem it{KP_LOSS_NOWHERE, KP_LOSS_NOWHERE, 0.f};
    if (fabsf(cx) <= 1048576.f && fabsf(cy) <= 1048576.f) {         // (false for a NaN)
        it.mux = (int)__fadd_rn(cx, 0.5f);
        it.muy = (int)__fadd_rn(cy, 0.5f);
        const int R = a.radius;
        const bool outside = it.mux - R >= a.W || it.muy - R >= a.H || it.mux + R < 0 || it.muy + R < 0;
        it.w = outside ? 0.f : a.tw ? a.tw[i] : 1.f;
    }
    return it;
}
// the loss is the frames' sums over B * count, count being the joints a frame's sum takes: all J (mean) or topk (OHKM)
__host__ __device__ __forceinline__ int kp_loss_count(const KpLossArgs& a) { return a.reduction == 0 ? a.J : a.topk; }
__device__ __forceinline__ float kp_loss_norm(const int B, const int count) { return __fmul_rn((float)B, (float)count); }
// g_bj of a selected item: 2 scale w^2 / (H W norm)
__device__ __forceinline__ float kp_loss_g(const KpLossArgs& a, const float w) {
    return __fdiv_rn(__fmul_rn(__fmul_rn(__fmul_rn(2.f, a.scale), w), w), __fmul_rn((float)(a.H * a.W), kp_loss_norm(a.B, kp_loss_count(a))));
}

// the backward of the integral decode: dz = beta p (gx (col - x) + gy (row - y)), p the softmax of beta z, (gx, gy) the cotangent of the
// heatmap coordinates.  The LDS tile holds dz itself; no bias column (softmax is shift-invariant: dbias is exactly zero)
struct KpIntegralRule {
    typedef KpHeadArgs Args;
    struct Shared { float st[MAX_JOINTS][6]; };                     // m, 1 / sum, x, y, gx, gy
    static constexpr bool SCALE_TILE = false, BIAS_COLS = false;
    static __device__ __forceinline__ const KpGeom& geom(const Args& a) { return a.g; }
    template <bool LOSS, bool GRAD>
    static __device__ __forceinline__ void setup(const Args& a, const int b, const int tid, Shared& sh) {
        float (&st)[MAX_JOINTS][6] = sh.st;
        const int J = a.J;
        if (tid < J) {
            const size_t i = (size_t)b * J + tid;
            const float* sv = a.stats + i * 4;
            float gx = a.dkcrop ? a.dkcrop[i * 2] : 0.f, gy = a.dkcrop ? a.dkcrop[i * 2 + 1] : 0.f;
            if (a.dk2d) {                                               // g += A[:, :2]^T dk2d
                const float* A = a.to_image + (size_t)b * 6;
                const float d0 = a.dk2d[i * 2], d1 = a.dk2d[i * 2 + 1];
                gx += A[0] * d0 + A[3] * d1;
                gy += A[1] * d0 + A[4] * d1;
            }
            st[tid][0] = sv[0]; st[tid][1] = 1.f / sv[1]; st[tid][2] = sv[2]; st[tid][3] = sv[3];
            st[tid][4] = gx * a.dec[0]; st[tid][5] = gy * a.dec[2];
        }
    }
    static __device__ __forceinline__ void value(const Args& a, const Shared& sh, const int j, const int row, const int col, const float z,
                                                 float& lds, float& dzo) {
        const float (&st)[MAX_JOINTS][6] = sh.st;
        const float p = expf(a.beta * z - st[j][0]) * st[j][1];
        const float dz = a.beta * p * (st[j][4] * ((float)col - st[j][2]) + st[j][5] * ((float)row - st[j][3]));
        lds = dz;
        dzo = dz;
    }
};

// heatmap supervision: the LDS tile holds the unscaled d = z - t (the loss adds its squares), dz = g_bj d; a tile's sums of d X and of d are
// scaled by g_bj, and the J bias columns are real
struct KpGaussRule {
    typedef KpLossArgs Args;
    struct alignas(16) Shared {                                     // (16: the alignment, and with it the size, the fp64 table has as an LDS array)
        int mu[MAX_JOINTS][2];
        float gj[MAX_JOINTS];
        double eg[KP_LOSS_MAX_RADIUS + 1];                          // exp(-k^2 / (2 sigma^2)), k = 0 .. R: the target is eg[|dx|] eg[|dy|]
    };
    static constexpr bool SCALE_TILE = true, BIAS_COLS = true;
    static __device__ __forceinline__ const KpGeom& geom(const Args& a) { return a.lg.g; }
    template <bool LOSS, bool GRAD>
    static __device__ __forceinline__ void setup(const Args& a, const int b, const int tid, Shared& sh) {
        const int J = a.J, R = a.radius;
        if (tid <= R) sh.eg[tid] = exp(-(double)(tid * tid) / (2.0 * (double)a.sigma * (double)a.sigma));
        if (tid < J) {
            const size_t i = (size_t)b * J + tid;
            const KpLossItem it = kp_loss_item(a, i);
            sh.mu[tid][0] = it.mux; sh.mu[tid][1] = it.muy;
            sh.gj[tid] = !GRAD ? 0.f : LOSS ? kp_loss_g(a, it.w) : a.gsel[i];
        }
    }
    static __device__ __forceinline__ void value(const Args& a, const Shared& sh, const int j, const int row, const int col, const float z,
                                                 float& lds, float& dzo) {
        const int R = a.radius;
        const int dx = col - sh.mu[j][0], dy = row - sh.mu[j][1];
        // z - t in double, rounded once: its error is relative to |z - t|, not to t, also where the two nearly cancel
        float d = z;
        if (dx >= -R && dx <= R && dy >= -R && dy <= R) d = (float)__fma_rn(-sh.eg[abs(dx)], sh.eg[abs(dy)], (double)z);
        lds = d;
        dzo = sh.gj[j] == 0.f ? 0.f : __fmul_rn(sh.gj[j], d);      // (an item without weight: exact zeros, whatever its logits)
    }
};

// LOSS: the sums of the tile values' squares per (block, joint) -> a.sq_part.  GRAD: dmap and the block's partials -> a.bw_part
// ([nout] per block, nout = J C (+ J with BIAS_COLS)), either only where the caller asked for it.
template <class L, class Rule, bool LOSS, bool GRAD>
__global__ void __launch_bounds__(KP_THREADS) kp_grad_kernel(const typename Rule::Args a) {
    __shared__ float zs[MAX_JOINTS * KP_ZS];
    __shared__ typename Rule::Shared sh;
    const int tid = threadIdx.x;
    const int nbw = Rule::geom(a).nbw, bw_tiles = Rule::geom(a).bw_tiles, ntiles = Rule::geom(a).ntiles;
    const int b = (int)blockIdx.x / nbw, s = (int)blockIdx.x - b * nbw;
    const int HW = a.H * a.W, J = a.J, C = a.C;
    const typename L::T* __restrict__ xb = static_cast<const typename L::T*>(a.x) + (size_t)b * HW * C;
    Rule::template setup<LOSS, GRAD>(a, b, tid, sh);
    __syncthreads();
    const int JC = J * C, nout = Rule::BIAS_COLS ? JC + J : JC;
    const bool wgrad = GRAD && (a.dW || a.dbias);
    float* part = a.bw_part + (size_t)blockIdx.x * nout;
    const int jl = tid >> 3, l = tid & 7;
    float sq = 0.f;
    const int t0 = s * bw_tiles;
    const int t1 = t0 + bw_tiles < ntiles ? t0 + bw_tiles : ntiles;
    for (int t = t0; t < t1; ++t) {
        const int base = t * KP_THREADS, pix = base + tid;
        const int n = HW - base < KP_THREADS ? HW - base : KP_THREADS;
        if (pix < HW) {
            float acc[MAX_JOINTS];
            kp_logits<L>(xb + (size_t)pix * C, a.wt, a.bias, C, J, acc);
            const int row = pix / a.W, col = pix - row * a.W;
#pragma unroll
            for (int j = 0; j < MAX_JOINTS; ++j) {
                if (j < J) {
                    float v, dz;
                    Rule::value(a, sh, j, row, col, acc[j], v, dz);
                    zs[j * KP_ZS + tid] = v;
                    acc[j] = dz;
                }
            }
            if (GRAD && a.dmap) {                                   // dmap[pixel, c] = sum_j dz[j] Wt[j, c], joints ascending
                float* dp = a.dmap + ((size_t)b * HW + pix) * C;
                for (int c = 0; c < C; c += 4) {
                    f32x4 d = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                    for (int j = 0; j < MAX_JOINTS; ++j) {
                        if (j < J) {
                            const float* __restrict__ w = a.wt + (size_t)j * C + c;
                            d[0] = fmaf(acc[j], w[0], d[0]);
                            d[1] = fmaf(acc[j], w[1], d[1]);
                            d[2] = fmaf(acc[j], w[2], d[2]);
                            d[3] = fmaf(acc[j], w[3], d[3]);
                        }
                    }
                    f32x4* q = reinterpret_cast<f32x4*>(dp + c);
                    *q = a.accumulate ? *q + d : d;
                }
            }
        }
        __syncthreads();
        if (LOSS && jl < J) {
            for (int p = l; p < n; p += 8) {
                const float d = zs[jl * KP_ZS + p];
                sq = fmaf(d, d, sq);
            }
        }
        if (wgrad) {
            for (int o = tid; o < nout; o += KP_THREADS) {          // o >= JC: the bias of joint o - JC, whose "X" is 1
                const bool isb = Rule::BIAS_COLS && o >= JC;
                const int j = isb ? o - JC : o / C, c = isb ? 0 : o - j * C;
                const typename L::T* __restrict__ xc = xb + (size_t)base * C + c;
                const float* zj = zs + j * KP_ZS;
                float sum = 0.f;
                if (isb) {
                    for (int p = 0; p < n; ++p) sum = __fadd_rn(sum, zj[p]);
                } else {
#pragma unroll 8
                    for (int p = 0; p < n; ++p) sum = fmaf(zj[p], L::ld1(xc + (size_t)p * C), sum);
                }
                if constexpr (Rule::SCALE_TILE) sum = sh.gj[j] == 0.f ? 0.f : __fmul_rn(sh.gj[j], sum);
                part[o] = t == t0 ? sum : __fadd_rn(part[o], sum);
            }
        }
        __syncthreads();
    }
    if constexpr (LOSS) {                                           // the 8 lanes of a joint, ascending (every thread takes part in the shuffles)
        float tot = __shfl(sq, 0, 8);
        for (int q = 1; q < 8; ++q) tot = __fadd_rn(tot, __shfl(sq, q, 8));
        if (l == 0 && jl < J) a.sq_part[(size_t)blockIdx.x * J + jl] = tot;
    }
}

// 8 frames a block, 32 threads a frame: l_bj, the OHKM selection (rank = how many joints of the frame come before this one: a NaN first,
// then the larger loss, then the smaller index), g_bj of the gradient pass, and the frame's sum over its selected joints, ascending
__global__ void __launch_bounds__(KP_THREADS) kp_loss_items_kernel(const KpLossArgs a) {
    __shared__ float lv[8][MAX_JOINTS];
    __shared__ int sl[8][MAX_JOINTS];
    const int fl = threadIdx.x >> 5, j = threadIdx.x & 31;
    const long bl = (long)blockIdx.x * 8 + fl;
    const int J = a.J, nbw = a.lg.g.nbw;
    const bool live = bl < a.B && j < J;
    const int b = (int)(bl < a.B ? bl : 0);
    const size_t i = (size_t)b * J + j;
    float lj = 0.f, w = 0.f;
    if (live) {
        w = kp_loss_item(a, i).w;
        float sum = 0.f;
        for (int s = 0; s < nbw; ++s) sum = __fadd_rn(sum, a.sq_part[((size_t)b * nbw + s) * J + j]);
        lj = w == 0.f ? 0.f : __fmul_rn(__fmul_rn(__fmul_rn(a.scale, w), w), __fdiv_rn(sum, (float)(a.H * a.W)));
        if (a.joint_loss) a.joint_loss[i] = lj;
    }
    lv[fl][j] = lj;
    __syncthreads();
    int sel = live;
    if (live && a.reduction == 1) {
        int rank = 0;
        for (int jj = 0; jj < J; ++jj) {
            const float o = lv[fl][jj];
            const bool before = jj == j ? false : o != o ? (lj == lj || jj < j) : (lj == lj && (o > lj || (o == lj && jj < j)));
            rank += before;
        }
        sel = rank < a.topk;
        a.gsel[i] = sel ? kp_loss_g(a, w) : 0.f;
    }
    sl[fl][j] = sel;
    __syncthreads();
    if (live && j == 0) {
        float fs = 0.f;
        for (int jj = 0; jj < J; ++jj)
            if (sl[fl][jj]) fs = __fadd_rn(fs, lv[fl][jj]);
        a.frame[b] = fs;
    }
}

// blocks 0 .. ceil(nout / 16) - 1: column o of the blocks' partials in two stages (part q of 16 takes blocks q, q + 16, ... ascending, the parts
// ascending); o < JC goes to dW, the rest to dbias, either where it is not NULL.  zero_bias = J: no bias column exists and dbias is exact
// zeros.  loss != NULL: the grid has one more block, the last, for the frames' sums in the same two stages (frames for blocks) -> loss
__global__ void __launch_bounds__(KP_THREADS) kp_reduce_kernel(const float* __restrict__ part, const int nparts, const int nout, const int JC,
                                                               float* __restrict__ dW, float* __restrict__ dbias, const int zero_bias,
                                                               const float* __restrict__ frame, const int B, const int count, float* __restrict__ loss) {
    __shared__ float sh[KP_RED_PARTS][16];
    const int lc = threadIdx.x & 15, q = threadIdx.x >> 4;
    float s = 0.f;
    if (loss && blockIdx.x == gridDim.x - 1) {
        if (lc == 0)
            for (int p = q; p < B; p += KP_RED_PARTS) s = __fadd_rn(s, frame[p]);
        sh[q][lc] = s;
        __syncthreads();
        if (threadIdx.x == 0) {
            s = 0.f;
            for (int p = 0; p < KP_RED_PARTS; ++p) s = __fadd_rn(s, sh[p][0]);
            loss[0] = __fdiv_rn(s, kp_loss_norm(B, count));
        }
        return;
    }
    const int o = (int)blockIdx.x * 16 + lc;
    if (o < nout)
        for (int p = q; p < nparts; p += KP_RED_PARTS) s = __fadd_rn(s, part[(size_t)p * nout + o]);
    sh[q][lc] = s;
    __syncthreads();
    if (q == 0 && o < nout) {
        s = 0.f;
        for (int p = 0; p < KP_RED_PARTS; ++p) s = __fadd_rn(s, sh[p][lc]);
        if (o < JC) { if (dW) dW[o] = s; }
        else if (dbias) dbias[o - JC] = s;
    }
    if (blockIdx.x == 0 && dbias && (int)threadIdx.x < zero_bias) dbias[threadIdx.x] = 0.f;
}

hipError_t launch_kp_head_backward(KpHeadArgs a, hipStream_t s) {
    a.g = kp_geom(a.B, a.H, a.W, a.C, a.J);
    if (!kp_args_ok(a) || a.mode != 1 || a.dtype != 0 || !a.dW || (!a.dkcrop && !a.dk2d) || (a.dk2d && !a.to_image)) return hipErrorInvalidValue;
    a.stats = a.part + a.g.fwd_elems;
    a.bw_part = a.stats + a.g.stat_elems;
    a.kcrop = a.k2d = a.score = a.heat = nullptr;
    kp_forward_launches<MapLdF32>(a, s);
    const int nblocks = a.B * a.g.nbw, JC = a.J * a.C;
    hipLaunchKernelGGL((kp_grad_kernel<MapLdF32, KpIntegralRule, false, true>), dim3((unsigned)nblocks), dim3(KP_THREADS), 0, s, a);
    hipLaunchKernelGGL(kp_reduce_kernel, dim3((unsigned)((JC + 15) / 16)), dim3(KP_THREADS), 0, s, a.bw_part, nblocks, JC, JC, a.dW, a.dbias, a.J,
                       nullptr, 0, 0, nullptr);
    return hipGetLastError();
}

template <class L>
static void kp_loss_launches(const KpLossArgs& a, hipStream_t s) {
    const dim3 blk(KP_THREADS), g1((unsigned)(a.B * a.lg.g.nbw)), g2((unsigned)((a.B + 7) / 8));
    const bool grads = a.dW || a.dbias || a.dmap;
    if (grads && a.reduction == 0) hipLaunchKernelGGL((kp_grad_kernel<L, KpGaussRule, true, true>), g1, blk, 0, s, a);
    else hipLaunchKernelGGL((kp_grad_kernel<L, KpGaussRule, true, false>), g1, blk, 0, s, a);
    hipLaunchKernelGGL(kp_loss_items_kernel, g2, blk, 0, s, a);
    if (grads && a.reduction == 1) hipLaunchKernelGGL((kp_grad_kernel<L, KpGaussRule, false, true>), g1, blk, 0, s, a);
    const int JC = a.J * a.C, nout = a.dW || a.dbias ? JC + a.J : 0;
    hipLaunchKernelGGL(kp_reduce_kernel, dim3((unsigned)((nout + 15) / 16 + 1)), blk, 0, s, a.bw_part, a.B * a.lg.g.nbw, nout, JC, a.dW, a.dbias, 0,
                       a.frame, a.B, kp_loss_count(a), a.loss);
}

hipError_t launch_kp_heatmap_loss(KpLossArgs a, hipStream_t s) {
    a.lg = kp_loss_geom(a.B, a.H, a.W, a.C, a.J);
    if (!a.lg.ok || !a.x || !a.wt || !a.gt || !a.loss || !a.scratch || a.dtype < 0 || a.dtype > 2 || (a.reduction != 0 && a.reduction != 1) ||
        a.topk < 1 || a.radius < 0 || a.radius > KP_LOSS_MAX_RADIUS || (a.dmap && a.dtype != 0))
        return hipErrorInvalidValue;
    a.sq_part = a.scratch;
    a.gsel = a.sq_part + a.lg.sq_elems;
    a.frame = a.gsel + (a.reduction == 1 ? a.lg.item_elems : 0);
    a.bw_part = a.frame + a.lg.frame_elems;
    with_map_loader(a.dtype, [&](auto l) { kp_loss_launches<decltype(l)>(a, s); });
    return hipGetLastError();
}

}  // namespace capf

