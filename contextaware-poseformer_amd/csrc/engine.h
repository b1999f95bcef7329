// Internal model of the hot path: parameter schema, static layer plan, workspace layout.
// (Public ABI: include/capf.h.)  Host-side C++; no torch types anywhere.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>
#include <map>
#include <string>
#include <variant>
#include <vector>

#include "capf.h"
#include "kernels.h"

namespace capf {

struct Param {
    std::string name;
    int64_t shape[4] = {0, 0, 0, 0};
    int ndim = 0;
    int kind = 0;
    const float* ptr = nullptr;  // borrowed device pointer (capf_set_param)
    int64_t numel() const {
        int64_t n = 1;
        for (int i = 0; i < ndim; ++i) n *= shape[i];
        return n;
    }
};

// Activation buffer inside the caller-owned workspace.  Sizes / offsets are per frame (elements);
// the run-time address is ws + offset * batch, so one plan serves every batch <= max_batch.
struct Buffer {
    size_t elems = 0;       // per frame, rounded up to 64 elements (256 B)
    size_t offset = 0;      // per frame, assigned by assign_offsets()
    int def_op = -1;        // first op that writes it
    int last_op = -1;       // last op that reads it (INT_MAX: persists to the end of forward)
    std::string tag;        // debug name ("feat0", "tok", ...)
};

struct Tensor {  // NHWC view of a buffer (per frame), or [rows, C] for the lifter (H = rows, W = 1)
    int buf = -1;
    int H = 0, W = 0, C = 0;
};

// nn.BatchNorm2d (eval): weight, bias, running_mean, running_var as parameter indices
struct BnRef { int g = -1, b = -1, m = -1, v = -1; };

// A private packed copy derived from borrowed parameters (rebuilt by capf_params_changed): one primary layout and, per flag below, further
// copies of the same weights for the kernels that want them laid out differently.  Every copy has its own offset (elements inside the pack
// arena) and, where its rows are padded, its own padded K; Engine::build lays them out, Engine::repack fills them, gemm_args hands them out
enum PackKind { CONV_BN = 0, LINEAR = 1 };   // conv with its eval BatchNorm folded in | nn.Linear (possibly several concatenated along N)
struct Pack {
    PackKind kind = CONV_BN;
    int w[4] = {-1, -1, -1, -1}, b[4] = {-1, -1, -1, -1};   // param indices (linear: up to 4 concatenated)
    int n_lin = 0;
    BnRef bn;
    int N = 0, K = 0, Cin = 0, ks = 1;
    int n_src = 0;                 // conv: rows the parameter and its BatchNorm have when that is fewer than N (0: N) -- the pack's rows n_src .. N - 1 are
                                   // zero weights with a zero folded bias (CPN's final_predict.1: 17 rows packed as 20); such a pack keeps the primary layout alone
    // ---- the primary layout: [N][Kpad] at w_off, the folded bias (conv) or the concatenated biases (linear) at b_off
    size_t w_off = 0, b_off = 0;
    int Kpad = 0;
    bool in_place = false;         // linear with Kpad == K and no concat: no copy at all, the kernels read the parameter itself
    bool bf16 = false;             // ... stored as bf16 (Kpad % 64 == 0): conv weights, or a linear for the bf16 MFMA projections
    bool quad = false;             // ... a linear for the fused lifter kernels: Wq[k / 4][n][4] (lanes n read consecutive 16-byte quads)
    bool fast3x3 = false;          // a 3x3 / stride-1 fp32 conv with routes besides the direct kernel (Engine::conv_bn has the rule): the primary layout is
                                   // the Winograd one of igemm_wino.hip (Kpad = 12 * Cin for F(2,3), 18 * Cin for F(4,3)), the direct layout is a further copy
    bool wino_skip = false;        // ... and no batch up to cfg.max_batch reaches a Winograd kernel (a split-fp32 tile takes the conv from its first Winograd
                                   // batch to max_batch): the Winograd layout is not packed and has no arena space (build())
    // ---- the further copies: flag, offset, padded K
    size_t direct_off = 0; int direct_Kpad = 0;                  // fast3x3: the direct kernel's layout [N][direct_Kpad] as well (small batches run the direct kernel)
    bool rh = false; size_t rh_off = 0; int rh_Kpad = 0;         // bf16 3x3 stride-1 conv: the row-halo layout, [N][rh_Kpad = 9 * Cin] bf16 (igemm_bf16.hip)
    bool ws = false; size_t ws_off = 0;                          // bf16 3x3 stride-1 conv: the 2-D halo tile's layout (igemm_bf16_ws.hip), run at the
                                                                 // batches [Op::tile_lo, Op::tile_hi]
    bool x3 = false; size_t x3_off = 0;                          // fast3x3: what the plan's split-fp32 tile takes -- two block-scaled fp16 pieces
                                                                 // (igemm_f32h2_ws.hip; Engine::plan.x3_h2) or three bf16 pieces (igemm_f32x3_ws.hip)
    bool h2g = false; size_t h2g_off = 0; int h2g_Kpad = 0;      // fp32 conv / linear: two block-scaled fp16 pieces for igemm_f32h2.hip, [N][h2g_Kpad] floats +
                                                                 // [N] inverse channel scales; h2g_Kpad = the direct fp32 layout's padded K
    bool chain = false; size_t chain_off = 0;                    // ... and that copy once more in MFMA fragment order for lifter_chain.hip (launch_res_chain_repack)
    bool raw = false;              // an entry of Engine::raw_packs: the same conv WITHOUT its BatchNorm folded in (scale 1, bias 0), in the same layouts
};

// One conv -> BatchNorm (-> + residual) (-> ReLU) unit of the batch-statistics route (CAPF_PLAN_BN_BATCH_STATS): the plan's conv op, run raw
// (Engine::raw_packs, no bias, no residual, no activation), the statistics of its output, and the normalise / residual / ReLU pass over it
struct BnUnit { int op = -1; BnRef bn; };

// The lifter's layers (pose_dformer.py:144-241), resolved once where build_lifter registers the schema: parameter indices and shapes.
// The ONE place the layer list lives -- the plan (plan.cpp) and the training step (train.cpp) read it, neither builds a parameter name
struct LinearRef { int w = -1, b = -1, N = 0, K = 0; };   // nn.Linear: weight [N][K], bias [N]
struct LnRef { int w = -1, b = -1; };                      // nn.LayerNorm
struct LifterMlp { LnRef norm2; LinearRef fc1, fc2; };    // the MLP half of any block: x + fc2(gelu(fc1(norm2(x))))
struct LifterAtt { LnRef norm1; LinearRef qkv, proj; LifterMlp mlp; };
struct LifterCtx {
    LnRef norm1;
    LinearRef aw, so, embed_proj[4];     // attention_weights, sampling_offsets, embed_proj.l
    LifterMlp mlp;
    int ao_pack = -1;                    // pack of [attention_weights | sampling_offsets] in the row layout (the training step's GEMMs)
    int tap_pos = -1, tap_idx = -1;      // debug tap buffers (sampling positions, NW corner indices)
};
struct LifterSchema {
    int pos = -1;                        // Spatial_pos_embed
    LinearRef coord, feat_embed[4];
    LifterAtt res[8], joint[8];          // (depth <= 8 of each)
    LifterCtx ctx[4];                    // (levels of them; none with context_blocks = 0)
    LnRef head_ln;
    LinearRef head;
};

enum OpKind {
    OP_GEMM = 0, OP_FUSE, OP_MAXPOOL, OP_RESIZE, OP_PREP_EMBED, OP_SAMPLE_REF, OP_LAYERNORM, OP_DEFORM,
    OP_ATTENTION, OP_HEAD, OP_FORK, OP_JOIN, OP_EMBED, OP_CTX_ATTN, OP_RES_CHAIN, OP_MLP_CHAIN,
    OP_CONCAT            // in[0..n_in) [B, H, W, C] each -> out [B, H, W, n_in * C], channels in input order (CAPF_PLAN_CPN_PREDICT: torch.cat(refine_fms, 1))
};

// Per-kind payloads of an Op, held by value (an op of another kind leaves them at their defaults)
struct Fork { int lanes = 0, first_event = 0; };                    // OP_FORK / OP_JOIN: lanes of the region, first of its event ids
struct Sampler { int J = 0, L = 0, L1 = 0, NH = 0, NS = 0; };       // the lifter's samplers: joints, levels, L + 1 tokens, deform heads / samples
struct Attn { int groups = 0, tokens = 0, heads = 0, head_dim = 0; };   // OP_ATTENTION (groups per frame); OP_RES_CHAIN: tokens and heads
struct ChainBlock { int qkv = -1, proj = -1, fc1 = -1, fc2 = -1; LnRef norm1, norm2; };   // packs and LayerNorms of one block (lifter_chain.hip)

struct Op {
    OpKind kind = OP_GEMM;
    std::string name;
    // buffers (ids; -1 unused; -2 = external "images" input)
    int in[4] = {-1, -1, -1, -1};
    int aux = -1;                 // residual / rows added (GEMM, resize, LayerNorm); OP_DEFORM: the attention / offset rows.  An input
    int up_in = -1, up_H = 0, up_W = 0;   // OP_GEMM conv: the low-resolution map added, upsampled, behind the activation, and its size (build_cpn)
    int out = -1;
    int idx_out = -1;             // OP_SAMPLE_REF: the corner-index rows, a second output
    int outs[4] = {-1, -1, -1, -1};       // per-level outputs: OP_EMBED sampled rows, OP_DEFORM / OP_CTX_ATTN sample sums U
    // What the op reads and writes, slot by slot (-1: unused) -- the ONE list behind schedule_regions, plan_f32_stream, capf_op_schedule and
    // capf_op_tensor.  Not listed: the debug taps (tap_pos / tap_idx, written by a debug run only) and OP_EMBED's idx_lvl rows -- named
    // tensors that live to the end of the forward in memory of their own, which no op reads
    std::array<int, 6> reads() const { return {in[0], in[1], in[2], in[3], aux, up_in}; }
    std::array<int, 7> writes() const { return {out, idx_out, outs[0], outs[1], outs[2], outs[3], sh}; }
    // gemm
    int pack = -1;                // (OP_CTX_ATTN: the quad pack of [attention_weights | sampling_offsets])
    int conv = 0, Cin = 0, H = 0, W = 0, Ho = 0, Wo = 0, ks = 1, stride = 1, pad = 0;
    long rows_per_frame = 0;      // M = rows_per_frame * batch
    int N = 0, K = 0, act = 0;
    RowMap amap{1, 0, 0, 0}, omap{1, 0, 0, 0}, rmap{1, 0, 0, 0};
    int res_param = -1;           // residual read from a parameter (pos-embed) instead of a buffer
    // fuse / resize / pool
    int n_in = 0, shift[4] = {0, 0, 0, 0}, relu = 0, C = 0;
    bool debug_only = false;      // OP_FUSE as a plain copy into a named tensor: runs under capf_set_debug only (Engine::skipped)
    Fork fork;
    // lifter
    LnRef ln;                     // the LayerNorm this op applies, eps in `eps`: OP_LAYERNORM, OP_CTX_ATTN (norm1), OP_HEAD, and an OP_GEMM in rows
                                  // mode that normalises its A rows on the fly
    float eps = 0.f;
    Sampler smp;                  // OP_EMBED, OP_PREP_EMBED, OP_SAMPLE_REF, OP_DEFORM, OP_CTX_ATTN (each sets what its kernel takes)
    LinearRef coord;              // OP_EMBED / OP_PREP_EMBED: coord_embed ...
    int pos = -1;                 // ... and Spatial_pos_embed
    LinearRef head;               // OP_HEAD: the head's linear (head.N output columns)
    Attn attn;
    std::vector<ChainBlock> blocks;   // OP_RES_CHAIN: its blocks; OP_MLP_CHAIN: one entry {fc1, fc2, norm2}, rows through amap
    int lvlH[4] = {0, 0, 0, 0}, lvlW[4] = {0, 0, 0, 0}, lvlC[4] = {0, 0, 0, 0};
    int idx_lvl[4] = {-1, -1, -1, -1};       // OP_EMBED: corner-index rows per level
    int tap_pos = -1, tap_idx = -1;          // OP_DEFORM / OP_CTX_ATTN: debug taps of the sampling site (positions as floats, NW corner indices)
    int pq[4] = {-1, -1, -1, -1};   // per-level quad-interleaved packs (OP_EMBED feat_embed, OP_CTX_ATTN embed_proj) ...
    int pb[4] = {-1, -1, -1, -1};   // ... and their bias parameters
    double flops_per_frame = 0.0;
    int bf16 = 0;                 // tensors of this op are bf16 (conv: bf16 MFMA kernel)
    int fast3x3 = 0;              // 3x3 stride-1 fp32 conv with routes besides the direct kernel (Pack::fast3x3): the split-fp32 tile at the batches
                                  // [tile_lo, tile_hi], a Winograd kernel from plan.wino_min_batch (Engine::gemm_family)
    int pw_pair = 0;              // one of a 64 -> 256 / 256 -> 64 pointwise pair that igemm_f32_pwchain.hip can run as one launch: stays on the fp32
                                  // kernels in every plan (the chained and the two-launch routes are bit-identical; test_pointwise_chain_*)
    int tile_lo = 0, tile_hi = -1;   // batches [tile_lo, tile_hi] at which this 3x3 stride-1 conv runs its plan's halo tile -- the 2-D halo tile of a 16-bit
                                  // conv (Pack::ws), the split-fp32 tile of a fast3x3 one (Pack::x3) -- (Engine::tile_takes; set by build(), empty = never)
    int out_bf16 = 0;             // fp32 stem conv writing bf16 activations
    int h2_exps = -1, h2_role = 0, h2_peer = -1;   // a BasicBlock's conv1 (role 1: writes planes + exponents to buffer h2_exps) / conv2 (role 2: reads them);
                                  // h2_peer = the other op's index: both must run the two-fp16-piece tile at a batch for the pair to use planes
    long h2_utab = -1;            // two-fp16-piece conv tile: word offset of this conv's map geometry in the engine's unit tables (-1: none)
    // CAPF_PLAN_BF16_F32_STREAM (Engine::plan_f32_stream): f32s = a bf16 conv with the fp32-stream epilogue (its residual, if any, is fp32);
    // st_f32 = the output is stored fp32 (conv or fuse sum); sh = buffer of its bf16 shadow, what the convs that read it take as operand (-1: none)
    int f32s = 0, st_f32 = 0, sh = -1;
    int feat_bf16 = 0;            // lifter samplers (embed, ctx_attn, sample_ref, deform_sample): how the context maps are stored -- 0 fp32, 1 bf16, 2 fp16
    int bneck_c3 = -1;            // conv1 / conv2 / downsample of a first bottleneck that may run as one kernel with its conv3 (that op's index; plan.cpp bneck0_mark)
    int lane = 0;                 // stream lane inside a fork/join region (0 = the caller's stream)
    int region = -1;              // index of the enclosing fork/join region, -1 outside
    int level = -1;               // dependency level inside the region (schedule_regions), -1 outside
};

struct NamedTensor {
    int buf;
    int64_t shape[4];   // shape[0] = -1 means "batch"
    int ndim;
    int is_int;
};

// float offsets inside the training region of the workspace (train.cpp :: Engine::train_layout)
struct TrainLayout {
    struct Mlp { size_t xh2, rs2, y2, hp, hg; };   // what the MLP half of a block keeps: LayerNorm x-hat / rstd / output, fc1 output, its GELU
    struct Ctx { size_t xh1, rs1, y1, ao, U[4]; Mlp mlp; };
    struct Att { size_t xh1, rs1, y1, qkv, o; Mlp mlp; };
    size_t X, S[4];
    Ctx ctx[4];                              // (one per context block: levels of them)
    Att res[8], joint[8];                    // (one per block of each group: depth <= 8 of them)
    size_t xhh, rsh, yh;
    size_t dX, gA, gB, gC, cat, dU[4], tA, tB, wT, slabs, red;
    size_t h2w, h2max;                       // the step's weights as two-fp16-piece packs (W and W^T: Engine::t_h2_specs), and their maxima scratch
    size_t wpad;                             // zero-padded [N][r32(K)] copies of the step's linears whose K (a context map's channel count) is no multiple of 32
    size_t slabs_elems = 0, red_elems = 0;   // capacities of the two scratch areas above (what the weight-gradient slicing may use)
    size_t red_cap = 0;                      // ... and one column reduction's partial sums of red_elems (the same arrangement: t_col_flush)
    size_t slab_cap = 0;                     // what ONE weight gradient's slabs may take of slabs_elems (the slab area holds several layers' slabs
                                             // until Engine::t_slab_flush sums them in one launch)
    size_t total;
};

// Per-launch event log of the product schedule (capf_forward_profile): launch k is bracketed by ev[k] and
// ev[k + 1]; leader[k] is the first op of the launch, op_leader[op] the leader of the launch an op rode in.
struct LaunchLog {
    std::vector<hipEvent_t> ev;
    std::vector<int> leader;
    std::vector<int> op_leader;
    std::vector<int> op_variant;       // per leader op: which device kernel a grouped 16-bit launch ran -- 0 / 1 / 2 as launch_gemm_bf16_group chose
                                       // (kernels.h), 3 the 2-D halo tile (a BF16_TILE launch) --, -1 otherwise
    hipError_t mark(hipStream_t s, const int* members, int n) {
        hipEvent_t e;
        hipError_t r = hipEventCreate(&e);
        if (r != hipSuccess) return r;
        ev.push_back(e);
        if (n > 0) {
            leader.push_back(members[0]);
            for (int i = 0; i < n; ++i) op_leader[members[i]] = members[0];
        }
        return hipEventRecord(e, s);
    }
    ~LaunchLog() {
        for (hipEvent_t e : ev) (void)hipEventDestroy(e);
    }
};

// Where a run's stem reads the image: nowhere (a lifter-only call, capf_set_features), an fp32 NHWC tensor, or a uint8 BGR crop
using ImageSource = std::variant<std::monostate, const float*, U8Input>;

// What a call leaves behind for the next one.  Engine::begin writes it, in one place and only after every check of the call has passed;
// the other writers are the mutators below, the training step (train_batch, t_h2_base: train.cpp) and capf_forward_profile_launches
// (last_variants), all behind a begin() that passed -- a refused call changes nothing here
struct Session {
    ImageSource image;
    const float* k2d = nullptr;          // the lifter's pointers (null behind a call that ran no lifter op)
    float* kcrop = nullptr;
    float* out = nullptr;
    int last_batch = 0;                  // batch of the tensors capf_tensor / capf_op_tensor hand out
    int feat_batch = 0;                  // batch of the context maps feat0..3 in the workspace (a whole backbone run or capf_set_features; 0: none)
    int train_batch = 0;                 // batch of the forward_train whose activations are still in the workspace (0: none)
    int64_t train_generation = 0;        // bumped by every run that (over)writes the workspace
    float* t_h2_base = nullptr;          // the saved step's W / W^T packs (set by t_h2_prepare; nullptr: the step runs on the fp32 matrix pipe)
    std::vector<int> last_variants;      // capf_forward_profile_launches: grouped-bf16 kernel variant per leader op

    const float* images() const { const auto* p = std::get_if<const float*>(&image); return p ? *p : nullptr; }
    const U8Input* u8() const { return std::get_if<U8Input>(&image); }
    void invalidate_train() { train_batch = 0; ++train_generation; t_h2_base = nullptr; }    // the workspace is about to be (over)written
    void drop_maps() { invalidate_train(); feat_batch = 0; }                                   // ... its context maps included
    void maps_written(int batch) { feat_batch = batch; }     // the end of run() and of capf_set_features (0: a prefix run left them half written)
};

// One call of a run entry as begin() sees it
struct Call {
    const char* who;                     // the entry's name, as the messages spell it
    ImageSource image;
    const float* k2d; float* kcrop; float* out;      // the lifter's pointers (all null: the call runs no lifter op)
    int batch;
    int first, last;                     // the op span [first, last) it runs
    bool training = false;               // the training step's lifter forward follows the span: refused by a handle created with training = 0
    bool maps = false;                   // reads context maps of this batch that an earlier call left (otherwise it writes the maps itself)
    bool bn = false;                     // the backbone span runs the batch-statistics route (capf_backbone_forward_bn) ...
    float momentum = 0.1f;               // ... moving the running statistics with this momentum
};

struct Engine {
    Engine() = default;
    Engine(const Engine&) = delete;
    capf_config cfg{};
    int device = -1;
    std::string err;

    // ---- plan switches: what cfg.plan_flags (and, in the diagnostic build, the CAPF_* knobs of diag_env) chose.  Set once by
    // set_plan_switches() before anything is planned; constant afterwards
    struct PlanSwitches {
        bool fused_lifter = true;      // fused embed / context-attention kernels + LayerNorm folded into the GEMMs (CAPF_PLAN_NO_FUSED_LIFTER, CAPF_LIFTER_FUSED=0:
                                       // the one-kernel-per-op plan, for A/B runs)
        bool use_wino = true;          // the eligible 3x3 stride-1 fp32 convs are fast3x3 (CAPF_PLAN_NO_WINOGRAD, CAPF_WINO=0: none is, the direct kernel
                                       // everywhere -- no split-fp32 tile either: Engine::conv_bn)
        bool wino_f43 = true;          // F(4,3) where W % 4 == 0, F(2,3) for the other even widths (CAPF_PLAN_WINOGRAD_F23_ONLY, CAPF_WINO_F43=0: F(2,3) everywhere)
        bool wino_f43_cpn = false;
        int wino_f43_min_hw = 0, wino_f43_max_hw = 1 << 30;   // F(4,3) only for maps with min <= H * W <= max pixels
        int wino_min_batch = 24;       // below this batch the fast3x3 convs the split-fp32 tile does not take run the direct kernel (with
                                       // split-K; batch 16: 4.75 vs 5.86 ms per forward, batch 24: 6.08 vs 6.37)
        bool use_rh = true;            // row-halo layout + kernel for the bf16 3x3 stride-1 convs (CAPF_PLAN_NO_ROW_HALO, CAPF_BF16_RH=0: off, A/B runs)
        bool use_ws = true;            // 2-D halo layout + kernel for the bf16 3x3 stride-1 convs (CAPF_PLAN_NO_WS clears it)
        bool use_x3 = true;            // split-fp32 tile for the fast3x3 convs (CAPF_PLAN_NO_F32X3 clears it)
        bool x3_h2 = true;             // ... the two-fp16-piece tile (three piece products per MAC); CAPF_PLAN_F32X3_EXACT: the three-bf16-piece tile (six)
        bool use_h2g = true;           // every other fp32 conv / linear of an inference batch >= 5 on the two-fp16-piece GEMM (igemm_f32h2.hip;
                                       // CAPF_PLAN_NO_F32H2_GEMM clears it)
        bool use_h2_planes = false;    // CAPF_PLAN_H2_PLANES sets it (opt-in: measured slower, EXPERIMENTS R6.5)
        bool use_pwchain = true;       // CAPF_PLAN_NO_PWCHAIN clears it
        bool use_bneck = true;         // CAPF_PLAN_NO_BNECK clears it
        bool use_upadd = true;         // CAPF_PLAN_NO_UPADD clears it (CPN bf16: lateral conv + upsampled add in one launch)
        bool batch_reduce = true;      // CAPF_PLAN_NO_BATCHED_REDUCE clears it: the backward's second-stage reductions one launch each
        bool f32_stream = false;       // CAPF_PLAN_BF16_F32_STREAM: bf16 only as conv operands, every other backbone tensor fp32
        bool bn_batch = false;         // CAPF_PLAN_BN_BATCH_STATS: the handle also carries the batch-statistics route of the backbone (bn_units)
    } plan;
    bool set_plan_switches();
    static constexpr int H2G_MIN_BATCH = 5;

    // ---- schema / plan data (plan.cpp)
    std::vector<Param> params;
    std::map<std::string, int> param_index;
    std::vector<Buffer> bufs;
    std::vector<Pack> packs;
    std::vector<Op> ops;
    // The batch-statistics route (capf_backbone_forward_bn; empty without CAPF_PLAN_BN_BATCH_STATS): the backbone's second op list.  It walks the
    // plan's backbone ops, with every conv replaced by its BnUnit -- so the raw convs keep the kernel family and the grouped launch per level that
    // the plan routes their geometry and batch to -- and without the launches that cross a BatchNorm (fused_at: none; no planes between convs).
    // raw_packs[i] is packs[i] unfolded (conv packs only), at offsets of its own behind the plan's packs; bn_unit_of[op] indexes bn_units (-1)
    std::vector<BnUnit> bn_units;
    std::vector<int> bn_unit_of;
    std::vector<Pack> raw_packs;
    bool bn_run = false;                 // a capf_backbone_forward_bn is being enqueued: gemm_args / fused_at / exec_op describe the second list
    float bn_momentum = 0.1f;
    int n_backbone_ops = 0;
    int stem_op = -1;              // the one conv that reads the image (-1: none, -2: several)
    int cur_lane = 0, cur_region = -1, n_regions = 0, n_events = 0;
    std::vector<std::pair<int, int>> regions;   // [fork op, join op]
    std::vector<std::vector<std::vector<int>>> region_levels;   // per region: dependency levels -> op indices
    std::map<std::string, NamedTensor> named;
    size_t ws_elems_per_frame = 0;
    size_t pack_elems = 0;
    size_t bias_tab_off = 0;       // inside the arena: the CopySegment table of the packed linears' bias vectors (launch_copy_segments)
    bool has_res_chain = false;    // the plan holds an OP_RES_CHAIN (lifter_chain.hip): its two-piece packs are needed at every batch
    std::vector<unsigned> utab_host;     // the unit tables of the two-fp16-piece conv tile, one per map geometry (H, W, Cin) of the plan (build())
    size_t utab_off = 0;                 // ... and their place in the pack arena (uploaded once: they depend on the plan alone)
    int batch_limit = 0;                 // largest batch the 32-bit tensor addressing of the kernels allows (build())
    int feat_buf[4] = {-1, -1, -1, -1}, feat_H[4] = {0, 0, 0, 0}, feat_W[4] = {0, 0, 0, 0}, feat_C[4] = {0, 0, 0, 0};
    LifterSchema lifter;                 // the lifter's layers as parameter indices (filled by build_lifter)
    std::vector<long> grad_off;          // per parameter: offset in the flat lifter gradient, -1 for the backbone
    long grad_elems = 0;

    int add_param(const std::string& name, int kind, std::initializer_list<int64_t> shape);
    int new_buffer(size_t elems, const std::string& tag);
    Tensor conv_bn(const std::string& conv, const std::string& bn, const Tensor& x, int Cout, int ks, int stride,
                   int act, const Tensor* residual, int pad_rows_to = 0);
    void build_hrnet(Tensor img, Tensor feats[4]);
    void build_cpn(Tensor img, Tensor feats[4]);
    void build_lifter(const Tensor feats[4]);
    bool build();
    void assign_offsets();
    void schedule_regions();
    bool b16() const { return cfg.compute_dtype == CAPF_BF16 || cfg.compute_dtype == CAPF_F16; }   // a 16-bit plan: one op list, one set of routing rules ...
    bool f16() const { return cfg.compute_dtype == CAPF_F16; }   // ... and the element format of its 16-bit kernels, tensors and packs (GemmArgs::f16)
    int dt16() const { return f16() ? 3 : 2; }                    // capf_tensor's code of a 16-bit tensor of this plan (2 bf16, 3 fp16)
    bool maps_bf16() const { return b16() && !plan.f32_stream; }   // the context maps feat0..3 are stored 16-bit
    int feat_fmt() const { return maps_bf16() ? 1 + (int)f16() : 0; }   // ... as the samplers take it: 0 fp32, 1 bf16, 2 fp16
    int depth() const { return cfg.depth > 0 ? cfg.depth : cfg.levels; }   // blocks per group (res_blocks / joint_blocks)
    bool plan_f32_stream(const Tensor feats[4]);
    size_t act_elems(size_t n) const { return b16() ? (n + 1) / 2 : n; }   // backbone activation size in float slots
    void use(int buf);   // mark buffer as read by the op being appended
    void push(Op op);    // append an op, tagging it with the current lane / region
    void fork(int n);    // open a region of n independent lanes (independent branches run on side streams)
    void set_lane(int l) { cur_lane = l; }
    void join();

    // ---- device state
    float* pack_arena = nullptr;   // device, owned
    std::vector<CopySegment> bias_tab;   // host image of the table at bias_tab_off (kept alive for the asynchronous upload); rebuilt by every full repack
    bool bias_tab_on_device = false;
    bool utab_on_device = false;
    float* split_ws = nullptr;     // device, owned: split-K slabs + per-tile counters of the small-batch conv launches
    int* split_cnt = nullptr;
    // the two-chain schedule (lanes == 3) runs two grouped chains CONCURRENTLY: the side chain's split-K convs get slabs and
    // counters of their own (a conv splits or not by its shape alone, so both chains may hold splitting convs at once)
    float* split_ws_side = nullptr;
    int* split_cnt_side = nullptr;
    static constexpr long SPLIT_WS_ELEMS = 4L << 20;
    static constexpr int SPLIT_CNT_ELEMS = 16384;
    float* ws = nullptr;           // device, borrowed
    size_t ws_bytes = 0;
    bool packed = false;
    bool h2g_lifter_dirty = true;  // the linear packs' two-piece copies are stale (parameters changed since they were packed)
    bool debug = false;            // run the debug-copy ops (capf_set_debug)
    int lanes = 3;                 // fork/join regions: 0 in program order, 1 one side stream per lane, 2 grouped launches on one stream,
                                   // 3 grouped launches as two chains on two streams (capf_set_lanes)
    int map_grad_mode = 0;         // dfeat of capf_backward_maps: 0 fp32 atomic adds, 1 the ordered sum (capf_set_map_grad_mode)
    hipStream_t side[3] = {nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> events;
    Session ses;                   // what the last call left behind (begin())
    ~Engine();                     // the ONE release path of the device resources above (capf_destroy, and capf_create where it fails half-way)

    // ---- execution (engine.cpp)
    float* bptr(int buf, int batch) const { return ws + bufs[buf].offset * (size_t)batch; }
    struct ConvSrc { const float *w, *g, *b, *m, *v; float eps; };   // what every conv packer folds: the weight and its BatchNorm (eval, eps 1e-5)
    ConvSrc conv_src(const Pack& pk) const;
    int repack(hipStream_t s, bool lifter_only = false);
    int ensure_h2g_lifter(hipStream_t s);
    size_t workspace_bytes(int batch) const {
        const size_t plain = ws_elems_per_frame * (size_t)batch + (cfg.training ? train_elems(batch) : 0);
        return (plan.bn_batch ? bn_base(batch) + BN_SLOTS * bn_slot_elems(batch) : plain) * sizeof(float);
    }
    // scratch of the batch-statistics route, behind the training region: BN_SLOTS slots (one per BatchNorm of a grouped launch; everything runs
    // on the caller's stream, so the next launch group reuses them), each {slab partials | scale | shift} of the plan's largest unit
    static constexpr int BN_SLOTS = 4;
    size_t bn_base(int batch) const { return (ws_elems_per_frame * (size_t)batch + (cfg.training ? train_elems(batch) : 0) + 63) / 64 * 64; }
    size_t bn_slot_elems(int batch) const;
    int bn_post(hipStream_t s, int batch, const int* members, int n);    // statistics + apply behind the raw convs `members` (ops; others skipped)
    int check_run(int batch);      // can this handle run this batch at all: a device, the batch range, fresh packs, a workspace that holds it
    int begin(const Call& c);      // every precondition of a run entry, then -- all passed -- the session state of the call
    int run(hipStream_t s, int batch, int first_op, int last_op, hipEvent_t* ev = nullptr, LaunchLog* log = nullptr);
    int exec_op(const Op& op, hipStream_t s, int batch, bool side_chain = false);
    bool skipped(const Op& op) const { return op.debug_only && !debug; }   // a debug copy outside a debug run: no launch, no log entry
    FuseSumArgs fuse_args(const Op& op, int batch) const;
    // ---- launch routes: pure functions of (op, batch) and the plan (no cache, no mutable state -- const-handle queries on other threads may ask
    // while a forward is being enqueued).  Which family's launcher runs a GEMM op (exec_op; run_region_grouped's pass that may group it), and
    // what the op reports: the kernel that runs it on its own (capf_op_info) and the FLOPs that kernel issues (capf_op_executed_flops).
    // A fast3x3 conv is F32_TILE (the plan's split-fp32 tile: igemm_f32h2_ws.hip, or igemm_f32x3_ws.hip under CAPF_PLAN_F32X3_EXACT) at the
    // batches build() found the tile to take it, WINO (igemm_wino.hip) at the other batches from plan.wino_min_batch where its Winograd
    // layout is packed, F32 (the direct kernel on the direct layout) below.  A 16-bit conv is BF16_TILE (the 2-D halo tile, igemm_bf16_ws.hip)
    // at the batches build() found that tile to take it, BF16 (igemm_bf16.hip) at every other: which of that file's kernels is the launcher's
    // choice, by the tile count of the whole launch.  gemm_family is THE decision: the launchers only check it
    enum class Family { NONE = -1, F32, BF16, BF16_TILE, F32_TILE, WINO, BF16_ROWS };
    struct OpRoute { Family family; const char* kernel; double flops; };
    bool tile_takes(const Op& op, int batch) const;          // build()'s question behind [tile_lo, tile_hi]: the size rule and the tile launcher's own test
    Family gemm_family(const Op& op, int batch) const;
    hipError_t launch_f32_tile(const GemmArgs* list, int n, hipStream_t s) const {      // the F32_TILE problems of one launch, on the plan's tile
        return (plan.x3_h2 ? launch_gemm_f32h2_group : launch_gemm_f32x3_group)(list, n, s);
    }
    OpRoute op_route(const Op& op, int batch) const;
    // Several ops as ONE launch: a first bottleneck (bneck_bf16.hip; at its fork op, m = {conv1, conv2, downsample, conv3}), an identity
    // bottleneck (256 -> 64 -> 64 -> 256, y = relu(conv3 + x); m = {conv1, conv2, conv3}), a 64 -> 256 / 256 -> 64 pointwise conv pair
    // (igemm_*_pwchain.hip; m = {a, b}).  fused_at: the launch that starts at op i in a run ending before last_op (n = 0: none; bneck_only:
    // bottlenecks alone).  fused_leader: the launch op i rides in in a whole forward (its leader is m[0])
    enum class Fusion { NONE, BNECK0, BNECK1, PWCHAIN };
    struct FusedLaunch { Fusion kind = Fusion::NONE; int n = 0; int m[4] = {-1, -1, -1, -1}; };
    FusedLaunch fused_at(int i, int batch, int last_op, bool bneck_only = false) const;
    FusedLaunch fused_leader(int i, int batch, bool bneck_only = false) const;
    // side_chain: the launches belong to the second of two concurrent chains and take its split-K scratch (default: the main chain's, which
    // is what every query about an op sees)
    int run_region_grouped(hipStream_t s, int batch, int region, LaunchLog* log, unsigned lane_mask = ~0u, bool side_chain = false);
    // lanes == 3 runs the region behind this fork op as two chains at this batch (on a device: run())
    bool two_chains(const Op& fork_op, int batch) const { return lanes == 3 && fork_op.fork.lanes >= 2 && batch >= 16 && batch <= 128; }
    GemmArgs gemm_args(const Op& op, int batch, bool planes = true, bool side_chain = false) const;

    // ---- training step (train.cpp)
    void train_layout(int B, TrainLayout& L) const;
    size_t train_elems(int B) const;
    int forward_train(hipStream_t s, int B, const float* masks);
    int backward(hipStream_t s, int B, const float* dOut, float* flat_grad, const float* masks, float* const* dfeat = nullptr,
                 float* dk2d = nullptr, float* dref = nullptr);
    int t_gemm(hipStream_t s, const float* A, RowMap amap, int M, int N, int K, const float* W, int Kpad, const float* bias,
               float* out, RowMap omap, const float* res, RowMap rmap, int act, const float* rscale, int rs_div, const float* Wh2 = nullptr);
    // The lifter's linears on the two-fp16-piece GEMM during a training step (forward: y = x W^T, backward: dX = dY W): which matrices,
    // where their packs sit in the training region (offsets from TrainLayout::h2w), and the table the pack launch reads (kernels.h)
    struct H2TrainSpec { int param, pack; int N, K, ld; bool fwd, bwd; };   // source: parameter `param`, or (param < 0) the row pack `pack`
    std::vector<H2TrainSpec> t_h2_specs;
    std::vector<H2TrainW> t_h2_tab;      // host image of the device table (offsets filled by t_h2_plan, pointers by t_h2_prepare)
    std::map<const float*, int> t_h2_index;
    size_t t_h2_tab_off = 0;             // inside the pack arena
    size_t t_h2_elems = 0, t_h2_max_elems = 0;
    int t_h2_tiles = 0;
    bool t_h2_on_device = false;
    // weight-gradient slabs waiting for their sum (backward): the slab area is a bump allocator, the sums run as ONE launch when it is
    // full, when SLAB_BATCH_MAX jobs wait, and at the end of backward -- 64 slab_sum launches per step -> a handful
    SlabBatch t_slab_jobs{};
    size_t t_slab_cur = 0;
    float* t_slab_take(hipStream_t s, float* area, size_t cap, size_t elems, int* rc);
    int t_slab_defer(hipStream_t s, const float* slabs, int nslab, long n, float* dst);
    int t_slab_flush(hipStream_t s);
    // the same for the second stages of the backward's column reductions (bias / LayerNorm gradients): 32 launches per step -> one or two
    ColFinalBatch t_col_jobs{};
    size_t t_col_cur = 0;
    int t_colreduce(hipStream_t s, const TrainLayout& L, float* tw, const float* A, RowMap amap, const float* Bm, RowMap bmap, int bmode,
                    int rows, int C, float* dst, long dst_stride, float* dst2, size_t cap_elems);
    int t_col_flush(hipStream_t s);
    void t_h2_plan();
    int t_h2_prepare(hipStream_t s, const TrainLayout& L, float* tw, int B);
    const float* t_h2_pack(const float* W, bool transposed) const;
    int t_linear_bwd(hipStream_t s, const TrainLayout& L, float* tw, const float* dY, RowMap dymap, int rows, int N, int K,
                     const float* Xin, RowMap xmap, const float* W, float* dX, RowMap dxmap, bool acc_dx, float* gW, float* gb);
};

}  // namespace capf

struct capf_handle {
    capf::Engine e;
};
