// Executor + C ABI (include/capf.h).  Walks the static plan and enqueues the gfx950 kernels on the
// caller's stream; no allocation, no synchronisation, no host round trip inside capf_forward.
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "engine.h"

namespace capf {

#define HIP_TRY(expr)                                                                      \
    do {                                                                                   \
        hipError_t _e = (expr);                                                            \
        if (_e != hipSuccess) {                                                            \
            err = std::string(#expr) + ": " + hipGetErrorString(_e);                       \
            return CAPF_ERR_HIP;                                                           \
        }                                                                                  \
    } while (0)

Engine::ConvSrc Engine::conv_src(const Pack& pk) const {
    if (pk.raw) return {params[pk.w[0]].ptr, nullptr, nullptr, nullptr, nullptr, 1e-5f};     // (no BatchNorm: the packers fold scale 1, bias 0)
    return {params[pk.w[0]].ptr, params[pk.bn.g].ptr, params[pk.bn.b].ptr, params[pk.bn.m].ptr, params[pk.bn.v].ptr, 1e-5f};
}

// Rebuild the private packed copies from the borrowed parameters.
int Engine::repack(hipStream_t s, bool lifter_only) {
    for (const Param& p : params) {
        if (p.kind == CAPF_P_BN_NBT) continue;
        if (!p.ptr) {
            err = "parameter not set: " + p.name;
            return CAPF_ERR_STATE;
        }
    }
    if (!utab_on_device && !utab_host.empty()) {        // the conv tile's unit tables: a function of the plan, uploaded once (synchronous: a pageable source)
        HIP_TRY(hipMemcpy(pack_arena + utab_off, utab_host.data(), utab_host.size() * sizeof(unsigned), hipMemcpyHostToDevice));
        utab_on_device = true;
    }
    for (const std::vector<Pack>* list : {&packs, &raw_packs})       // (raw_packs: the batch-statistics route's unfolded copies of the conv packs)
        for (const Pack& pk : *list) {                  // the convs' two-fp16-piece copies (igemm_f32h2.hip); the linears' are packed lazily
            if (!pk.h2g || pk.kind != CONV_BN || lifter_only || (list == &raw_packs && !pk.raw)) continue;
            const ConvSrc c = conv_src(pk);
            HIP_TRY(launch_pack_f32h2_gemm(c.w, c.g, c.b, c.m, c.v, c.eps, pack_arena + pk.h2g_off, nullptr, pk.N, pk.Cin, pk.ks, pk.K, pk.h2g_Kpad, s));
        }
    h2g_lifter_dirty = true;
    std::vector<CopySegment> jobs;                      // the packed linears' bias vectors: one launch for all of them (below)
    for (const std::vector<Pack>* list : {&packs, &raw_packs})
    for (const Pack& pk : *list) {
        if (pk.in_place || (list == &raw_packs && !pk.raw)) continue;
        float* W = pack_arena + pk.w_off;
        float* B = pack_arena + pk.b_off;
        if (pk.kind == CONV_BN) {
            if (lifter_only) continue;                  // conv+BN packs belong to the frozen backbone
            const ConvSrc c = conv_src(pk);
            if (pk.n_src) {                             // fewer parameter rows than pack rows: zeros first, then the parameter's rows of the primary layout
                HIP_TRY(hipMemsetAsync(W, 0, (size_t)pk.N * pk.Kpad * (pk.bf16 ? 2 : 4), s));
                HIP_TRY(hipMemsetAsync(B, 0, (size_t)pk.N * sizeof(float), s));
                if (pk.bf16) HIP_TRY(launch_pack_conv_bf16(c.w, c.g, c.b, c.m, c.v, c.eps, W, B, pk.n_src, pk.Cin, pk.ks, pk.Kpad, s, f16()));
                else HIP_TRY(launch_pack_conv(c.w, c.g, c.b, c.m, c.v, c.eps, W, B, pk.n_src, pk.Cin, pk.ks, pk.Kpad, s));
                continue;
            }
            if (pk.bf16) {
                HIP_TRY(launch_pack_conv_bf16(c.w, c.g, c.b, c.m, c.v, c.eps, W, B, pk.N, pk.Cin, pk.ks, pk.Kpad, s, f16()));
                if (pk.rh) HIP_TRY(launch_pack_conv_bf16_rh(c.w, c.g, c.b, c.m, c.v, c.eps, pack_arena + pk.rh_off, B, pk.N, pk.Cin, bf16_rh_width(pk.Cin), s, f16()));
                if (pk.ws) HIP_TRY(launch_pack_conv_bf16_ws(c.w, c.g, c.b, c.m, c.v, c.eps, pack_arena + pk.ws_off, B, pk.N, pk.Cin, s, f16()));
            } else if (pk.fast3x3) {
                if (!pk.wino_skip) HIP_TRY(launch_pack_conv_wino(c.w, c.g, c.b, c.m, c.v, c.eps, W, B, pk.N, pk.Cin, s, pk.Kpad == 18 * pk.Cin ? 43 : 23));
                HIP_TRY(launch_pack_conv(c.w, c.g, c.b, c.m, c.v, c.eps, pack_arena + pk.direct_off, B, pk.N, pk.Cin, pk.ks, pk.direct_Kpad, s));
                if (pk.x3)
                    HIP_TRY((plan.x3_h2 ? launch_pack_conv_f32h2 : launch_pack_conv_f32x3)(c.w, c.g, c.b, c.m, c.v, c.eps, pack_arena + pk.x3_off, B, pk.N, pk.Cin, s));
            } else {
                HIP_TRY(launch_pack_conv(c.w, c.g, c.b, c.m, c.v, c.eps, W, B, pk.N, pk.Cin, pk.ks, pk.Kpad, s));
            }
            continue;
        }
        int n0 = 0;                                     // linears, concatenated along N: each into its rows of the pack's layout
        for (int i = 0; i < pk.n_lin; ++i) {
            const int n = (int)params[pk.w[i]].shape[0];
            const float* w = params[pk.w[i]].ptr;
            if (pk.bf16)                                // bf16 [N][Kpad] (a 1x1 "conv" without BatchNorm), bias fp32
                HIP_TRY(launch_pack_conv_bf16(w, nullptr, nullptr, nullptr, nullptr, 0.f, reinterpret_cast<unsigned short*>(W) + (size_t)n0 * pk.Kpad,
                                              nullptr, n, pk.K, 1, pk.Kpad, s, f16()));
            else if (pk.quad) HIP_TRY(launch_pack_linear_quad(w, W, n, pk.K, n0, pk.N, s));     // fused lifter kernels: Wq[k / 4][n][4]
            else HIP_TRY(launch_pack_linear(w, W + (size_t)n0 * pk.Kpad, n, pk.K, pk.Kpad, s));
            jobs.push_back(CopySegment{params[pk.b[i]].ptr, B + n0, n, 0});
            n0 += n;
        }
    }
    if (!jobs.empty()) {
        CopySegment* tab_dev = reinterpret_cast<CopySegment*>(pack_arena + bias_tab_off);
        const bool same = bias_tab_on_device && bias_tab.size() == jobs.size() &&
                          memcmp(bias_tab.data(), jobs.data(), jobs.size() * sizeof(CopySegment)) == 0;
        if (!same) {                                    // (parameters moved or first pack: a per-step lifter repack finds the table in place)
            HIP_TRY(hipStreamSynchronize(s));           // an upload still reading the previous host image must not see it change
            bias_tab = jobs;
            HIP_TRY(hipMemcpyAsync(tab_dev, bias_tab.data(), bias_tab.size() * sizeof(CopySegment), hipMemcpyHostToDevice, s));
            bias_tab_on_device = true;
        }
        HIP_TRY(launch_copy_segments(tab_dev, (int)jobs.size(), s));
    }
    packed = true;
    return CAPF_OK;
}

// The lifter's linears as two fp16 pieces (igemm_f32h2.hip), rebuilt on the forward's stream when an inference forward of batch >= 5 finds
// them stale: several linears concatenated along N are packed on their own rows, the inverse scales of all rows follow the whole matrix
int Engine::ensure_h2g_lifter(hipStream_t s) {
    if (!h2g_lifter_dirty) return CAPF_OK;
    for (const Pack& pk : packs) {
        if (!pk.h2g || pk.kind != LINEAR) continue;
        int n0 = 0;
        for (int i = 0; i < pk.n_lin; ++i) {
            const int n = (int)params[pk.w[i]].shape[0];
            HIP_TRY(launch_pack_f32h2_gemm_rows(params[pk.w[i]].ptr, pack_arena + pk.h2g_off, n0, n, pk.N, pk.K, pk.h2g_Kpad, s));
            n0 += n;
        }
        if (pk.chain) HIP_TRY(launch_res_chain_repack(pack_arena + pk.h2g_off, pack_arena + pk.chain_off, pk.N, pk.h2g_Kpad, s));
    }
    h2g_lifter_dirty = false;
    return CAPF_OK;
}

GemmArgs Engine::gemm_args(const Op& op, int batch, bool planes, bool side_chain) const {
    auto ptr = [&](int buf) -> float* { return (buf >= 0 && ws) ? bptr(buf, batch) : nullptr; };
    const bool raw = bn_run && bn_unit_of[&op - ops.data()] >= 0;      // a raw conv of the batch-statistics route: unfolded weights, zero bias,
    const Pack& pk = raw ? raw_packs[op.pack] : packs[op.pack];      // no residual, no activation, no planes (bn_post applies them behind the statistics)
    if (raw) planes = false;
    GemmArgs a{};
    a.A = op.in[0] == -2 ? ses.images() : ptr(op.in[0]);
    if (pk.in_place) {
        a.Wp = params[pk.w[0]].ptr;
        a.bias = params[pk.b[0]].ptr;
    } else {
        a.Wp = pack_arena + pk.w_off;
        a.bias = pack_arena + pk.b_off;
    }
    a.res = raw ? nullptr : op.res_param >= 0 ? params[op.res_param].ptr : ptr(op.aux);
    a.out = ptr(op.out);
    a.M = (int)(op.rows_per_frame * batch);
    a.N = op.N; a.K = op.K; a.Kpad = pk.Kpad;
    if (pk.rh) a.Wp2 = pack_arena + pk.rh_off;
    if (pk.ws || pk.x3) a.Wp3 = pack_arena + (pk.ws ? pk.ws_off : pk.x3_off);
    a.x3_h2 = pk.x3 && plan.x3_h2;
    if (a.x3_h2 && op.h2_utab >= 0 && utab_on_device) a.h2_utab = reinterpret_cast<const unsigned*>(pack_arena + utab_off) + op.h2_utab;
    const Family family = gemm_family(op, batch);
    // the plain fp32 MFMA kernels' problems on the two-fp16-piece GEMM from batch 5 (launch_gemm_f32 / _group route them; below, the fp32
    // kernels with split-K win); LayerNorm folds of up to 256 columns included (igemm_f32h2.hip, LNA)
    if (pk.h2g && batch >= H2G_MIN_BATCH && family == Family::F32 && !op.pw_pair) a.Wh2 = pack_arena + pk.h2g_off;
    if (op.fast3x3 && family == Family::F32) {       // small batch: the direct kernel on the direct-layout copy of the weights
        a.Wp = pack_arena + pk.direct_off;
        a.Kpad = pk.direct_Kpad;
    } else if (family == Family::F32_TILE && pk.wino_skip) {
        a.Wp = nullptr;                              // no Winograd layout was packed; the tile reads Wp3
    }
    a.conv = op.conv;
    a.Cin = op.Cin; a.H = op.H; a.W = op.W; a.Ho = op.Ho; a.Wo = op.Wo;
    a.ks = op.ks; a.stride = op.stride; a.pad = op.pad;
    a.amap = op.amap; a.omap = op.omap; a.rmap = op.rmap;
    a.act = raw ? ACT_NONE : op.act;
    a.out_bf16 = op.out_bf16;
    a.f16 = f16();                                     // (the element format of whatever 16-bit kernel takes the problem)
    a.f32s = op.f32s;                                  // (CAPF_PLAN_BF16_F32_STREAM: fp32 residual; fp32 result + bf16 shadow, or bf16 result)
    a.out_f32 = op.st_f32;
    a.out_sh = op.sh >= 0 ? ptr(op.sh) : nullptr;
    // planes between a BasicBlock's two convs (hr_basic_block pairs them under the two-fp16-piece plan only): where BOTH run the tile at this batch
    if (planes && op.h2_role && family == Family::F32_TILE && gemm_family(ops[op.h2_peer], batch) == Family::F32_TILE) {
        int* e = reinterpret_cast<int*>(ptr(op.h2_exps));
        if (op.h2_role == 1) a.h2_eout = e; else a.h2_ein = e;
    }
    if (op.conv && op.up_in >= 0) {                    // + bilinear_upsample(up_in) behind the activation (build_cpn: lateral + upsampled path)
        a.up = ptr(op.up_in);
        a.up_H = op.up_H; a.up_W = op.up_W;
        a.up_sh = op.Ho > 1 ? (float)(op.up_H - 1) / (float)(op.Ho - 1) : 0.f;
        a.up_sw = op.Wo > 1 ? (float)(op.up_W - 1) / (float)(op.Wo - 1) : 0.f;
    }
    static const bool splitk_on = [] { const char* e = diag_env("CAPF_SPLITK"); return !e || atoi(e) != 0; }();   // A/B runs only
    if ((op.conv || (op.kind == OP_GEMM && op.ln.w < 0 && op.res_param < 0)) && !op.bf16 && split_ws && lanes != 1 && splitk_on) {   // one stream: launches use the scratch one after the other
        a.split_ws = side_chain ? split_ws_side : split_ws;
        a.split_cnt = side_chain ? split_cnt_side : split_cnt;
        a.split_ws_elems = SPLIT_WS_ELEMS; a.split_cnt_elems = SPLIT_CNT_ELEMS;
    }
    if (op.ln.w >= 0) {
        a.ln_g = params[op.ln.w].ptr;
        a.ln_b = params[op.ln.b].ptr;
        a.ln_eps = op.eps;
    }
    return a;
}

// Fused launches, the priority among them written out here: at a fork, a first bottleneck; at a conv, an identity bottleneck, else a
// pointwise pair -- which never starts inside a fused bottleneck, nor takes the conv1 of one (the conv3 of a fused bottleneck does not chain
// into the next block; a fused next block runs its own conv1).  Both bottlenecks need 64 Ki pixels: below, the 256 persistent blocks get
// fewer than four tiles each and the separate launches win.
Engine::FusedLaunch Engine::fused_at(int i, int batch, int last_op, bool bneck_only) const {
    const int n_all = (int)ops.size();
    if (i < 0 || i >= n_all || bn_run) return {};              // (the batch-statistics route: no launch crosses a BatchNorm)
    const Op& o = ops[i];
    if (o.kind == OP_FORK) {                                   // conv1, conv2 | downsample inside the region, conv3 right after its join
        if (!plan.use_bneck || !b16() || o.fork.lanes != 2 || o.region < 0) return {};
        const int j = regions[o.region].second;
        if (j != i + 4 || j + 1 >= last_op || j + 1 >= n_all) return {};
        int c1 = -1, c2 = -1, ds = -1;
        for (int k = i + 1; k < j; ++k) {
            const Op& g = ops[k];
            if (g.kind != OP_GEMM || !g.conv || g.bf16 != 1) return {};
            if (g.lane == 1) ds = k; else if (c1 < 0) c1 = k; else c2 = k;
        }
        const int c3 = j + 1;
        if (c1 < 0 || c2 < 0 || ds < 0 || ops[c3].kind != OP_GEMM || !ops[c3].conv || ops[c3].bf16 != 1) return {};
        if (ops[c2].in[0] != ops[c1].out || ops[ds].in[0] != ops[c1].in[0] || ops[c3].in[0] != ops[c2].out || ops[c3].aux != ops[ds].out) return {};
        if (ops[c1].rows_per_frame * batch < 65536) return {};
        if (!bneck0_bf16_ok(gemm_args(ops[c1], batch), gemm_args(ops[c2], batch), gemm_args(ops[ds], batch), gemm_args(ops[c3], batch))) return {};
        return {Fusion::BNECK0, 4, {c1, c2, ds, c3}};
    }
    if (o.kind != OP_GEMM) return {};
    if (plan.use_bneck && b16() && i + 2 < last_op && i + 2 < n_all) {
        const Op &c2 = ops[i + 1], &c3 = ops[i + 2];
        bool ok = o.bneck_c3 == i + 2 && c2.in[0] == o.out && c3.in[0] == c2.out && c3.aux == o.in[0] && o.aux < 0 && c2.aux < 0 &&
                  o.rows_per_frame * batch >= 65536;
        for (const Op* g : {&o, &c2, &c3})
            ok = ok && g->kind == OP_GEMM && g->conv && g->bf16 == 1 && g->region == o.region && g->lane == o.lane && g->up_in < 0;
        if (ok && bneck1_bf16_ok(gemm_args(o, batch), gemm_args(c2, batch), gemm_args(c3, batch))) return {Fusion::BNECK1, 3, {i, i + 1, i + 2}};
    }
    if (bneck_only || !plan.use_pwchain || i + 1 >= last_op || i + 1 >= n_all) return {};
    const Op& b = ops[i + 1];
    if (!o.conv || b.kind != OP_GEMM || !b.conv || o.bf16 != b.bf16 || o.bf16 > 1 || b.in[0] != o.out || b.region != o.region || b.lane != o.lane) return {};
    if (o.bf16 && (fused_leader(i, batch, true).n || fused_at(i + 1, batch, last_op, true).n)) return {};
    const GemmArgs ga = gemm_args(o, batch), gb = gemm_args(b, batch);
    if (!(o.bf16 ? gemm_bf16_pwchain_ok(ga, gb) : gemm_f32_pwchain_ok(ga, gb))) return {};
    return {Fusion::PWCHAIN, 2, {i, i + 1}};
}

Engine::FusedLaunch Engine::fused_leader(int i, int batch, bool bneck_only) const {
    for (int f = i - 5; f <= i; ++f) {                         // (the longest launch spans fork, conv1, conv2, downsample, join, conv3)
        const FusedLaunch l = fused_at(f, batch, (int)ops.size(), bneck_only);
        for (int k = 0; k < l.n; ++k)
            if (l.m[k] == i) return l;
    }
    return {};
}

Engine::Family Engine::gemm_family(const Op& op, int batch) const {
    const bool tile = batch >= op.tile_lo && batch <= op.tile_hi;                   // (build() sets the range for 3x3 stride-1 convs with a tile pack alone)
    if (op.bf16) return op.bf16 == 2 ? Family::BF16_ROWS : tile ? Family::BF16_TILE : Family::BF16;
    if (tile) return Family::F32_TILE;
    return op.fast3x3 && batch >= plan.wino_min_batch && !packs[op.pack].wino_skip ? Family::WINO : Family::F32;
}

// Does the plan's halo tile take this conv at this batch?  Where it is big enough for the tile to pay -- a 16-bit conv from 1 GFLOP and batch
// 24 (bf16_tile_big_enough), an fp32 one from 370 MFLOP and batch 5 (f32_tile_big_enough) -- and the tile's launcher accepts the problem as
// gemm_args describes it -- pointers aside: the test looks at none but whether there is a residual, which a placeholder stands for that
// nothing reads through.  build() asks this once per op and batch range; nothing on the launch path asks again
bool Engine::tile_takes(const Op& op, int batch) const {
    if (!(op.bf16 ? bf16_tile_big_enough : f32_tile_big_enough)(batch, op.H, op.W, op.Cin, op.N)) return false;
    static const float residual = 0.f;
    GemmArgs a = gemm_args(op, batch, false);
    if (op.aux >= 0 || op.res_param >= 0) a.res = &residual;
    return op.bf16 ? gemm_bf16_ws_ok(a) : plan.x3_h2 ? gemm_f32h2_ok(a) : gemm_f32x3_ok(a);
}

// FLOPs the MFMA pipe is asked to execute (2 x MACs issued, K padding included, tile-edge padding not): the Winograd kernels issue 18
// (F(4,3), per four outputs) or 12 (F(2,3), per two) MACs per (cin, cout) where the direct conv issues 36 / 18, i.e. 1/2 or 2/3 of the
// algorithmic count; the split-fp32 tiles three fp16 / six bf16 piece products per fp32 product, the two-fp16-piece GEMM three -- on the
// 16-bit pipe, whose peak is 16 x the fp32 pipe's
Engine::OpRoute Engine::op_route(const Op& op, int batch) const {
    static const char* kn[] = {"", "fuse_sum", "maxpool3x3s2", "bilinear_resize", "prep_embed", "sample_ref",
                               "layernorm", "deform_sample", "attention", "head", "", "", "embed", "ctx_attn", "res_chain", "mlp_chain", "concat_channels"};
    if (op.kind != OP_GEMM) return {Family::NONE, kn[op.kind], op.flops_per_frame * batch};
    const Pack& pk = packs[op.pack];
    const double MN = 2.0 * (double)op.rows_per_frame * batch * op.N;
    const Family f = gemm_family(op, batch);
    if (f == Family::BF16_ROWS) return {f, gemm_bf16_rows_kernel_name((int)(op.rows_per_frame * batch), op.N, f16()), MN * (pk.in_place ? op.K : pk.Kpad)};
    const GemmArgs a = gemm_args(op, batch);
    if (f == Family::BF16)                                     // (the row-halo layout has no K padding: decided per launch, a lower bound)
        return {f, gemm_bf16_kernel_name(a), MN * (pk.rh || pk.in_place ? op.K : pk.Kpad)};
    // (the tile issues op.K: its pack has no K padding.  The count stays the one these ops had as BF16 ops -- the standard layout's padded K
    // under CAPF_PLAN_NO_ROW_HALO, where K = 9 * Cin is no multiple of 64 -- so that tests/golden/op_routes.npz stands as recorded)
    if (f == Family::BF16_TILE) return {f, gemm_bf16_ws_kernel_name(a), MN * (pk.rh || pk.in_place ? op.K : pk.Kpad)};
    if (f == Family::F32_TILE) return {f, plan.x3_h2 ? gemm_f32h2_kernel_name() : gemm_f32x3_kernel_name(), (plan.x3_h2 ? 3.0 : 6.0) * MN * op.K};
    if (f == Family::WINO) return {f, gemm_wino_kernel_name(a), MN * op.Cin * (pk.Kpad == 18 * pk.Cin ? 4.5 : 6.0)};
    return {f, gemm_f32_kernel_name(a), gemm_f32_route(a).path == F32Path::H2G ? 3.0 * MN * pk.h2g_Kpad       // (small batch: a fast3x3 conv on
                                        : MN * (op.fast3x3 ? pk.direct_Kpad : pk.in_place ? op.K : pk.Kpad)};     // the direct layout)
}

FuseSumArgs Engine::fuse_args(const Op& op, int batch) const {
    FuseSumArgs a{};
    a.n_in = op.n_in;
    for (int i = 0; i < op.n_in; ++i) {
        a.in[i] = op.in[i] >= 0 ? bptr(op.in[i], batch) : nullptr;
        a.shift[i] = op.shift[i];
    }
    a.out = op.out >= 0 ? bptr(op.out, batch) : nullptr;
    a.B = batch; a.H = op.H; a.W = op.W; a.C = op.C; a.relu = op.relu;
    a.bf16 = op.bf16;
    a.f16 = f16();
    a.out_sh = op.sh >= 0 ? bptr(op.sh, batch) : nullptr;
    return a;
}

// one non-control op on stream s
int Engine::exec_op(const Op& op, hipStream_t s, int batch, bool side_chain) {
    auto ptr = [&](int buf) -> float* {
        if (buf >= 0) return bptr(buf, batch);
        return nullptr;
    };
    const float* const k2d = ses.k2d;
    float* const kcrop = ses.kcrop;
    switch (op.kind) {
        case OP_GEMM: {
            const GemmArgs a = gemm_args(op, batch, true, side_chain);
            switch (gemm_family(op, batch)) {
                case Family::BF16_ROWS:
                    HIP_TRY(launch_gemm_bf16_rows(a.A, a.Wp, a.bias, a.M, a.N, a.K, a.Kpad, a.out, a.omap, a.res, a.rmap, op.out_bf16, s, f16()));
                    break;
                case Family::BF16: HIP_TRY(launch_gemm_bf16(a, s)); break;
                case Family::BF16_TILE: HIP_TRY(launch_gemm_bf16_ws_group(&a, 1, s)); break;
                case Family::F32_TILE: HIP_TRY(launch_f32_tile(&a, 1, s)); break;
                case Family::WINO: HIP_TRY(launch_gemm_wino(a, s)); break;
                default:
                    if (op.in[0] == -2 && ses.u8()) HIP_TRY(launch_gemm_stem(a, ses.u8(), s));   // the stem from the uint8 crop: same route, U8 form
                    else HIP_TRY(launch_gemm_f32(a, s));
            }
            if (bn_run) {
                const int oi = (int)(&op - ops.data());
                if (const int rc = bn_post(s, batch, &oi, 1)) return rc;
            }
            break;
        }
        case OP_FUSE: {
            if (skipped(op)) break;
            HIP_TRY(launch_fuse_sum(fuse_args(op, batch), s));
            break;
        }
        case OP_MAXPOOL:
            HIP_TRY(launch_maxpool3x3s2(ptr(op.in[0]), ptr(op.out), batch, op.H, op.W, op.C, op.Ho, op.Wo, s, op.bf16, f16()));
            break;
        case OP_RESIZE:
            HIP_TRY(launch_bilinear_resize(ptr(op.in[0]), ptr(op.out), batch, op.H, op.W, op.C, op.Ho, op.Wo, s, op.bf16, ptr(op.aux), f16()));
            break;
        case OP_CONCAT: {
            const float* src[4] = {ptr(op.in[0]), ptr(op.in[1]), ptr(op.in[2]), ptr(op.in[3])};
            HIP_TRY(launch_concat_channels(src, op.n_in, ptr(op.out), (long)batch * op.H * op.W, op.C * (op.bf16 ? 2 : 4), s));
            break;
        }
        case OP_PREP_EMBED:
            HIP_TRY(launch_prep_embed(kcrop, k2d, params[op.coord.w].ptr, params[op.coord.b].ptr, params[op.pos].ptr,
                                      ptr(op.out), batch, op.smp.J, op.smp.L1, op.C, s));
            break;
        case OP_SAMPLE_REF:
            HIP_TRY(launch_sample_ref(ptr(op.in[0]), kcrop, ptr(op.out), reinterpret_cast<int*>(ptr(op.idx_out)),
                                      batch, op.smp.J, op.H, op.W, op.C, s, op.feat_bf16));
            break;
        case OP_LAYERNORM:
            HIP_TRY(launch_layernorm(ptr(op.in[0]), op.amap, ptr(op.aux), op.rmap, params[op.ln.w].ptr,
                                     params[op.ln.b].ptr, op.eps, ptr(op.out), (int)(op.rows_per_frame * batch),
                                     op.C, s, op.out_bf16 ? 1 + (int)f16() : 0));
            break;
        case OP_DEFORM: {
            DeformArgs a{};
            for (int l = 0; l < op.smp.L; ++l) {
                a.feat[l] = ptr(op.in[l]);
                a.H[l] = op.lvlH[l]; a.W[l] = op.lvlW[l]; a.C[l] = op.lvlC[l];
                a.U[l] = ptr(op.outs[l]);
            }
            a.AO = ptr(op.aux);
            a.ref = kcrop;
            a.B = batch; a.J = op.smp.J; a.L = op.smp.L; a.NH = op.smp.NH; a.NS = op.smp.NS;
            a.feat_bf16 = op.feat_bf16;
            if (debug && op.tap_pos >= 0) { a.cpos = ptr(op.tap_pos); a.cidx = reinterpret_cast<int*>(ptr(op.tap_idx)); }
            HIP_TRY(launch_deform_sample(a, s));
            break;
        }
        case OP_EMBED: {
            EmbedArgs a{};
            a.kcrop = kcrop; a.k2d = k2d;
            a.cw = params[op.coord.w].ptr; a.cb = params[op.coord.b].ptr; a.pos = params[op.pos].ptr;
            for (int l = 0; l < op.smp.L; ++l) {
                a.feat[l] = ptr(op.in[l]);
                a.H[l] = op.lvlH[l]; a.W[l] = op.lvlW[l]; a.Cl[l] = op.lvlC[l];
                a.fw[l] = pack_arena + packs[op.pq[l]].w_off; a.fb[l] = params[op.pb[l]].ptr;
                a.sampled[l] = ptr(op.outs[l]);
                a.idx[l] = reinterpret_cast<int*>(ptr(op.idx_lvl[l]));
            }
            a.X = ptr(op.out);
            a.BJ = batch * op.smp.J; a.J = op.smp.J; a.L = op.smp.L; a.L1 = op.smp.L1; a.C = op.C;
            a.feat_bf16 = op.feat_bf16;
            HIP_TRY(launch_embed(a, s));
            break;
        }
        case OP_CTX_ATTN: {
            CtxAttnArgs a{};
            const Pack& pk = packs[op.pack];
            for (int l = 0; l < op.smp.L; ++l) {
                a.feat[l] = ptr(op.in[l]);
                a.H[l] = op.lvlH[l]; a.W[l] = op.lvlW[l]; a.Cl[l] = op.lvlC[l];
                a.Wp[l] = pack_arena + packs[op.pq[l]].w_off; a.bp[l] = params[op.pb[l]].ptr;
                a.U[l] = op.outs[l] >= 0 ? ptr(op.outs[l]) : nullptr;
            }
            a.Wao = pack_arena + pk.w_off; a.bao = pack_arena + pk.b_off; a.ldw = pk.Kpad;
            a.ln_g = params[op.ln.w].ptr; a.ln_b = params[op.ln.b].ptr; a.eps = op.eps;
            a.ref = kcrop;
            a.X = ptr(op.out);
            a.BJ = batch * op.smp.J; a.J = op.smp.J; a.L = op.smp.L; a.L1 = op.smp.L + 1; a.C = op.C; a.NH = op.smp.NH; a.NS = op.smp.NS;
            a.feat_bf16 = op.feat_bf16;
            if (debug && op.tap_pos >= 0) { a.cpos = ptr(op.tap_pos); a.cidx = reinterpret_cast<int*>(ptr(op.tap_idx)); }
            HIP_TRY(launch_ctx_attn(a, s));
            break;
        }
        case OP_ATTENTION:
            HIP_TRY(launch_attention(ptr(op.in[0]), ptr(op.out), op.attn.groups * batch, op.attn.tokens, op.attn.heads, op.attn.head_dim, s, op.out_bf16 ? 1 + (int)f16() : 0));
            break;
        case OP_RES_CHAIN: {
            ResBlockW blk[8];
            const int nblk = (int)op.blocks.size();
            for (int i = 0; i < nblk; ++i) {
                const ChainBlock& c = op.blocks[i];
                const Pack *q = &packs[c.qkv], *pr = &packs[c.proj], *f1 = &packs[c.fc1], *f2 = &packs[c.fc2];
                if (!q->chain || !pr->chain || !f1->chain || !f2->chain || q->h2g_Kpad != q->K || f2->h2g_Kpad != f2->K) return CAPF_ERR_STATE;
                blk[i] = ResBlockW{params[c.norm1.w].ptr, params[c.norm1.b].ptr, pack_arena + q->chain_off, params[q->b[0]].ptr, pack_arena + pr->chain_off,
                                   params[pr->b[0]].ptr, params[c.norm2.w].ptr, params[c.norm2.b].ptr, pack_arena + f1->chain_off, params[f1->b[0]].ptr,
                                   pack_arena + f2->chain_off, params[f2->b[0]].ptr};
            }
            HIP_TRY(launch_res_chain(ptr(op.out), (int)(op.rows_per_frame * batch), op.attn.tokens, op.attn.heads, op.eps, blk, nblk, s));
            break;
        }
        case OP_MLP_CHAIN: {
            const ChainBlock& c = op.blocks[0];
            const Pack *f1 = &packs[c.fc1], *f2 = &packs[c.fc2];
            if (!f1->chain || !f2->chain || f1->h2g_Kpad != f1->K || f2->h2g_Kpad != f2->K) return CAPF_ERR_STATE;
            ResBlockW w{};
            w.ln2_g = params[c.norm2.w].ptr; w.ln2_b = params[c.norm2.b].ptr;
            w.wfc1 = pack_arena + f1->chain_off; w.bfc1 = params[f1->b[0]].ptr;
            w.wfc2 = pack_arena + f2->chain_off; w.bfc2 = params[f2->b[0]].ptr;
            HIP_TRY(launch_mlp_chain(ptr(op.out), op.amap, (int)(op.rows_per_frame * batch), op.eps, w, s));
            break;
        }
        case OP_HEAD:
            HIP_TRY(launch_head(ptr(op.in[0]), params[op.ln.w].ptr, params[op.ln.b].ptr, op.eps, params[op.head.w].ptr,
                                params[op.head.b].ptr, ses.out, (int)(op.rows_per_frame * batch), op.C, op.head.N, s));
            break;
        default: break;
    }
    return CAPF_OK;
}

// Fork/join region as dependency levels on ONE stream: the convs of a level (one per HRNet branch, or
// the many small convs of a fuse layer) go out as grouped launches, one per kernel family (gemm_family; a
// level's 2-D halo tile convs ahead of its other 16-bit convs), everything else one by one.  Any
// topological order is valid on a single stream, and no two buffers of a region share memory
// (assign_offsets keeps them alive for the whole region).  With `log` every launch is bracketed by
// events (profiling): log gets (event index, leader op) pairs and member ops point at their leader.
int Engine::run_region_grouped(hipStream_t s, int batch, int region, LaunchLog* log, unsigned lane_mask, bool side_chain) {
    auto mine = [&](const Op& op) { return ((lane_mask >> op.lane) & 1u) != 0; };
    auto groupable = [&](const Op& op, const GemmArgs& a) {
        if (op.kind != OP_GEMM) return false;
        switch (gemm_family(op, batch)) {
            case Family::BF16: return gemm_bf16_groupable(a);
            case Family::BF16_TILE: case Family::F32_TILE: return true;
            case Family::WINO: return gemm_wino_ok(a);
            case Family::F32: return gemm_f32_groupable(a);
            default: return false;
        }
    };
    for (const std::vector<int>& level : region_levels[region]) {
        for (Family pass : {Family::F32, Family::BF16_TILE, Family::BF16, Family::F32_TILE, Family::WINO}) {
            GemmArgs group[MAXG];
            int members[MAXG];
            int n = 0;
            auto flush = [&]() -> int {
                if (n == 0) return CAPF_OK;
                if (log) HIP_TRY(log->mark(s, members, n));
                if (pass == Family::F32) HIP_TRY(launch_gemm_f32_group(group, n, s));
                else if (pass == Family::BF16_TILE) {
                    HIP_TRY(launch_gemm_bf16_ws_group(group, n, s));
                    if (log && !log->op_variant.empty()) log->op_variant[members[0]] = 3;
                }
                else if (pass == Family::BF16) {
                    int v = -1;
                    HIP_TRY(launch_gemm_bf16_group(group, n, s, &v));
                    if (log && !log->op_variant.empty()) log->op_variant[members[0]] = v;
                }
                else if (pass == Family::F32_TILE) HIP_TRY(launch_f32_tile(group, n, s));
                else HIP_TRY(launch_gemm_wino_group(group, n, s));
                if (bn_run)
                    if (const int rc = bn_post(s, batch, members, n)) return rc;
                n = 0;
                return CAPF_OK;
            };
            for (int oi : level) {
                const Op& op = ops[oi];
                if (op.kind != OP_GEMM || !mine(op) || gemm_family(op, batch) != pass) continue;
                const GemmArgs a = gemm_args(op, batch, true, side_chain);
                if (!groupable(op, a)) continue;
                group[n] = a;
                members[n++] = oi;
                if (n == MAXG) { int rc = flush(); if (rc) return rc; }
            }
            int rc = flush();
            if (rc) return rc;
        }
        {   // the fuse sums of a level (schedule_regions gathers a module's sums in its last level): one launch
            FuseSumArgs fg[4];
            int fm[4], nf = 0;
            for (int oi : level) {
                const Op& op = ops[oi];
                if (op.kind != OP_FUSE || skipped(op) || !mine(op)) continue;
                if (nf > 0 && (op.bf16 != ops[fm[0]].bf16 || (op.C % 8 == 0) != (ops[fm[0]].C % 8 == 0))) continue;
                if (nf == 4) break;
                fg[nf] = fuse_args(op, batch);
                fm[nf++] = oi;
            }
            if (nf < 2) nf = 0;
            if (nf) {
                if (log) HIP_TRY(log->mark(s, fm, nf));
                HIP_TRY(launch_fuse_sum_group(fg, nf, s));
            }
            for (int oi : level) {
                const Op& op = ops[oi];
                if (!mine(op)) continue;
                if (op.kind == OP_GEMM && groupable(op, gemm_args(op, batch))) continue;
                if (skipped(op)) continue;
                bool done = false;
                for (int k = 0; k < nf; ++k) done |= fm[k] == oi;
                if (done) continue;
                if (log) HIP_TRY(log->mark(s, &oi, 1));
                int rc = exec_op(op, s, batch, side_chain);
                if (rc) return rc;
            }
        }
    }
    return CAPF_OK;
}

// ev: per-op events (profiling, everything in program order on one stream).  log: per-launch events of
// the product schedule (grouped launches included).
int Engine::run(hipStream_t s, int batch, int first_op, int last_op, hipEvent_t* ev, LaunchLog* log) {
    hipStream_t main_stream = s;
    if (plan.use_h2g && (batch >= H2G_MIN_BATCH || has_res_chain) && last_op > n_backbone_ops && !b16()) {      // (the fused res blocks read the packs at every batch)
        const int rc = ensure_h2g_lifter(s);
        if (rc) return rc;
    }
    const bool grouped = (lanes == 2 || lanes == 3) && !ev;
    const bool par = lanes == 1 && !ev && !log && side[0] && !bn_run;      // (the batch-statistics route shares its scratch slots: one stream)
    for (int oi = first_op; oi < last_op; ++oi) {
        const Op& op = ops[oi];
        s = (par && op.lane > 0) ? side[op.lane - 1] : main_stream;
        if (ev) HIP_TRY(hipEventRecord(ev[oi], s));
        if (const FusedLaunch f = ev ? FusedLaunch{} : fused_at(oi, batch, last_op); f.n) {
            // several ops as one launch (bneck_bf16.hip, igemm_*_pwchain.hip); prefix runs (the layer-wise tests' capf_forward_prefix) and
            // debug runs take the bottleneck variant that also stores the inner convs' outputs where the separate launches would have
            const bool tap = debug || last_op < (int)ops.size();
            GemmArgs m[4];
            for (int k = 0; k < f.n; ++k) m[k] = gemm_args(ops[f.m[k]], batch);
            if (log) HIP_TRY(log->mark(s, f.m, f.n));
            if (f.kind == Fusion::BNECK0) HIP_TRY(launch_bneck0_bf16(m[0], m[1], m[2], m[3], tap, s));
            else if (f.kind == Fusion::BNECK1) HIP_TRY(launch_bneck1_bf16(m[0], m[1], m[2], tap, s));
            else if (op.bf16) HIP_TRY(launch_gemm_bf16_pwchain(m[0], m[1], s));
            else HIP_TRY(launch_gemm_f32_pwchain(m[0], m[1], s));
            oi = f.m[f.n - 1];
            continue;
        }
        switch (op.kind) {
            case OP_FORK: {
                if (grouped && regions[op.region].second <= last_op) {
                    // lanes == 3: the lanes of a region as TWO grouped chains on two streams (lanes 0 + 3 on the caller's, 1 + 2 on a
                    // side stream), so that one chain's launch ramp / tail overlaps the other's body.  Measured at batch 64 (one
                    // box, frames/s): one chain 6418; {0,3}|{1,2} 6497; {0,1}|{2,3} 5964; {0,2}|{1,3} 6101; {0,1,2}|{3} 6149;
                    // {0}|{1,2,3} 6398.  Across the configurations: cfg1 +0.4..1.2 %, cfg2 +0.9 %, cfg4 +1.3 %, but -0.8 % at batch 512 (every launch already fills
                    // the chip many times over), and below batch 16 a region is a handful of tiles (and may use the split-K scratch):
                    // one chain outside 16..256 (until round 11).  Round 11, five alternating pairs against one chain per configuration: cfg1 (batch 64) +1.2 % and
                    // +2.2 % on two boxes, cfg2 (bf16, batch 256) -0.45 % at twice its pair-to-pair spread: two chains up to batch 128 (two_chains()).
                    const bool two = two_chains(op, batch) && !log && side[0] && !bn_run;
                    if (two) {
                        HIP_TRY(hipEventRecord(events[op.fork.first_event], main_stream));
                        HIP_TRY(hipStreamWaitEvent(side[0], events[op.fork.first_event], 0));
                        int rc = run_region_grouped(side[0], batch, op.region, nullptr, 0x6u, true);
                        if (rc) return rc;
                        rc = run_region_grouped(main_stream, batch, op.region, nullptr, ~0x6u);
                        if (rc) return rc;
                        HIP_TRY(hipEventRecord(events[op.fork.first_event + 1], side[0]));
                        HIP_TRY(hipStreamWaitEvent(main_stream, events[op.fork.first_event + 1], 0));
                        oi = regions[op.region].second;
                        break;
                    }
                    int rc = run_region_grouped(main_stream, batch, op.region, log);
                    if (rc) return rc;
                    oi = regions[op.region].second;      // continue after the join
                } else if (par) {
                    HIP_TRY(hipEventRecord(events[op.fork.first_event], main_stream));
                    for (int l = 1; l < op.fork.lanes; ++l) HIP_TRY(hipStreamWaitEvent(side[l - 1], events[op.fork.first_event], 0));
                }
                break;
            }
            case OP_JOIN:
                if (par) {
                    for (int l = 1; l < op.fork.lanes; ++l) {
                        HIP_TRY(hipEventRecord(events[op.fork.first_event + l], side[l - 1]));
                        HIP_TRY(hipStreamWaitEvent(main_stream, events[op.fork.first_event + l], 0));
                    }
                }
                break;
            default: {
                if (skipped(op)) break;
                if (log) {
                    HIP_TRY(log->mark(s, &oi, 1));
                    // (a lone 2-D halo tile conv is a one-problem launch of the tile's grouped kernel: the log says so, as for a region's)
                    if (!log->op_variant.empty() && op.kind == OP_GEMM && gemm_family(op, batch) == Family::BF16_TILE) log->op_variant[oi] = 3;
                }
                int rc = exec_op(op, s, batch);
                if (rc) return rc;
            }
        }
    }
    if (ev) HIP_TRY(hipEventRecord(ev[last_op], main_stream));
    if (log) HIP_TRY(log->mark(main_stream, nullptr, 0));
    if (first_op == 0) ses.maps_written(last_op >= n_backbone_ops ? batch : 0);      // (a prefix run leaves the maps half written)
    return CAPF_OK;
}

size_t Engine::bn_slot_elems(int batch) const {
    size_t worst = 0;
    for (const BnUnit& u : bn_units) {
        const Op& op = ops[u.op];
        worst = std::max(worst, 2 * (size_t)op.N + bn_scratch_elems(op.rows_per_frame * batch, op.N));
    }
    return (worst + 63) / 64 * 64;
}

// Behind raw convs of the batch-statistics route: per unit the statistics of the conv's output (two launches: slab partials, then their
// combination into scale / shift and the running statistics, written through the pointers capf_set_param borrowed) and the normalise /
// residual / ReLU pass in place over it -- up to BN_SLOTS units per launch, slot k = {scale | shift | slab partials} of the k-th
int Engine::bn_post(hipStream_t s, int batch, const int* members, int n) {
    float* const base = ws + bn_base(batch);
    const size_t slot = bn_slot_elems(batch);
    for (int i = 0; i < n;) {
        BnStatsArgs st[BN_SLOTS];
        BnApplyArgs ap[BN_SLOTS];
        int k = 0;
        for (; i < n && k < BN_SLOTS; ++i) {
            const int ui = bn_unit_of[members[i]];
            if (ui < 0) continue;
            const Op& op = ops[members[i]];
            const BnRef& bn = bn_units[ui].bn;
            float* const sl = base + slot * k;
            BnStatsArgs& a = st[k];
            a = BnStatsArgs{};
            a.x = bptr(op.out, batch);
            a.gamma = params[bn.g].ptr; a.beta = params[bn.b].ptr;
            a.rmean = const_cast<float*>(params[bn.m].ptr); a.rvar = const_cast<float*>(params[bn.v].ptr);
            a.scale = sl; a.shift = sl + op.N;
            a.part = reinterpret_cast<double*>(sl + 2 * (size_t)op.N);
            a.rows = op.rows_per_frame * batch; a.C = op.N;
            a.eps = 1e-5f; a.momentum = bn_momentum;
            ap[k] = BnApplyArgs{a.x, op.aux >= 0 ? bptr(op.aux, batch) : nullptr, bptr(op.out, batch), a.scale, a.shift, a.rows, a.C, op.act == ACT_RELU};
            ++k;
        }
        if (k == 0) continue;
        HIP_TRY(launch_bn_stats_group(st, k, s));
        HIP_TRY(launch_bn_apply_group(ap, k, s));
    }
    return CAPF_OK;
}

Engine::~Engine() {
    for (void* p : {(void*)pack_arena, (void*)split_ws, (void*)split_cnt, (void*)split_ws_side, (void*)split_cnt_side})
        if (p) (void)hipFree(p);
    for (hipEvent_t x : events)
        if (x) (void)hipEventDestroy(x);
    for (hipStream_t st : side)
        if (st) (void)hipStreamDestroy(st);
}

int Engine::check_run(int batch) {
    if (device < 0) {
        err = "plan-only handle (device < 0)";
        return CAPF_ERR_STATE;
    }
    if (batch <= 0 || batch > cfg.max_batch) {
        err = "batch out of range (1..max_batch)";
        return CAPF_ERR_INVALID;
    }
    if (batch > batch_limit) {
        err = "batch too large for this input size: the kernels address one activation tensor with 32-bit offsets (limit " +
              std::to_string(batch_limit) + " frames)";
        return CAPF_ERR_UNSUPPORTED;
    }
    if (!packed) {
        err = "capf_params_changed has not been called since the last capf_set_param";
        return CAPF_ERR_STATE;
    }
    if (!ws || ws_bytes < workspace_bytes(batch)) {
        err = "workspace missing or too small";
        return CAPF_ERR_STATE;
    }
    return CAPF_OK;
}

// The checks in the order every entry has always made them: training, the uint8 source's own (capf_forward_u8 and its siblings: nothing but
// the stem's load differs from the float entries, launch_gemm_stem), check_run, the maps, the uint8 stem.  Then, and only then, the state
int Engine::begin(const Call& c) {
    if (c.training && !cfg.training) {
        err = "handle was created with training = 0";
        return CAPF_ERR_STATE;
    }
    const U8Input* u8 = std::get_if<U8Input>(&c.image);
    if (u8) {
        if (!u8->img) return CAPF_ERR_INVALID;             // (a null image or mean: u8_source)
        if (u8->mode < 0 || u8->mode > 2) {
            err = "mode must be 0 (as is), 1 (every frame mirrored) or 2 (flip test: [orig | mirrored])";
            return CAPF_ERR_INVALID;
        }
        if (u8->mode == 2 && (c.batch & 1)) {
            err = "mode 2 runs 2 * Bsrc engine frames: batch must be even";
            return CAPF_ERR_INVALID;
        }
    }
    if (c.bn && !plan.bn_batch) {
        err = std::string(c.who) + ": the handle was created without CAPF_PLAN_BN_BATCH_STATS";
        return CAPF_ERR_STATE;
    }
    if (const int rc = check_run(c.batch)) return rc;
    if (c.bn) {
        if (!(c.momentum >= 0.f && c.momentum <= 1.f)) {
            err = std::string(c.who) + ": momentum must lie in [0, 1]";
            return CAPF_ERR_INVALID;
        }
        for (const BnUnit& u : bn_units)
            if (ops[u.op].rows_per_frame * c.batch < 2) {
                err = std::string(c.who) + ": expected more than 1 value per channel when training: " + ops[u.op].name + " has " +
                      std::to_string(ops[u.op].Ho) + " x " + std::to_string(ops[u.op].Wo) + " outputs per frame at batch " + std::to_string(c.batch);
                return CAPF_ERR_INVALID;
            }
    }
    if (c.maps && ses.feat_batch != c.batch) {      // (every buffer lives at offset * batch: maps of another batch are not where this call would sample)
        err = std::string(c.who) + ": the workspace holds no context maps of this batch (capf_set_features or capf_backbone_forward "
              "of the same batch comes first)";
        return CAPF_ERR_STATE;
    }
    if (u8 && (stem_op < 0 || gemm_family(ops[stem_op], c.batch) != Family::F32 || ops[stem_op].Cin != 3)) {
        err = "this plan has no single Cin = 3 stem conv reading the image";
        return CAPF_ERR_UNSUPPORTED;
    }
    ses.image = c.image;
    ses.k2d = c.k2d; ses.kcrop = c.kcrop; ses.out = c.out;
    ses.last_batch = c.batch;
    if (c.maps) ses.invalidate_train();
    else ses.drop_maps();                                  // (until run() or capf_set_features has written them)
    return CAPF_OK;
}

}  // namespace capf

// ---------------------------------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------------------------------
using capf::Engine;

static std::string g_create_error;

extern "C" {

const char* capf_version(void) { return "capf 0.12 (gfx950)"; }
int capf_abi_version(void) { return CAPF_ABI_VERSION; }

const char* capf_last_error(const capf_handle* h) { return h ? h->e.err.c_str() : g_create_error.c_str(); }

int capf_create(const capf_config* cfg, int device, capf_handle** out) {
    if (!cfg || !out) {
        g_create_error = "null argument";
        return CAPF_ERR_INVALID;
    }
    capf_handle* h = new capf_handle();
    Engine& e = h->e;
    e.cfg = *cfg;
    e.device = device;
    if (cfg->compute_dtype != CAPF_F32 && cfg->compute_dtype != CAPF_BF16 && cfg->compute_dtype != CAPF_F16) {
        g_create_error = "compute_dtype must be CAPF_F32, CAPF_BF16 or CAPF_F16";
        delete h;
        return CAPF_ERR_UNSUPPORTED;
    }
    if (cfg->plan_flags & CAPF_PLAN_BN_BATCH_STATS) {      // the batch-statistics route: HRNet, fp32, training handles
        const char* why = cfg->backbone != CAPF_HRNET ? "CAPF_PLAN_BN_BATCH_STATS is an HRNet plan (CPN50 is not supported)"
                          : cfg->compute_dtype != CAPF_F32 ? "CAPF_PLAN_BN_BATCH_STATS needs compute_dtype = CAPF_F32 (bf16 / fp16 batch statistics are not supported)"
                          : !cfg->training ? "CAPF_PLAN_BN_BATCH_STATS needs training = 1 (batch statistics belong to a training handle)"
                          : (cfg->plan_flags & CAPF_PLAN_BF16_F32_STREAM) ? "CAPF_PLAN_BN_BATCH_STATS cannot be combined with CAPF_PLAN_BF16_F32_STREAM" : nullptr;
        if (why) {
            g_create_error = why;
            delete h;
            return CAPF_ERR_UNSUPPORTED;
        }
    }
    if (cfg->compute_dtype == CAPF_F16) {       // the fp16 plan is the HRNet inference plan; what else a 16-bit plan can do is bf16's until it has tests of its own
        const char* why = cfg->backbone != CAPF_HRNET ? "compute_dtype = CAPF_F16 is an HRNet plan (CPN50 is not supported)"
                          : (cfg->plan_flags & CAPF_PLAN_BF16_F32_STREAM) ? "CAPF_PLAN_BF16_F32_STREAM needs compute_dtype = CAPF_BF16 (CAPF_F16 is not supported)"
                          : cfg->training ? "compute_dtype = CAPF_F16 is an inference plan (training = 1 is not supported)" : nullptr;
        if (why) {
            g_create_error = why;
            delete h;
            return CAPF_ERR_UNSUPPORTED;
        }
    }
    if ((cfg->plan_flags & CAPF_PLAN_CPN_PREDICT) && cfg->backbone != CAPF_CPN50) {      // the head of a CPN checkpoint: no other backbone has it
        g_create_error = "CAPF_PLAN_CPN_PREDICT is a CPN50 plan (refine_net.final_predict; HRNet is not supported)";
        delete h;
        return CAPF_ERR_UNSUPPORTED;
    }
    if (cfg->plan_flags & ~(16383 | CAPF_PLAN_BF16_F32_STREAM | CAPF_PLAN_BN_BATCH_STATS | CAPF_PLAN_CPN_PREDICT)) {
        g_create_error = "unknown capf_plan_flag bits";
        delete h;
        return CAPF_ERR_INVALID;
    }
    if (cfg->max_batch <= 0) {
        g_create_error = "max_batch must be positive";
        delete h;
        return CAPF_ERR_INVALID;
    }
    if (!e.build()) {
        g_create_error = e.err;
        delete h;
        return CAPF_ERR_UNSUPPORTED;
    }
    if (device >= 0) {
        hipError_t r = hipSetDevice(device);
        if (r == hipSuccess && e.pack_elems) r = hipMalloc(reinterpret_cast<void**>(&e.pack_arena), e.pack_elems * sizeof(float));
        if (r == hipSuccess) r = hipMalloc(reinterpret_cast<void**>(&e.split_ws), Engine::SPLIT_WS_ELEMS * sizeof(float));
        if (r == hipSuccess) r = hipMalloc(reinterpret_cast<void**>(&e.split_cnt), Engine::SPLIT_CNT_ELEMS * sizeof(int));
        if (r == hipSuccess) r = hipMemset(e.split_cnt, 0, Engine::SPLIT_CNT_ELEMS * sizeof(int));
        if (r == hipSuccess) r = hipMalloc(reinterpret_cast<void**>(&e.split_ws_side), Engine::SPLIT_WS_ELEMS * sizeof(float));
        if (r == hipSuccess) r = hipMalloc(reinterpret_cast<void**>(&e.split_cnt_side), Engine::SPLIT_CNT_ELEMS * sizeof(int));
        if (r == hipSuccess) r = hipMemset(e.split_cnt_side, 0, Engine::SPLIT_CNT_ELEMS * sizeof(int));
        for (int i = 0; i < 3 && r == hipSuccess; ++i) r = hipStreamCreateWithFlags(&e.side[i], hipStreamNonBlocking);
        e.events.resize(e.n_events);
        for (auto& x : e.events)
            if (r == hipSuccess) r = hipEventCreateWithFlags(&x, hipEventDisableTiming);
        if (r != hipSuccess) {
            g_create_error = std::string("hip: ") + hipGetErrorString(r);
            delete h;
            return CAPF_ERR_HIP;
        }
    }
    *out = h;
    return CAPF_OK;
}

void capf_destroy(capf_handle* h) { delete h; }      // (~Engine releases what the handle owns on the device)

int capf_max_batch(const capf_handle* h) { return h ? (h->e.batch_limit < h->e.cfg.max_batch ? h->e.batch_limit : h->e.cfg.max_batch) : CAPF_ERR_INVALID; }

int capf_num_params(const capf_handle* h) { return h ? (int)h->e.params.size() : CAPF_ERR_INVALID; }

int capf_param_info(const capf_handle* h, int index, const char** name, int64_t shape[4], int* ndim, int* kind) {
    if (!h || index < 0 || index >= (int)h->e.params.size()) return CAPF_ERR_INVALID;
    const capf::Param& p = h->e.params[index];
    if (name) *name = p.name.c_str();
    if (shape) memcpy(shape, p.shape, sizeof(p.shape));
    if (ndim) *ndim = p.ndim;
    if (kind) *kind = p.kind;
    return CAPF_OK;
}

int capf_set_param(capf_handle* h, const char* name, const void* dev_ptr, const int64_t* shape, int ndim) {
    if (!h || !name) return CAPF_ERR_INVALID;
    Engine& e = h->e;
    auto it = e.param_index.find(name);
    if (it == e.param_index.end()) {
        e.err = std::string("unknown parameter: ") + name;
        return CAPF_ERR_INVALID;
    }
    capf::Param& p = e.params[it->second];
    bool ok = (ndim == p.ndim);
    for (int i = 0; ok && i < ndim; ++i) ok = (shape[i] == p.shape[i]);
    if (!ok) {
        e.err = std::string("shape mismatch for ") + name;
        return CAPF_ERR_INVALID;
    }
    p.ptr = static_cast<const float*>(dev_ptr);
    e.packed = false;
    return CAPF_OK;
}

int capf_lifter_params_changed(capf_handle* h, void* stream) {
    if (!h) return CAPF_ERR_INVALID;
    if (h->e.device < 0 || !h->e.packed) {
        h->e.err = "capf_params_changed must have run once before capf_lifter_params_changed";
        return CAPF_ERR_STATE;
    }
    return h->e.repack(static_cast<hipStream_t>(stream), true);
}

int capf_params_changed(capf_handle* h, void* stream) {
    if (!h) return CAPF_ERR_INVALID;
    if (h->e.device < 0) {
        h->e.err = "plan-only handle (device < 0)";
        return CAPF_ERR_STATE;
    }
    return h->e.repack(static_cast<hipStream_t>(stream));
}

size_t capf_workspace_bytes(const capf_handle* h, int batch) { return h && batch > 0 ? h->e.workspace_bytes(batch) : 0; }

int capf_set_workspace(capf_handle* h, void* dev_ptr, size_t bytes) {
    if (!h) return CAPF_ERR_INVALID;
    h->e.ws = static_cast<float*>(dev_ptr);
    h->e.ws_bytes = bytes;
    h->e.ses.drop_maps();
    return CAPF_OK;
}

int capf_set_lanes(capf_handle* h, int on) {
    if (!h) return CAPF_ERR_INVALID;
    if (on < 0 || on > 3) return CAPF_ERR_INVALID;
    h->e.lanes = on;
    return CAPF_OK;
}

int capf_set_debug(capf_handle* h, int on) {
    if (!h) return CAPF_ERR_INVALID;
    h->e.debug = on != 0;
    return CAPF_OK;
}

// ---- the run entries.  Each makes its own null checks, describes itself as a Call and hands it to begin(): the order of the checks and the
// session state are begin()'s alone.  begin_and_run: begin(), the call's op span, and behind it the training step's lifter where the call is one
using capf::Call;

static int begin_and_run(Engine& e, void* stream, const Call& c, const float* drop_masks = nullptr) {
    if (const int rc = e.begin(c)) return rc;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (const int rc = e.run(s, c.batch, c.first, c.last)) return rc;
    return c.training ? e.forward_train(s, c.batch, drop_masks) : CAPF_OK;
}

// the uint8 BGR crop of capf_forward_u8 and its siblings as an image source.  A null image or mean gives a source without an image, which
// begin() refuses where these entries always have: behind the training check, in front of the mode's
static capf::ImageSource u8_source(const uint8_t* images_bgr_u8, const float* mean, const float* std3, int mode, int batch) {
    capf::U8Input u{};
    if (!images_bgr_u8 || !mean) return u;
    u.img = images_bgr_u8;
    u.Bsrc = mode == 2 ? batch / 2 : batch;
    u.mode = mode;
    for (int c = 0; c < 3; ++c) { u.mean[c] = mean[c]; u.stdv[c] = std3 ? std3[c] : 1.f; }
    u.use_std = std3 ? 1 : 0;
    return u;
}

int capf_forward(capf_handle* h, void* stream, const float* images_nhwc, const float* k2d, float* kcrop_inout,
                 int batch, float* out) {
    if (!h || !images_nhwc || !k2d || !kcrop_inout || !out) return CAPF_ERR_INVALID;
    return begin_and_run(h->e, stream, {"capf_forward", images_nhwc, k2d, kcrop_inout, out, batch, 0, (int)h->e.ops.size()});
}

int capf_backbone_forward(capf_handle* h, void* stream, const float* images_nhwc, int batch) {
    if (!h || !images_nhwc) return CAPF_ERR_INVALID;
    return begin_and_run(h->e, stream, {"capf_backbone_forward", images_nhwc, nullptr, nullptr, nullptr, batch, 0, h->e.n_backbone_ops});
}

int capf_backbone_forward_bn(capf_handle* h, void* stream, const float* images_nhwc, int batch, float momentum) {
    if (!h || !images_nhwc) return CAPF_ERR_INVALID;
    Engine& e = h->e;
    Call c{"capf_backbone_forward_bn", images_nhwc, nullptr, nullptr, nullptr, batch, 0, e.n_backbone_ops};
    c.bn = true;
    c.momentum = momentum;
    if (const int rc = e.begin(c)) return rc;
    e.bn_run = true;                     // (the second op list: Engine::gemm_args, fused_at, exec_op, run_region_grouped)
    e.bn_momentum = momentum;
    const int rc = e.run(static_cast<hipStream_t>(stream), batch, c.first, c.last);
    e.bn_run = false;
    return rc;
}

int capf_forward_train(capf_handle* h, void* stream, const float* images_nhwc, const float* k2d, float* kcrop_inout,
                       int batch, float* out, const float* drop_masks) {
    if (!h || !images_nhwc || !k2d || !kcrop_inout || !out) return CAPF_ERR_INVALID;
    return begin_and_run(h->e, stream, {"capf_forward_train", images_nhwc, k2d, kcrop_inout, out, batch, 0, h->e.n_backbone_ops, true}, drop_masks);
}

int capf_forward_u8(capf_handle* h, void* stream, const uint8_t* images_bgr_u8, const float mean[3], const float* std3, int mode,
                    const float* k2d, float* kcrop_inout, int batch, float* out) {
    if (!h || !k2d || !kcrop_inout || !out) return CAPF_ERR_INVALID;
    return begin_and_run(h->e, stream, {"capf_forward_u8", u8_source(images_bgr_u8, mean, std3, mode, batch), k2d, kcrop_inout, out, batch, 0,
                                        (int)h->e.ops.size()});
}

int capf_backbone_forward_u8(capf_handle* h, void* stream, const uint8_t* images_bgr_u8, const float mean[3], const float* std3, int mode,
                             int batch) {
    if (!h) return CAPF_ERR_INVALID;
    return begin_and_run(h->e, stream, {"capf_backbone_forward_u8", u8_source(images_bgr_u8, mean, std3, mode, batch), nullptr, nullptr, nullptr,
                                        batch, 0, h->e.n_backbone_ops});
}

int capf_forward_train_u8(capf_handle* h, void* stream, const uint8_t* images_bgr_u8, const float mean[3], const float* std3, int mode,
                          const float* k2d, float* kcrop_inout, int batch, float* out, const float* drop_masks) {
    if (!h || !k2d || !kcrop_inout || !out) return CAPF_ERR_INVALID;
    return begin_and_run(h->e, stream, {"capf_forward_train_u8", u8_source(images_bgr_u8, mean, std3, mode, batch), k2d, kcrop_inout, out, batch, 0,
                                        h->e.n_backbone_ops, true}, drop_masks);
}

int capf_lifter_forward(capf_handle* h, void* stream, const float* k2d, float* kcrop_inout, int batch, float* out) {
    if (!h || !k2d || !kcrop_inout || !out) return CAPF_ERR_INVALID;
    return begin_and_run(h->e, stream, {"capf_lifter_forward", {}, k2d, kcrop_inout, out, batch, h->e.n_backbone_ops, (int)h->e.ops.size(), false, true});
}

int capf_lifter_forward_train(capf_handle* h, void* stream, const float* k2d, float* kcrop_inout, int batch, float* out,
                              const float* drop_masks) {
    if (!h || !k2d || !kcrop_inout || !out) return CAPF_ERR_INVALID;
    const int nb = h->e.n_backbone_ops;                    // (an empty span: the training step's lifter is all that runs)
    return begin_and_run(h->e, stream, {"capf_lifter_forward_train", {}, k2d, kcrop_inout, out, batch, nb, nb, true, true}, drop_masks);
}

int capf_backward(capf_handle* h, void* stream, const float* grad_out, int batch, float* flat_grad, const float* drop_masks) {
    if (!h || !grad_out || !flat_grad) return CAPF_ERR_INVALID;
    return h->e.backward(static_cast<hipStream_t>(stream), batch, grad_out, flat_grad, drop_masks);
}

// caller-supplied context maps: fp32 plans only (a 16-bit plan stores feat0..3 in its own element format)
static int maps_f32_only(Engine& e, const char* who) {
    if (!e.b16()) return CAPF_OK;
    e.err = std::string(who) + ": context maps are supplied and differentiated in fp32 only; this handle's compute_dtype is " +
            (e.f16() ? "fp16" : "bf16");
    return CAPF_ERR_UNSUPPORTED;
}

int capf_set_features(capf_handle* h, void* stream, const float* const feat_nhwc[4], int batch) {
    if (!h || !feat_nhwc) return CAPF_ERR_INVALID;
    Engine& e = h->e;
    for (int l = 0; l < e.cfg.levels; ++l)
        if (!feat_nhwc[l]) return CAPF_ERR_INVALID;
    int rc = maps_f32_only(e, "capf_set_features");
    if (rc) return rc;
    if (batch < 1 || batch > capf_max_batch(h)) {
        e.err = "capf_set_features: batch out of range (1..capf_max_batch)";
        return CAPF_ERR_INVALID;
    }
    if ((rc = e.begin({"capf_set_features", {}, nullptr, nullptr, nullptr, batch, 0, 0}))) return rc;      // (no op runs: the copies below write the maps)
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int l = 0; l < e.cfg.levels; ++l) {
        const size_t bytes = sizeof(float) * (size_t)batch * e.feat_H[l] * e.feat_W[l] * e.feat_C[l];
        if (hipMemcpyAsync(e.bptr(e.feat_buf[l], batch), feat_nhwc[l], bytes, hipMemcpyDeviceToDevice, s) != hipSuccess) {
            e.err = "capf_set_features: hipMemcpyAsync failed";
            return CAPF_ERR_HIP;
        }
    }
    e.ses.maps_written(batch);
    return CAPF_OK;
}

int capf_backward_maps(capf_handle* h, void* stream, const float* grad_out, int batch, float* flat_grad, const float* drop_masks,
                       float* const dfeat_nhwc[4]) {
    if (!h || !grad_out || !flat_grad || !dfeat_nhwc || batch < 1) return CAPF_ERR_INVALID;
    Engine& e = h->e;
    for (int l = 0; l < e.cfg.levels; ++l)
        if (!dfeat_nhwc[l]) return CAPF_ERR_INVALID;
    if (int rc = maps_f32_only(e, "capf_backward_maps")) return rc;
    for (int l = 0; l < e.cfg.levels; ++l)
        if ((size_t)dfeat_nhwc[l] & 15) {
            e.err = "capf_backward_maps: dfeat_nhwc pointers must be 16-byte aligned";
            return CAPF_ERR_INVALID;
        }
    return e.backward(static_cast<hipStream_t>(stream), batch, grad_out, flat_grad, drop_masks, dfeat_nhwc);
}

// keypoint gradients: fp32 plans only (the position gradients are formed from fp32 maps; a 16-bit plan stores feat0..3 in its own format)
int capf_backward_points(capf_handle* h, void* stream, const float* grad_out, int batch, float* flat_grad, const float* drop_masks,
                         float* const dfeat_nhwc[4], float* dk2d, float* dref) {
    if (!h || !grad_out || !flat_grad || batch < 1) return CAPF_ERR_INVALID;
    Engine& e = h->e;
    for (int l = 0; dfeat_nhwc && l < e.cfg.levels; ++l)
        if (!dfeat_nhwc[l]) return CAPF_ERR_INVALID;
    if (e.b16()) {
        e.err = std::string("capf_backward_points: keypoint gradients are computed on fp32 plans only; this handle's compute_dtype is ") +
                (e.f16() ? "fp16" : "bf16");
        return CAPF_ERR_UNSUPPORTED;
    }
    for (int l = 0; dfeat_nhwc && l < e.cfg.levels; ++l)
        if ((size_t)dfeat_nhwc[l] & 15) {
            e.err = "capf_backward_points: dfeat_nhwc pointers must be 16-byte aligned";
            return CAPF_ERR_INVALID;
        }
    return e.backward(static_cast<hipStream_t>(stream), batch, grad_out, flat_grad, drop_masks, dfeat_nhwc, dk2d, dref);
}

int capf_set_map_grad_mode(capf_handle* h, int mode) {
    if (!h) return CAPF_ERR_INVALID;
    Engine& e = h->e;
    if (mode != 0 && mode != 1) {
        e.err = "capf_set_map_grad_mode: mode is 0 (atomic) or 1 (ordered)";
        return CAPF_ERR_INVALID;
    }
    if (int rc = maps_f32_only(e, "capf_set_map_grad_mode")) return rc;
    e.map_grad_mode = mode;
    return CAPF_OK;
}

int capf_map_grad_mode(const capf_handle* h) { return h ? h->e.map_grad_mode : -1; }

int64_t capf_train_generation(const capf_handle* h) { return h ? h->e.ses.train_generation : -1; }

int64_t capf_grad_elems(const capf_handle* h) { return h ? h->e.grad_elems : -1; }

int capf_train_h2_matrices(const capf_handle* h) { return h ? (int)h->e.t_h2_specs.size() : 0; }

int capf_grad_info(const capf_handle* h, int index, int64_t* offset) {
    if (!h || index < 0 || index >= (int)h->e.params.size() || !offset) return CAPF_ERR_INVALID;
    *offset = h->e.grad_off[index];
    return CAPF_OK;
}

int capf_mpjpe(void* stream, const float* pred, const float* gt, int rows, float* loss, float* dpred, float grad_scale) {
    if (!pred || !gt || !loss || rows <= 0) return CAPF_ERR_INVALID;
    return capf::launch_mpjpe(pred, gt, rows, loss, dpred, grad_scale, static_cast<hipStream_t>(stream)) == hipSuccess
               ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_mpjpe_nd(void* stream, const float* pred, const float* gt, int rows, int dim, float* loss, float* dpred, float grad_scale) {
    if (!pred || !gt || !loss || rows <= 0 || dim <= 0) return CAPF_ERR_INVALID;
    return capf::launch_mpjpe_nd(pred, gt, rows, dim, loss, dpred, grad_scale, static_cast<hipStream_t>(stream)) == hipSuccess
               ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_adamw_step(void* stream, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                    float beta1, float beta2, float eps, float weight_decay, int step, float grad_scale) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || n <= 0 || step <= 0) return CAPF_ERR_INVALID;
    return capf::launch_adamw(params, grads, exp_avg, exp_avg_sq, n, lr, beta1, beta2, eps, weight_decay, step,
                              static_cast<hipStream_t>(stream), grad_scale) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

size_t capf_optim_ctrl_bytes(void) { return sizeof(capf::OptimCtrl); }

int capf_optim_ctrl_init(void* stream, void* ctrl, int64_t steps_taken) {
    if (!ctrl || (reinterpret_cast<uintptr_t>(ctrl) & 7) || steps_taken < 0) return CAPF_ERR_INVALID;
    return capf::launch_optim_ctrl_init(static_cast<capf::OptimCtrl*>(ctrl), steps_taken, static_cast<hipStream_t>(stream)) == hipSuccess
               ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_grad_sumsq(void* stream, const float* grads, int64_t n, float grad_scale, void* ctrl) {
    if (!grads || n <= 0 || !ctrl || (reinterpret_cast<uintptr_t>(ctrl) & 7)) return CAPF_ERR_INVALID;
    return capf::launch_grad_sumsq(grads, n, grad_scale, static_cast<capf::OptimCtrl*>(ctrl), static_cast<hipStream_t>(stream)) == hipSuccess
               ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_adamw_step_guarded(void* stream, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                            const capf_optim_segment* segments, int n_segments, float beta1, float beta2, float eps, float grad_scale,
                            float max_norm, int64_t attempt, const float* loss, int rows, void* ctrl) {
    if (!params || !grads || !exp_avg || !exp_avg_sq || n <= 0 || !segments || n_segments <= 0 || attempt <= 0 || rows < 0 || !ctrl ||
        (reinterpret_cast<uintptr_t>(ctrl) & 7))
        return CAPF_ERR_INVALID;
    if (n_segments > CAPF_OPTIM_MAX_SEGMENTS) return CAPF_ERR_UNSUPPORTED;
    capf::AdamwSegments segs = {};
    int64_t at = 0;
    for (int k = 0; k < n_segments; ++k) {
        if (segments[k].begin != at || segments[k].end < at) return CAPF_ERR_INVALID;
        at = segments[k].end;
        segs.end[k] = (long)at;
        segs.lr[k] = segments[k].lr;
        segs.wd[k] = segments[k].weight_decay;
    }
    if (at != n) return CAPF_ERR_INVALID;
    segs.count = n_segments;
    return capf::launch_adamw_guarded(params, grads, exp_avg, exp_avg_sq, n, segs, beta1, beta2, eps, grad_scale, max_norm, attempt, loss,
                                      rows, static_cast<capf::OptimCtrl*>(ctrl), static_cast<hipStream_t>(stream)) == hipSuccess
               ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_tensor(const capf_handle* h, const char* name, const void** dev_ptr, int64_t shape[4], int* ndim) {
    if (!h || !name) return CAPF_ERR_INVALID;
    const Engine& e = h->e;
    auto it = e.named.find(name);
    if (it == e.named.end()) return CAPF_ERR_INVALID;
    const capf::NamedTensor& t = it->second;
    if (shape) {
        for (int i = 0; i < 4; ++i) shape[i] = t.shape[i];
        shape[0] = e.ses.last_batch;
    }
    if (ndim) *ndim = t.ndim;
    if (dev_ptr) *dev_ptr = (e.ws && e.ses.last_batch > 0) ? e.bptr(t.buf, e.ses.last_batch) : nullptr;
    return t.is_int;      // 0 fp32, 1 int32, 2 bf16, 3 fp16
}

// ---- stand-alone operators (capf_op_*: op-level tests and micro-benchmarks) ----------------------------------------------------------
static int hip_rc(hipError_t e, int fail = CAPF_ERR_HIP) { return e == hipSuccess ? CAPF_OK : fail; }

static capf_conv_desc conv_desc(const void* x, const void* wp, const float* bias, const void* residual, void* y, int B, int H, int W,
                                int Cin, int Cout, int ks, int stride, int act) {
    return {static_cast<const float*>(x), static_cast<const float*>(wp), bias, static_cast<const float*>(residual), static_cast<float*>(y),
            B, H, W, Cin, Cout, ks, stride, act};
}

// one conv as the launchers take it (padding ks / 2): the packed weights go to the family's slot, Kpad = K rounded up to kround
static capf::GemmArgs conv_args(const capf_conv_desc& d, const float* capf::GemmArgs::*wslot, int kround) {
    capf::GemmArgs a{};
    const int pad = d.ks / 2;
    a.A = d.x; a.*wslot = d.w_packed; a.bias = d.bias; a.res = d.residual; a.out = d.y;
    a.Ho = (d.H + 2 * pad - d.ks) / d.stride + 1;
    a.Wo = (d.W + 2 * pad - d.ks) / d.stride + 1;
    a.M = d.B * a.Ho * a.Wo; a.N = d.Cout; a.K = d.ks * d.ks * d.Cin; a.Kpad = (a.K + kround - 1) / kround * kround;
    a.conv = 1; a.Cin = d.Cin; a.H = d.H; a.W = d.W; a.ks = d.ks; a.stride = d.stride; a.pad = pad;
    a.omap = capf::row_ld(d.Cout); a.rmap = capf::row_ld(d.Cout); a.amap = capf::row_ld(0);
    a.act = d.act;
    return a;
}

// y[M, N] = act(x[M, K] W^T + bias (+ residual)), dense rows
static capf::GemmArgs rows_args(const float* capf::GemmArgs::*wslot, const float* x, const float* w, const float* bias, const float* residual,
                                float* y, int M, int N, int K, int act) {
    capf::GemmArgs a{};
    a.A = x; a.*wslot = w; a.bias = bias; a.res = residual; a.out = y;
    a.M = M; a.N = N; a.K = K; a.Kpad = K;
    a.amap = capf::row_ld(K); a.omap = capf::row_ld(N); a.rmap = capf::row_ld(N);
    a.act = act;
    return a;
}

static bool is_3x3_s1(const capf_conv_desc& d) { return d.ks == 3 && d.stride == 1; }

// the steps every *_group entry point shares: n / d validation, build(d[i], i, args) per problem (a CAPF_* status: the family's own
// checks), one launch
extern "C++" template <class Build, class Launch>
static int conv_group(void* stream, int n, const capf_conv_desc* d, Build build, Launch launch) {
    if (n <= 0 || n > capf::MAXG || !d) return CAPF_ERR_INVALID;
    capf::GemmArgs g[capf::MAXG];
    for (int i = 0; i < n; ++i)
        if (const int rc = build(d[i], i, g[i])) return rc;
    return hip_rc(launch(g, n, static_cast<hipStream_t>(stream)));
}

// the 3x3 / stride-1 tiles that take their weights in Wp3 (bf16 2-D halo, fp32 split pieces; x3_h2: the pieces are the two-fp16-piece tile's)
static int wp3_build(const capf_conv_desc& d, capf::GemmArgs& a, bool (*ok)(const capf::GemmArgs&), int x3_h2) {
    if (!is_3x3_s1(d)) return CAPF_ERR_UNSUPPORTED;
    a = conv_args(d, &capf::GemmArgs::Wp3, 1);
    a.x3_h2 = x3_h2;
    return ok(a) ? CAPF_OK : CAPF_ERR_UNSUPPORTED;
}

int capf_op_pack_conv(void* stream, const float* w, const float* gamma, const float* beta, const float* mean,
                      const float* var, float eps, float* wp, float* bias, int Cout, int Cin, int ks) {
    const int Kpad = (ks * ks * Cin + 31) / 32 * 32;
    return hip_rc(capf::launch_pack_conv(w, gamma, beta, mean, var, eps, wp, bias, Cout, Cin, ks, Kpad, static_cast<hipStream_t>(stream)));
}

int capf_op_conv(void* stream, const float* x, const float* wp, const float* bias, const float* residual, float* y,
                 int B, int H, int W, int Cin, int Cout, int ks, int stride, int act) {
    const capf::GemmArgs a = conv_args(conv_desc(x, wp, bias, residual, y, B, H, W, Cin, Cout, ks, stride, act), &capf::GemmArgs::Wp, 32);
    return hip_rc(capf::launch_gemm_f32(a, static_cast<hipStream_t>(stream)));
}

int capf_op_conv_group(void* stream, int n, const capf_conv_desc* d) {
    return conv_group(stream, n, d, [](const capf_conv_desc& c, int, capf::GemmArgs& a) {
        a = conv_args(c, &capf::GemmArgs::Wp, 32);
        return capf::gemm_f32_groupable(a) ? CAPF_OK : CAPF_ERR_UNSUPPORTED;
    }, capf::launch_gemm_f32_group);
}

int capf_op_pack_conv_wino(void* stream, const float* w, const float* gamma, const float* beta, const float* mean,
                           const float* var, float eps, float* wp, float* bias, int Cout, int Cin, int variant) {
    return hip_rc(capf::launch_pack_conv_wino(w, gamma, beta, mean, var, eps, wp, bias, Cout, Cin, static_cast<hipStream_t>(stream), variant),
                  CAPF_ERR_UNSUPPORTED);
}

// the variant rides in the packed-weight pitch: 12 Cin for F(2,3), 18 Cin for F(4,3)
static int wino_build(const capf_conv_desc& d, capf::GemmArgs& a, int variant) {
    if (!is_3x3_s1(d)) return CAPF_ERR_UNSUPPORTED;
    a = conv_args(d, &capf::GemmArgs::Wp, 1);
    a.Kpad = (variant == 43 ? 18 : 12) * d.Cin;
    return capf::gemm_wino_ok(a) ? CAPF_OK : CAPF_ERR_UNSUPPORTED;
}

static bool wino_variant(int variant) { return variant == 23 || variant == 43; }

int capf_op_conv_wino(void* stream, const float* x, const float* wp, const float* bias, const float* residual, float* y, int B,
                      int H, int W, int Cin, int Cout, int act, int variant) {
    capf::GemmArgs a;
    if (!wino_variant(variant) || wino_build(conv_desc(x, wp, bias, residual, y, B, H, W, Cin, Cout, 3, 1, act), a, variant))
        return CAPF_ERR_UNSUPPORTED;
    return hip_rc(capf::launch_gemm_wino(a, static_cast<hipStream_t>(stream)));
}

int capf_op_conv_wino_group(void* stream, int n, const capf_conv_desc* d, int variant) {
    if (!wino_variant(variant)) return CAPF_ERR_INVALID;
    return conv_group(stream, n, d, [variant](const capf_conv_desc& c, int, capf::GemmArgs& a) { return wino_build(c, a, variant); },
                      capf::launch_gemm_wino_group);
}

int64_t capf_op_f32h2_gemm_pack_elems(int N, int K) { return N > 0 && K > 0 ? capf::f32h2_gemm_pack_elems(N, (K + 31) / 32 * 32) : 0; }

int capf_op_pack_f32h2_gemm(void* stream, const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                            float eps, float* wp, float* bias, int N, int Cin, int ks, int K) {
    if (!w || !wp || N <= 0 || (N & 3) || K <= 0 || (ks > 0 && K != ks * ks * Cin)) return CAPF_ERR_UNSUPPORTED;
    return hip_rc(capf::launch_pack_f32h2_gemm(w, gamma, beta, mean, var, eps, wp, bias, N, Cin, ks, K, (K + 31) / 32 * 32,
                                               static_cast<hipStream_t>(stream)));
}

static int h2g_build(const capf_conv_desc& d, capf::GemmArgs& a) {
    if (d.ks < 1 || d.stride < 1) return CAPF_ERR_INVALID;
    a = conv_args(d, &capf::GemmArgs::Wh2, 32);
    return capf::gemm_f32h2g_ok(a) ? CAPF_OK : CAPF_ERR_UNSUPPORTED;
}

int capf_op_conv_f32h2g(void* stream, const float* x, const float* wp, const float* bias, const float* residual, float* y,
                        int B, int H, int W, int Cin, int Cout, int ks, int stride, int act) {
    capf::GemmArgs a;
    if (const int rc = h2g_build(conv_desc(x, wp, bias, residual, y, B, H, W, Cin, Cout, ks, stride, act), a)) return rc;
    return hip_rc(capf::launch_gemm_f32h2g(a, static_cast<hipStream_t>(stream)));
}

int capf_op_conv_f32h2g_group(void* stream, int n, const capf_conv_desc* d) {
    return conv_group(stream, n, d, [](const capf_conv_desc& c, int, capf::GemmArgs& a) { return h2g_build(c, a); },
                      capf::launch_gemm_f32h2g_group);
}

int capf_op_linear_f32h2g(void* stream, const float* x, const float* wp, const float* bias, const float* residual, float* y,
                          int M, int N, int K, int act) {
    if (K % 32 != 0) return CAPF_ERR_UNSUPPORTED;
    const capf::GemmArgs a = rows_args(&capf::GemmArgs::Wh2, x, wp, bias, residual, y, M, N, K, act);
    if (!capf::gemm_f32h2g_ok(a)) return CAPF_ERR_UNSUPPORTED;
    return hip_rc(capf::launch_gemm_f32h2g(a, static_cast<hipStream_t>(stream)));
}

int capf_op_wgrad(void* stream, const float* dY, const float* X, int M, int N, int K, float* dw_db, int two_piece) {
    if (!dY || !X || !dw_db || M <= 0 || N <= 0 || K <= 0 || N % 4 || K % 4 || (two_piece && (N % 128 || K % 128))) return CAPF_ERR_UNSUPPORTED;
    return hip_rc(capf::launch_wgrad_tn(dY, N, X, K, M, N, K, dw_db, (long)N * K + N, 1, 1, static_cast<hipStream_t>(stream), two_piece != 0));
}

int capf_op_linear_ln_f32h2g(void* stream, const float* x, const float* ln_gamma, const float* ln_beta, float eps, const float* wp,
                             const float* bias, const float* residual, float* y, int M, int N, int K, int act) {
    if (K % 32 != 0 || !ln_gamma || !ln_beta) return CAPF_ERR_UNSUPPORTED;
    capf::GemmArgs a = rows_args(&capf::GemmArgs::Wh2, x, wp, bias, residual, y, M, N, K, act);
    a.ln_g = ln_gamma; a.ln_b = ln_beta; a.ln_eps = eps;
    if (!capf::gemm_f32h2g_ok(a)) return CAPF_ERR_UNSUPPORTED;
    return hip_rc(capf::launch_gemm_f32h2g(a, static_cast<hipStream_t>(stream)));
}

int capf_op_linear(void* stream, const float* x, const float* w, const float* bias, const float* residual, float* y,
                   int M, int N, int K, int act) {
    if (K % 32 != 0) return CAPF_ERR_UNSUPPORTED;
    return hip_rc(capf::launch_gemm_f32(rows_args(&capf::GemmArgs::Wp, x, w, bias, residual, y, M, N, K, act), static_cast<hipStream_t>(stream)));
}

size_t capf_op_bn_stats_scratch_bytes(int64_t rows, int C) { return capf::bn_scratch_elems((long)rows, C) * sizeof(float); }

int capf_op_bn_stats(void* stream, const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps, float momentum,
                     float* running_mean, float* running_var, float* scale, float* shift, void* scratch, size_t scratch_bytes) {
    if (!x || !gamma || !beta || !scale || !shift || !scratch || rows < 2) return CAPF_ERR_INVALID;      // (rows < 2: no variance of one value)
    const size_t need = capf_op_bn_stats_scratch_bytes(rows, C);
    if (need == 0) return CAPF_ERR_UNSUPPORTED;
    if (scratch_bytes < need || (reinterpret_cast<uintptr_t>(scratch) & 7)) return CAPF_ERR_INVALID;
    capf::BnStatsArgs a{};
    a.x = x; a.gamma = gamma; a.beta = beta; a.rmean = running_mean; a.rvar = running_var;
    a.part = static_cast<double*>(scratch); a.scale = scale; a.shift = shift;
    a.rows = (long)rows; a.C = C; a.eps = eps; a.momentum = momentum;
    return capf::launch_bn_stats_group(&a, 1, static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_op_bn_apply(void* stream, const float* x, const float* scale, const float* shift, const float* residual, float* y, int64_t rows, int C,
                     int act) {
    if (!x || !scale || !shift || !y || rows < 1 || (act != 0 && act != 1)) return CAPF_ERR_INVALID;
    if (C < 4 || C % 4 != 0 || C > 1024 || rows * (C / 4) >= (int64_t(1) << 31)) return CAPF_ERR_UNSUPPORTED;
    const capf::BnApplyArgs a{x, residual, y, scale, shift, (long)rows, C, act};
    return capf::launch_bn_apply_group(&a, 1, static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_op_bilinear_corners(void* stream, const float* grid, int n, int H, int W, int border, int32_t* idx, float* frac) {
    if (!grid || !idx || !frac || n <= 0 || H <= 0 || W <= 0) return CAPF_ERR_INVALID;
    return capf::launch_bilinear_corners(grid, n, H, W, border, idx, frac, static_cast<hipStream_t>(stream)) == hipSuccess
               ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_op_pack_conv_bf16(void* stream, const float* w, const float* gamma, const float* beta, const float* mean,
                           const float* var, float eps, void* wp, float* bias, int Cout, int Cin, int ks) {
    const int Kpad = (ks * ks * Cin + 63) / 64 * 64;
    return hip_rc(capf::launch_pack_conv_bf16(w, gamma, beta, mean, var, eps, wp, bias, Cout, Cin, ks, Kpad, static_cast<hipStream_t>(stream)));
}

// (the bf16 single-conv entry points report a failed launch as CAPF_ERR_UNSUPPORTED, as they always have)
int capf_op_conv_bf16(void* stream, const void* x, const void* wp, const float* bias, const void* residual, void* y, int B,
                      int H, int W, int Cin, int Cout, int ks, int stride, int act) {
    const capf::GemmArgs a = conv_args(conv_desc(x, wp, bias, residual, y, B, H, W, Cin, Cout, ks, stride, act), &capf::GemmArgs::Wp, 64);
    return hip_rc(capf::launch_gemm_bf16(a, static_cast<hipStream_t>(stream)), CAPF_ERR_UNSUPPORTED);
}

int capf_op_conv_bf16_rh_width(int Cin) {
    return capf::gemm_bf16_rh_cw(conv_args(conv_desc(nullptr, nullptr, nullptr, nullptr, nullptr, 1, 8, 8, Cin, 8, 3, 1, 0), &capf::GemmArgs::Wp, 1));
}

int capf_op_pack_conv_bf16_rh(void* stream, const float* w, const float* gamma, const float* beta, const float* mean,
                              const float* var, float eps, void* wp, float* bias, int Cout, int Cin) {
    const int cw = capf_op_conv_bf16_rh_width(Cin);
    if (!cw) return CAPF_ERR_UNSUPPORTED;
    return hip_rc(capf::launch_pack_conv_bf16_rh(w, gamma, beta, mean, var, eps, wp, bias, Cout, Cin, cw, static_cast<hipStream_t>(stream)));
}

int capf_op_conv_bf16_rh(void* stream, const void* x, const void* wp, const float* bias, const void* residual, void* y, int B,
                         int H, int W, int Cin, int Cout, int act) {
    const capf::GemmArgs a = conv_args(conv_desc(x, wp, bias, residual, y, B, H, W, Cin, Cout, 3, 1, act), &capf::GemmArgs::Wp, 1);
    return hip_rc(capf::launch_gemm_bf16_rh(a, static_cast<hipStream_t>(stream)), CAPF_ERR_UNSUPPORTED);
}

int64_t capf_op_conv_bf16_ws_pack_elems(int Cout, int Cin) { return Cin % 16 == 0 && Cout > 0 ? capf::bf16_ws_pack_elems(Cout, Cin) : 0; }

int capf_op_pack_conv_bf16_ws(void* stream, const float* w, const float* gamma, const float* beta, const float* mean,
                              const float* var, float eps, void* wp, float* bias, int Cout, int Cin) {
    if (!w || !wp || Cin % 16 != 0 || Cout % 8 != 0) return CAPF_ERR_UNSUPPORTED;
    return hip_rc(capf::launch_pack_conv_bf16_ws(w, gamma, beta, mean, var, eps, wp, bias, Cout, Cin, static_cast<hipStream_t>(stream)));
}

int capf_op_conv_bf16_ws_group(void* stream, int n, const capf_conv_desc* d) {
    return conv_group(stream, n, d, [](const capf_conv_desc& c, int, capf::GemmArgs& a) { return wp3_build(c, a, capf::gemm_bf16_ws_ok, 0); },
                      capf::launch_gemm_bf16_ws_group);
}

int64_t capf_op_conv_f32x3_pack_elems(int Cout, int Cin) { return Cin % 16 == 0 && Cout > 0 ? capf::f32x3_pack_elems(Cout, Cin) : 0; }

int capf_op_pack_conv_f32x3(void* stream, const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                            float eps, void* wp, float* bias, int Cout, int Cin) {
    if (!w || !wp || Cin % 16 != 0 || Cout % 4 != 0) return CAPF_ERR_UNSUPPORTED;
    return hip_rc(capf::launch_pack_conv_f32x3(w, gamma, beta, mean, var, eps, wp, bias, Cout, Cin, static_cast<hipStream_t>(stream)));
}

int capf_op_conv_f32x3_group(void* stream, int n, const capf_conv_desc* d) {
    return conv_group(stream, n, d, [](const capf_conv_desc& c, int, capf::GemmArgs& a) { return wp3_build(c, a, capf::gemm_f32x3_ok, 0); },
                      capf::launch_gemm_f32x3_group);
}

int64_t capf_op_conv_f32h2_pack_elems(int Cout, int Cin) { return Cin % 16 == 0 && Cout > 0 ? capf::f32h2_pack_elems(Cout, Cin) : 0; }

int capf_op_pack_conv_f32h2(void* stream, const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                            float eps, void* wp, float* bias, int Cout, int Cin) {
    if (!w || !wp || Cin % 16 != 0 || Cout % 4 != 0) return CAPF_ERR_UNSUPPORTED;
    return hip_rc(capf::launch_pack_conv_f32h2(w, gamma, beta, mean, var, eps, wp, bias, Cout, Cin, static_cast<hipStream_t>(stream)));
}

int capf_op_conv_f32h2_group(void* stream, int n, const capf_conv_desc* d) {
    return conv_group(stream, n, d, [](const capf_conv_desc& c, int, capf::GemmArgs& a) { return wp3_build(c, a, capf::gemm_f32h2_ok, 1); },
                      capf::launch_gemm_f32h2_group);
}

int capf_op_conv_f32h2_tiles(int B, int H, int W, int* tile_pixels) { return capf::f32h2_tiles_m(B, H, W, tile_pixels); }

int capf_op_conv_f32h2_planes(void* stream, const capf_conv_desc* d, const int32_t* exps_in, int32_t* exps_out) {
    if (!d || !is_3x3_s1(*d) || (exps_in && exps_out)) return CAPF_ERR_UNSUPPORTED;
    capf::GemmArgs g = conv_args(*d, &capf::GemmArgs::Wp3, 1);
    g.x3_h2 = 1; g.h2_ein = exps_in; g.h2_eout = exps_out;
    if (!capf::gemm_f32h2_ok(g)) return CAPF_ERR_UNSUPPORTED;
    const hipError_t e = capf::launch_gemm_f32h2_group(&g, 1, static_cast<hipStream_t>(stream));
    return hip_rc(e, e == hipErrorInvalidValue ? CAPF_ERR_UNSUPPORTED : CAPF_ERR_HIP);
}

int capf_op_conv_bf16_group(void* stream, int n, const capf_conv_desc* d, const void* const* w_rh, int32_t* variant) {
    return conv_group(stream, n, d, [w_rh](const capf_conv_desc& c, int i, capf::GemmArgs& a) {
        a = conv_args(c, &capf::GemmArgs::Wp, 64);
        a.Wp2 = w_rh ? static_cast<const float*>(w_rh[i]) : nullptr;
        return capf::gemm_bf16_groupable(a) ? CAPF_OK : CAPF_ERR_UNSUPPORTED;
    }, [variant](const capf::GemmArgs* g, int n, hipStream_t s) {
        int v = -1;
        const hipError_t e = capf::launch_gemm_bf16_group(g, n, s, &v);
        if (variant) *variant = v;
        return e;
    });
}

int capf_op_linear_bf16(void* stream, const void* x_bf16, const void* w_bf16, const float* bias, const float* residual, void* y,
                        int M, int N, int K, int gelu_bf16_out) {
    if (!x_bf16 || !w_bf16 || !y || K % 64 != 0) return CAPF_ERR_INVALID;
    return capf::launch_gemm_bf16_rows(x_bf16, w_bf16, bias, M, N, K, K, static_cast<float*>(y), capf::row_ld(N), residual,
                                       capf::row_ld(N), gelu_bf16_out, static_cast<hipStream_t>(stream)) == hipSuccess
               ? CAPF_OK : CAPF_ERR_UNSUPPORTED;
}

// ---- the 16-bit kernel families for either element format (dtype = CAPF_BF16 or CAPF_F16): the entries above are these at CAPF_BF16
static bool dtype16(int dtype) { return dtype == CAPF_BF16 || dtype == CAPF_F16; }
// a stand-alone 16-bit stem op is an op of the 16-bit stem kernels: a problem they do not take is refused, not handed on to the fp32 ones
static bool stem_op_takes(const capf::GemmArgs& a) { return !a.out_bf16 || capf::stem_is_16bit(capf::gemm_stem_route(a).kernel); }

int capf_op_pack_conv_16(void* stream, const float* w, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                         void* wp, float* bias, int Cout, int Cin, int ks, int layout, int dtype) {
    if (!w || !wp || !dtype16(dtype) || Cout <= 0 || Cin <= 0) return CAPF_ERR_INVALID;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int f16 = dtype == CAPF_F16;
    switch (layout) {
        case 0: return hip_rc(capf::launch_pack_conv_bf16(w, gamma, beta, mean, var, eps, wp, bias, Cout, Cin, ks, (ks * ks * Cin + 63) / 64 * 64, s, f16));
        case 1: {
            const int cw = ks == 3 ? capf_op_conv_bf16_rh_width(Cin) : 0;
            if (!cw) return CAPF_ERR_UNSUPPORTED;
            return hip_rc(capf::launch_pack_conv_bf16_rh(w, gamma, beta, mean, var, eps, wp, bias, Cout, Cin, cw, s, f16));
        }
        case 2:
            if (ks != 3 || Cin % 16 != 0 || Cout % 8 != 0) return CAPF_ERR_UNSUPPORTED;
            return hip_rc(capf::launch_pack_conv_bf16_ws(w, gamma, beta, mean, var, eps, wp, bias, Cout, Cin, s, f16));
        default: return CAPF_ERR_INVALID;
    }
}

int capf_op_conv_16(void* stream, const void* x, const void* wp, const float* bias, const void* residual, void* y, int B, int H, int W,
                    int Cin, int Cout, int ks, int stride, int act, int dtype) {
    if (!dtype16(dtype)) return CAPF_ERR_INVALID;
    if (Cin % 8 != 0) {         // the stem of a 16-bit plan: fp32 image and fp32 pack (capf_op_pack_conv) in, both rounded on their way into LDS; 16-bit result
        if (residual) return CAPF_ERR_UNSUPPORTED;
        capf::GemmArgs a = conv_args(conv_desc(x, wp, bias, nullptr, y, B, H, W, Cin, Cout, ks, stride, act), &capf::GemmArgs::Wp, 32);
        a.out_bf16 = 1;
        a.f16 = dtype == CAPF_F16;
        if (!stem_op_takes(a)) return CAPF_ERR_UNSUPPORTED;
        return hip_rc(capf::launch_gemm_stem(a, nullptr, static_cast<hipStream_t>(stream)), CAPF_ERR_UNSUPPORTED);
    }
    capf::GemmArgs a = conv_args(conv_desc(x, wp, bias, residual, y, B, H, W, Cin, Cout, ks, stride, act), &capf::GemmArgs::Wp, 64);
    a.f16 = dtype == CAPF_F16;
    return hip_rc(capf::launch_gemm_bf16(a, static_cast<hipStream_t>(stream)), CAPF_ERR_UNSUPPORTED);
}

int capf_op_conv_16_group(void* stream, int n, const capf_conv_desc* d, const void* const* w_rh, int32_t* variant, int dtype) {
    if (!dtype16(dtype)) return CAPF_ERR_INVALID;
    return conv_group(stream, n, d, [w_rh, dtype](const capf_conv_desc& c, int i, capf::GemmArgs& a) {
        a = conv_args(c, &capf::GemmArgs::Wp, 64);
        a.Wp2 = w_rh ? static_cast<const float*>(w_rh[i]) : nullptr;
        a.f16 = dtype == CAPF_F16;
        return capf::gemm_bf16_groupable(a) ? CAPF_OK : CAPF_ERR_UNSUPPORTED;
    }, [variant](const capf::GemmArgs* g, int n, hipStream_t s) {
        int v = -1;
        const hipError_t e = capf::launch_gemm_bf16_group(g, n, s, &v);
        if (variant) *variant = v;
        return e;
    });
}

int capf_op_conv_16_ws_group(void* stream, int n, const capf_conv_desc* d, int dtype) {
    if (!dtype16(dtype)) return CAPF_ERR_INVALID;
    return conv_group(stream, n, d, [dtype](const capf_conv_desc& c, int, capf::GemmArgs& a) {
        const int rc = wp3_build(c, a, capf::gemm_bf16_ws_ok, 0);
        a.f16 = dtype == CAPF_F16;
        return rc;
    }, capf::launch_gemm_bf16_ws_group);
}

int capf_op_linear_16(void* stream, const void* x, const void* w, const float* bias, const float* residual, void* y, int M, int N, int K,
                      int gelu_out16, int dtype) {
    if (!x || !w || !y || K % 64 != 0 || !dtype16(dtype)) return CAPF_ERR_INVALID;
    return hip_rc(capf::launch_gemm_bf16_rows(x, w, bias, M, N, K, K, static_cast<float*>(y), capf::row_ld(N), residual, capf::row_ld(N), gelu_out16,
                                              static_cast<hipStream_t>(stream), dtype == CAPF_F16), CAPF_ERR_UNSUPPORTED);
}

int capf_op_bneck_16(void* stream, const void* x, const void* const w[4], const float* const bias[4], void* t1, void* t2, void* shortcut, void* y,
                     int B, int H, int W, int tap, int dtype) {
    if (!x || !w || !bias || !t1 || !t2 || !y || !dtype16(dtype) || B <= 0) return CAPF_ERR_INVALID;
    const bool first = w[3] != nullptr;                  // a downsample conv: the first bottleneck (64 channels in), else the identity one (256 in)
    if (first && !shortcut) return CAPF_ERR_INVALID;
    const int cin = first ? 64 : 256;
    capf::GemmArgs c1 = conv_args(conv_desc(x, w[0], bias[0], nullptr, t1, B, H, W, cin, 64, 1, 1, capf::ACT_RELU), &capf::GemmArgs::Wp, 64);
    capf::GemmArgs c2 = conv_args(conv_desc(t1, w[1], bias[1], nullptr, t2, B, H, W, 64, 64, 3, 1, capf::ACT_RELU), &capf::GemmArgs::Wp, 64);
    capf::GemmArgs c3 = conv_args(conv_desc(t2, w[2], bias[2], first ? shortcut : x, y, B, H, W, 64, 256, 1, 1, capf::ACT_RELU), &capf::GemmArgs::Wp, 64);
    capf::GemmArgs ds = conv_args(conv_desc(x, w[3], bias[3], nullptr, shortcut, B, H, W, 64, 256, 1, 1, capf::ACT_NONE), &capf::GemmArgs::Wp, 64);
    c1.f16 = c2.f16 = c3.f16 = ds.f16 = dtype == CAPF_F16;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (first) return hip_rc(capf::launch_bneck0_bf16(c1, c2, ds, c3, tap != 0, s), CAPF_ERR_UNSUPPORTED);
    return hip_rc(capf::launch_bneck1_bf16(c1, c2, c3, tap != 0, s), CAPF_ERR_UNSUPPORTED);
}

int capf_debug_f16_round(const float* in, uint16_t* out, int n) {
    if (!in || !out || n < 0) return CAPF_ERR_INVALID;
    for (int i = 0; i + 1 < n; i += 2) {                   // the two-element pack, as the kernels' epilogues store; an odd tail through the scalar form
        const unsigned u = capf::F16Fmt::pack2(in[i], in[i + 1]);
        out[i] = (uint16_t)(u & 0xFFFFu);
        out[i + 1] = (uint16_t)(u >> 16);
    }
    if (n & 1) out[n - 1] = capf::F16Fmt::narrow(in[n - 1]);
    return CAPF_OK;
}

int capf_preprocess(void* stream, const uint8_t* images_bgr, int batch, int height, int width, const float mean[3],
                    const float* std3, int mode, float* images_out, const float* gt_in, float* gt_out, const float* k2d_in,
                    float* k2d_out, const float* kcrop_in, float* kcrop_out) {
    if (!images_bgr || !images_out || !k2d_in || !k2d_out || !kcrop_in || !kcrop_out || !mean || batch <= 0 || mode < 0 ||
        mode > 2 || (gt_in && !gt_out))
        return CAPF_ERR_INVALID;
    return capf::launch_preprocess(images_bgr, batch, height, width, mean, std3, mode, images_out, gt_in, gt_out, k2d_in,
                                   k2d_out, kcrop_in, kcrop_out, static_cast<hipStream_t>(stream)) == hipSuccess
               ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_preprocess_points(void* stream, int batch, int mode, const float* gt_in, float* gt_out, const float* k2d_in, float* k2d_out,
                           const float* kcrop_in, float* kcrop_out) {
    if (!k2d_in || !k2d_out || !kcrop_in || !kcrop_out || batch <= 0 || mode < 0 || mode > 2 || (gt_in && !gt_out)) return CAPF_ERR_INVALID;
    return hip_rc(capf::launch_preprocess_points(batch, mode, gt_in, gt_out, k2d_in, k2d_out, kcrop_in, kcrop_out, static_cast<hipStream_t>(stream)));
}

int capf_input_rule_host(const uint8_t* u, int n, int channel, const float mean[3], const float* std3, float* out) {
    if (!u || !out || !mean || n < 0 || channel < 0 || channel > 2) return CAPF_ERR_INVALID;
    for (int i = 0; i < n; ++i) out[i] = capf::pixel_rule(u[i], channel, mean, std3);
    return CAPF_OK;
}

// the stem conv as the plan's stem op runs it from a uint8 crop: the float op's problem (capf_op_conv / capf_op_conv_16's Cin = 3 branch) with the
// image descriptor beside it, through the same dispatch
static int conv_u8_args(const float* wp, const float* bias, void* y, int Bsrc, int mode, int H, int W, int Cout, int ks, int stride, int act,
                        const float* mean, const float* std3, int out_dtype, capf::GemmArgs& a, capf::U8Input& in) {
    if (Bsrc <= 0 || mode < 0 || mode > 2 || H <= 0 || W <= 0 || Cout <= 0 || ks <= 0 || stride <= 0 || !mean ||
        (out_dtype != CAPF_F32 && !dtype16(out_dtype)))
        return CAPF_ERR_INVALID;
    const int frames = mode == 2 ? 2 * Bsrc : Bsrc;
    a = conv_args(conv_desc(nullptr, wp, bias, nullptr, y, frames, H, W, 3, Cout, ks, stride, act), &capf::GemmArgs::Wp, 32);
    if (out_dtype != CAPF_F32) { a.out_bf16 = 1; a.f16 = out_dtype == CAPF_F16; }
    in = capf::U8Input{};
    in.Bsrc = Bsrc; in.mode = mode;
    for (int c = 0; c < 3; ++c) { in.mean[c] = mean[c]; in.stdv[c] = std3 ? std3[c] : 1.f; }
    in.use_std = std3 ? 1 : 0;
    return CAPF_OK;
}

int capf_op_conv_u8(void* stream, const uint8_t* images_bgr_u8, const float* wp, const float* bias, void* y, int Bsrc, int mode, int H, int W,
                    int Cout, int ks, int stride, int act, const float mean[3], const float* std3, int out_dtype) {
    if (!images_bgr_u8 || !wp || !y) return CAPF_ERR_INVALID;
    capf::GemmArgs a;
    capf::U8Input in;
    if (const int rc = conv_u8_args(wp, bias, y, Bsrc, mode, H, W, Cout, ks, stride, act, mean, std3, out_dtype, a, in)) return rc;
    in.img = images_bgr_u8;
    if (!stem_op_takes(a)) return CAPF_ERR_UNSUPPORTED;
    return hip_rc(capf::launch_gemm_stem(a, &in, static_cast<hipStream_t>(stream)), CAPF_ERR_UNSUPPORTED);
}

const char* capf_op_conv_u8_kernel_name(int Bsrc, int mode, int H, int W, int Cout, int ks, int stride, int out_dtype) {
    static const float zero[3] = {0.f, 0.f, 0.f};
    capf::GemmArgs a;
    capf::U8Input in;
    if (conv_u8_args(nullptr, nullptr, nullptr, Bsrc, mode, H, W, Cout, ks, stride, 0, zero, nullptr, out_dtype, a, in)) return "";
    return stem_op_takes(a) ? capf::gemm_stem_kernel_name(a, true) : "";
}

// ... and of the float stem op of the same shape at B frames (capf_op_conv; capf_op_conv_16's Cin = 3 branch)
const char* capf_op_conv_stem_kernel_name(int B, int H, int W, int Cout, int ks, int stride, int out_dtype) {
    static const float zero[3] = {0.f, 0.f, 0.f};
    capf::GemmArgs a;
    capf::U8Input in;
    if (conv_u8_args(nullptr, nullptr, nullptr, B, 0, H, W, Cout, ks, stride, 0, zero, nullptr, out_dtype, a, in)) return "";
    return stem_op_takes(a) ? capf::gemm_stem_kernel_name(a, false) : "";
}

int capf_fliptest_fuse(void* stream, const float* pred2, int batch, float* out) {
    if (!pred2 || !out || batch <= 0) return CAPF_ERR_INVALID;
    return capf::launch_fliptest_fuse(pred2, batch, out, static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_fliptest_fuse_swap(void* stream, const float* pred2, int batch, int joints, const int32_t* swap, float* out) {
    if (!pred2 || !out || batch <= 0 || !capf::swap_table_ok(swap, joints)) return CAPF_ERR_INVALID;
    return capf::launch_fliptest_fuse_swap(pred2, batch, joints, swap, out, static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_affine_from_center_scale(const double center[2], const double scale[2], int out_w, int out_h, double m[6]) {
    if (!center || !scale || !m || out_w <= 1 || out_h <= 1) return CAPF_ERR_INVALID;
    return capf::affine_from_center_scale(center, scale, out_w, out_h, m) ? CAPF_OK : CAPF_ERR_INVALID;
}

int capf_warp_affine(void* stream, const uint8_t* const* frames, const int32_t* dims, const double* m, int batch, int out_h,
                     int out_w, uint8_t* out) {
    if (!frames || !dims || !m || !out || batch <= 0 || out_h <= 0 || out_w <= 0) return CAPF_ERR_INVALID;
    return capf::launch_warp_affine_u8(frames, dims, m, out, batch, out_h, out_w, static_cast<hipStream_t>(stream)) == hipSuccess
               ? CAPF_OK : CAPF_ERR_HIP;
}

// ---- erase_image for crop batches (erase.hip): every argument is judged here, before anything is launched ----
size_t capf_erase_scratch_bytes(int batch, int patches) {
    if (batch < 1 || patches < 1 || patches > capf::MAX_JOINTS) return 0;
    return (size_t)batch * (size_t)patches * capf::ERASE_PATCH_BYTES;
}

int capf_erase_patches(void* stream, const uint8_t* images, int batch, int height, int width, const float* centers, const uint8_t* mask,
                       int patches, int size, int use_mean, uint8_t* out, void* scratch, size_t scratch_bytes) {
    if (!images || !centers || !out || !scratch || batch < 1 || height < 1 || width < 1 || patches < 1 || size < 0) return CAPF_ERR_INVALID;
    const long long frame = (long long)height * width * 3, per_frame = (frame / 3 + 255) / 256;          // (the pixel-per-thread grid is the larger one)
    if (patches > capf::MAX_JOINTS || frame > 0x7fffffffLL || per_frame * batch > 0x7fffffffLL) return CAPF_ERR_UNSUPPORTED;
    if (scratch_bytes < capf_erase_scratch_bytes(batch, patches) || (reinterpret_cast<uintptr_t>(scratch) & 15)) return CAPF_ERR_INVALID;
    // out is images itself or shares no byte with it; the scratch shares none with either
    const uintptr_t a = reinterpret_cast<uintptr_t>(images), o = reinterpret_cast<uintptr_t>(out), w = reinterpret_cast<uintptr_t>(scratch);
    const uintptr_t n = (uintptr_t)frame * (uintptr_t)batch, nw = capf_erase_scratch_bytes(batch, patches);
    if (o != a && o < a + n && a < o + n) return CAPF_ERR_INVALID;
    if ((w < a + n && a < w + nw) || (w < o + n && o < w + nw)) return CAPF_ERR_INVALID;
    return capf::launch_erase_patches(images, batch, height, width, centers, mask, patches, size, use_mean, out, scratch,
                                      static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_pose_errors(void* stream, const float* pred, const float* gt, int n, int joints, const int32_t* prev, float* err) {
    if (!pred || !gt || !err || n <= 0 || joints <= 0) return CAPF_ERR_INVALID;
    hipError_t r = capf::launch_pose_errors(pred, gt, n, joints, prev, err, static_cast<hipStream_t>(stream));
    return r == hipSuccess ? CAPF_OK : (r == hipErrorInvalidValue ? CAPF_ERR_UNSUPPORTED : CAPF_ERR_HIP);
}

int capf_segment_sums(void* stream, const float* err, const int32_t* segment, const int32_t* prev, int n, int n_segments,
                      double* sums, int32_t* counts) {
    if (!err || !sums || !counts || n <= 0 || n_segments <= 0 || (n_segments > 1 && !segment)) return CAPF_ERR_INVALID;
    return capf::launch_segment_sums(err, segment, prev, n, n_segments, sums, counts, static_cast<hipStream_t>(stream)) == hipSuccess
               ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_pck_counts(void* stream, const float* pred, const float* gt, int n, int joints, int root, double to_mm, const int32_t* segment,
                    int n_segments, int32_t* counts, double* mpjpe_sums, int32_t* frames) {
    if (!counts || !mpjpe_sums || !frames || n < 0 || (n > 0 && (!pred || !gt)) || joints <= 0 || joints > 32 || root < 0 ||
        root >= joints || n_segments <= 0 || (n_segments > 1 && n > 0 && !segment) || !(to_mm > 0.0))
        return CAPF_ERR_INVALID;
    return capf::launch_pck_counts(pred, gt, n, joints, root, to_mm, segment, n_segments, counts, mpjpe_sums, frames,
                                   static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_pck2d_counts(void* stream, const float* pred, const float* gt, int n, int joints, const float* norm, const float* weight,
                      const double* thresholds, int n_thresholds, int strict, const int32_t* segment, int n_segments, int32_t* counts,
                      int32_t* valid, double* err_sums) {
    if (!counts || !valid || !err_sums || !thresholds || n_thresholds < 1 || n_thresholds > capf::PCK2D_MAX_THRESHOLDS || joints <= 0 ||
        n < 0 || n_segments <= 0 || (strict != 0 && strict != 1) || (n > 0 && (!pred || !gt || (!segment && n_segments != 1))))
        return CAPF_ERR_INVALID;
    for (int k = 0; k < n_thresholds; ++k)
        if (thresholds[k] != thresholds[k]) return CAPF_ERR_INVALID;                      // a NaN threshold
    if (joints > 32 || (long)n_segments * joints > 0x7fffffffL) return CAPF_ERR_UNSUPPORTED;
    return capf::launch_pck2d_counts(pred, gt, n, joints, norm, weight, thresholds, n_thresholds, strict, segment, n_segments, counts, valid,
                                     err_sums, static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_keypoints_loss(void* stream, int mode, const float* pred, const float* gt, const float* validity, int rows, int dim,
                        float threshold, float* loss, float* dpred) {
    if (!pred || !gt || !validity || !loss || rows <= 0 || dim <= 0 || mode < 0 || mode > 2) return CAPF_ERR_INVALID;
    return capf::launch_keypoints_loss(pred, gt, validity, rows, dim, mode, threshold, loss, dpred,
                                       static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

// ---- the remaining pose losses (pose_losses.hip): every argument is judged here, before anything is launched ----
int capf_keypoints_l2_loss(void* stream, const float* pred, const float* gt, const float* validity, int rows, int dim, float* loss,
                           float* dpred, float grad_scale) {
    if (!pred || !gt || !validity || !loss || rows <= 0 || dim <= 0) return CAPF_ERR_INVALID;
    return capf::launch_keypoints_l2_loss(pred, gt, validity, rows, dim, loss, dpred, grad_scale, static_cast<hipStream_t>(stream)) == hipSuccess
               ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_limb_length_errors(void* stream, const float* pred, const float* gt, int n, int joints, const int32_t* limbs, int n_limbs,
                            float* err, float* dpred, float grad_scale) {
    if (!pred || !gt || !err || !limbs || n <= 0 || joints <= 0 || n_limbs < 1 || n_limbs > capf::LIMB_MAX) return CAPF_ERR_INVALID;
    if (joints > capf::MAX_JOINTS) return CAPF_ERR_UNSUPPORTED;
    capf::LimbTable t = {};
    for (int l = 0; l < n_limbs; ++l) {
        const int32_t a = limbs[2 * l], b = limbs[2 * l + 1];
        if (a < 0 || a >= joints || b < 0 || b >= joints) return CAPF_ERR_INVALID;
        t.a[l] = (unsigned char)a;
        t.b[l] = (unsigned char)b;
    }
    return capf::launch_limb_length_errors(pred, gt, n, joints, t, n_limbs, err, dpred, grad_scale, static_cast<hipStream_t>(stream)) == hipSuccess
               ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_limb_length_sums(void* stream, const float* err, const int32_t* segment, int n, int n_limbs, int n_segments, double* sums,
                          int64_t* counts) {
    if (!err || !sums || !counts || n <= 0 || n_limbs < 1 || n_limbs > capf::LIMB_MAX || n_segments <= 0 || (!segment && n_segments != 1) ||
        (long long)n_segments * n_limbs > 0x7fffffffLL)
        return CAPF_ERR_INVALID;
    return capf::launch_limb_length_sums(err, segment, n, n_limbs, n_segments, sums, reinterpret_cast<long long*>(counts),
                                         static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_uncertainty_loss(void* stream, const float* pred, const float* gt, int rows, int dim, const float* const* sigmas,
                          const int32_t* sigma_widths, int n_sigmas, float* loss, float* dpred, float* const* dsigmas, float grad_scale) {
    if (!pred || !gt || !loss || !sigmas || !sigma_widths || rows <= 0 || dim <= 0 || n_sigmas < 1 || n_sigmas > capf::UNCERTAINTY_MAX_SIGMAS)
        return CAPF_ERR_INVALID;
    capf::UncertaintySigmas sg = {};
    for (int k = 0; k < n_sigmas; ++k) {
        if (!sigmas[k] || (sigma_widths[k] != dim && sigma_widths[k] != 1)) return CAPF_ERR_INVALID;
        sg.sigma[k] = sigmas[k];
        sg.dsigma[k] = dsigmas ? dsigmas[k] : nullptr;
        sg.width[k] = sigma_widths[k];
    }
    return capf::launch_uncertainty_loss(pred, gt, rows, dim, sg, n_sigmas, loss, dpred, grad_scale, static_cast<hipStream_t>(stream)) == hipSuccess
               ? CAPF_OK : CAPF_ERR_HIP;
}

// ---- the 2-D keypoint head (kp_head.hip): every argument is judged here, before anything is launched ----
size_t capf_kp_head_scratch_bytes(int B, int H, int W, int C, int J, int backward) {
    const capf::KpGeom g = capf::kp_geom(B, H, W, C, J);
    if (!g.ok) return 0;
    return (g.fwd_elems + (backward ? g.stat_elems + g.bw_elems : 0)) * sizeof(float);
}

// a map's base address serves its widest load: 16 bytes of fp32, 8 of a 16-bit format
static bool map_aligned(const void* map, int dtype) { return (reinterpret_cast<uintptr_t>(map) & (dtype == CAPF_F32 ? 15 : 7)) == 0; }

// what the head's entries and capf_kp_heatmap_loss judge alike: the shape ...
static int kp_shape_check(int B, int H, int W, int C, int J) { return capf::kp_shape_ok(B, H, W, C, J) ? CAPF_OK : CAPF_ERR_INVALID; }

// ... and, after each entry's own tests, the scratch (`need`: what the entry's own size query answers) and the addresses
static int kp_scratch_check(const void* map, int map_dtype, const void* scratch, size_t scratch_bytes, size_t need) {
    if (need == 0) return CAPF_ERR_UNSUPPORTED;                                             // (more than 2^24 pixels a frame, a grid beyond 2^31)
    if (scratch_bytes < need) return CAPF_ERR_INVALID;
    if (!map_aligned(map, map_dtype) || (reinterpret_cast<uintptr_t>(scratch) & 3)) return CAPF_ERR_INVALID;
    return CAPF_OK;
}

static int kp_head_check(const void* map, int map_dtype, const float* weight, int B, int H, int W, int C, int J, int mode, float beta,
                         const float* decode, const void* scratch, size_t scratch_bytes, int backward) {
    if (!map || !weight || !decode || !scratch) return CAPF_ERR_INVALID;
    if (const int rc = kp_shape_check(B, H, W, C, J)) return rc;
    if (!(beta > 0.f) || !std::isfinite(beta)) return CAPF_ERR_INVALID;
    if ((mode != 0 && mode != 1) || map_dtype < CAPF_F32 || map_dtype > CAPF_F16) return CAPF_ERR_INVALID;
    if (backward && (mode != 1 || map_dtype != CAPF_F32)) return CAPF_ERR_UNSUPPORTED;
    return kp_scratch_check(map, map_dtype, scratch, scratch_bytes, capf_kp_head_scratch_bytes(B, H, W, C, J, backward));
}

// the record of a judged call: what the forward, the pair and the backward have in common, and the outputs of the two forward forms
static capf::KpHeadArgs kp_head_args(const void* map, int map_dtype, const float* weight, const float* bias, int B, int H, int W, int C, int J,
                                     int mode, float beta, const float* decode, const float* to_image, void* scratch, float* kcrop = nullptr,
                                     float* k2d = nullptr, float* score = nullptr, float* heat = nullptr) {
    capf::KpHeadArgs a{};
    a.x = map; a.dtype = map_dtype; a.wt = weight; a.bias = bias; a.to_image = to_image; a.part = static_cast<float*>(scratch);
    a.B = B; a.H = H; a.W = W; a.C = C; a.J = J; a.mode = mode; a.beta = beta;
    std::copy(decode, decode + 4, a.dec);
    a.kcrop = kcrop; a.k2d = to_image ? k2d : nullptr; a.score = score; a.heat = heat;
    return a;
}

int capf_kp_head_forward(void* stream, const void* map_nhwc, int map_dtype, const float* weight, const float* bias, int B, int H, int W, int C,
                         int J, int mode, float beta, const float decode[4], const float* to_image, float* kcrop, float* k2d, float* score,
                         float* heat, void* scratch, size_t scratch_bytes) {
    if (!kcrop) return CAPF_ERR_INVALID;
    if (const int rc = kp_head_check(map_nhwc, map_dtype, weight, B, H, W, C, J, mode, beta, decode, scratch, scratch_bytes, 0)) return rc;
    return capf::launch_kp_head_forward(kp_head_args(map_nhwc, map_dtype, weight, bias, B, H, W, C, J, mode, beta, decode, to_image, scratch, kcrop,
                                                     k2d, score, heat), static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

// the flip-test pair: the map holds 2 * Bsrc frames, everything else is sized by Bsrc
size_t capf_kp_head_pair_scratch_bytes(int Bsrc, int H, int W, int C, int J) {
    if (Bsrc > (1 << 30)) return 0;                                                         // (frame Bsrc + b is an int)
    return capf_kp_head_scratch_bytes(Bsrc, H, W, C, J, 0);
}

int capf_kp_head_forward_pair(void* stream, const void* map_nhwc, int map_dtype, const float* weight, const float* bias, int Bsrc, int H, int W,
                              int C, int J, int mode, float beta, const int32_t* swap, int shift, const float decode[4], const float* to_image,
                              float mirror_width, float* kcrop2, float* k2d2, float* score, float* heat, void* scratch, size_t scratch_bytes) {
    if (!kcrop2 || !swap || (k2d2 && !to_image) || (shift != 0 && shift != 1) || !std::isfinite(mirror_width) || Bsrc > (1 << 30)) return CAPF_ERR_INVALID;
    if (const int rc = kp_head_check(map_nhwc, map_dtype, weight, Bsrc, H, W, C, J, mode, beta, decode, scratch, scratch_bytes, 0)) return rc;
    if (!capf::swap_table_ok(swap, J)) return CAPF_ERR_INVALID;
    capf::KpPairArgs a{};
    static_cast<capf::KpHeadArgs&>(a) = kp_head_args(map_nhwc, map_dtype, weight, bias, Bsrc, H, W, C, J, mode, beta, decode, to_image, scratch,
                                                     kcrop2, k2d2, score, heat);
    std::copy(swap, swap + J, a.swap.j);
    a.shift = shift; a.mirror_w = mirror_width;
    return capf::launch_kp_head_forward_pair(a, static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_kp_head_backward(void* stream, const float* dkcrop, const float* dk2d, const void* map_nhwc, int map_dtype, const float* weight,
                          const float* bias, int B, int H, int W, int C, int J, int mode, float beta, const float decode[4],
                          const float* to_image, float* dweight, float* dbias, float* dmap, int accumulate, void* scratch, size_t scratch_bytes) {
    if (!dweight || !dbias || (!dkcrop && !dk2d) || (dk2d && !to_image) || (accumulate != 0 && accumulate != 1)) return CAPF_ERR_INVALID;
    if (const int rc = kp_head_check(map_nhwc, map_dtype, weight, B, H, W, C, J, mode, beta, decode, scratch, scratch_bytes, 1)) return rc;
    if (reinterpret_cast<uintptr_t>(dmap) & 15) return CAPF_ERR_INVALID;
    capf::KpHeadArgs a = kp_head_args(map_nhwc, map_dtype, weight, bias, B, H, W, C, J, mode, beta, decode, to_image, scratch);
    a.dkcrop = dkcrop; a.dk2d = dk2d; a.dW = dweight; a.dbias = dbias; a.dmap = dmap; a.accumulate = accumulate;
    return capf::launch_kp_head_backward(a, static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

// heatmap supervision of the head: the scratch holds the block sums, (OHKM) g_bj, the frame sums and the dweight / dbias partials
size_t capf_kp_heatmap_loss_scratch_bytes(int B, int H, int W, int C, int J, int reduction) {
    const capf::KpLossGeom lg = capf::kp_loss_geom(B, H, W, C, J);
    if (!lg.ok || (reduction != 0 && reduction != 1)) return 0;
    return (lg.sq_elems + (reduction == 1 ? lg.item_elems : 0) + lg.frame_elems + lg.bw_elems) * sizeof(float);
}

int capf_kp_heatmap_loss(void* stream, const void* map_nhwc, int map_dtype, const float* weight, const float* bias, int B, int H, int W, int C,
                         int J, const float* kcrop_gt, const float* target_weight, const float decode[4], float sigma, int reduction, int topk,
                         float scale, float* loss, float* joint_loss, float* dweight, float* dbias, float* dmap, int accumulate, void* scratch,
                         size_t scratch_bytes) {
    if (!map_nhwc || !weight || !kcrop_gt || !decode || !loss || !scratch) return CAPF_ERR_INVALID;
    if (const int rc = kp_shape_check(B, H, W, C, J)) return rc;
    if (!std::isfinite(decode[0]) || !std::isfinite(decode[2]) || decode[0] == 0.f || decode[2] == 0.f) return CAPF_ERR_INVALID;
    if (!(sigma > 0.f) || !std::isfinite(sigma) || std::ceil(3.f * sigma) > (float)capf::KP_LOSS_MAX_RADIUS) return CAPF_ERR_INVALID;
    if ((reduction != 0 && reduction != 1) || map_dtype < CAPF_F32 || map_dtype > CAPF_F16) return CAPF_ERR_INVALID;
    if (topk < 1 || !std::isfinite(scale) || (accumulate != 0 && accumulate != 1)) return CAPF_ERR_INVALID;
    if (dmap && map_dtype != CAPF_F32) return CAPF_ERR_UNSUPPORTED;
    if (const int rc = kp_scratch_check(map_nhwc, map_dtype, scratch, scratch_bytes, capf_kp_heatmap_loss_scratch_bytes(B, H, W, C, J, reduction))) return rc;
    if (reinterpret_cast<uintptr_t>(dmap) & 15) return CAPF_ERR_INVALID;
    capf::KpLossArgs a{};
    a.x = map_nhwc; a.dtype = map_dtype; a.wt = weight; a.bias = bias; a.gt = kcrop_gt; a.tw = target_weight;
    a.B = B; a.H = H; a.W = W; a.C = C; a.J = J;
    std::copy(decode, decode + 4, a.dec);
    a.sigma = sigma; a.radius = (int)std::ceil(3.f * sigma); a.reduction = reduction; a.topk = topk; a.scale = scale;
    a.loss = loss; a.joint_loss = joint_loss; a.dW = dweight; a.dbias = dbias; a.dmap = dmap; a.accumulate = accumulate;
    a.scratch = static_cast<float*>(scratch);
    return capf::launch_kp_heatmap_loss(a, static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

// ---- CPN's two-peak decode (cpn_decode.hip): every argument is judged here, before anything is launched ----
void capf_cpn_decode_taps(double taps[21]) {
    if (taps) capf::cpn_decode_taps(taps);
}

size_t capf_cpn_decode_lds_bytes(int H, int W) {
    const size_t n = capf::cpn_decode_lds_bytes(H, W);
    return n == (size_t)-1 ? 0 : n;
}

// the record of a call, filled before it is judged (B: the frames decoded, the pair's Bsrc) ...
static capf::CpnDecodeArgs cpn_decode_args(const void* heat, int heat_dtype, int B, int H, int W, int C, int J, const float* decode,
                                           const float* to_image, float* kcrop, float* k2d, float* score, double* blurred) {
    capf::CpnDecodeArgs a{};
    a.heat = heat; a.dtype = heat_dtype; a.B = B; a.H = H; a.W = W; a.C = C; a.J = J;
    if (decode) std::copy(decode, decode + 4, a.dec);
    a.to_image = to_image; a.kcrop = kcrop; a.k2d = k2d; a.score = score; a.blurred = blurred;      // (k2d without to_image: cpn_decode_check refuses it)
    return a;
}

// ... and what the single decode and the pair judge alike.  Not the limit on B * J: the two entries answer it with different codes, each keeps
// its own comparison.
static int cpn_decode_check(const capf::CpnDecodeArgs& a, const float* decode) {
    if (!a.heat || !a.kcrop || !decode || (a.k2d && !a.to_image)) return CAPF_ERR_INVALID;
    if (a.B < 1 || a.H < 1 || a.W < 1 || a.J < 1 || a.J > a.C || a.C > capf::MAX_JOINTS) return CAPF_ERR_INVALID;
    if (a.dtype < CAPF_F32 || a.dtype > CAPF_F16) return CAPF_ERR_INVALID;
    if (!map_aligned(a.heat, a.dtype) || (reinterpret_cast<uintptr_t>(a.kcrop) & 3) || (reinterpret_cast<uintptr_t>(a.blurred) & 7)) return CAPF_ERR_INVALID;
    return capf::cpn_decode_lds_bytes(a.H, a.W) > capf::CPN_LDS_LIMIT ? CAPF_ERR_UNSUPPORTED : CAPF_OK;   // (a workgroup's two planes must fit the 160 KiB of a CU)
}

int capf_cpn_decode(void* stream, const void* heat_nhwc, int heat_dtype, int B, int H, int W, int C, int J, const float decode[4],
                    const float* to_image, float* kcrop, float* k2d, float* score, double* blurred) {
    const capf::CpnDecodeArgs a = cpn_decode_args(heat_nhwc, heat_dtype, B, H, W, C, J, decode, to_image, kcrop, k2d, score, blurred);
    if ((long)B * J >= (1L << 31)) return CAPF_ERR_INVALID;
    if (const int rc = cpn_decode_check(a, decode)) return rc;
    return capf::launch_cpn_decode(a, static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

// the flip-test pair: the map holds 2 * Bsrc frames, everything else is sized by Bsrc
int capf_cpn_decode_pair(void* stream, const void* heat_nhwc, int heat_dtype, int Bsrc, int H, int W, int C, int J, const int32_t* swap,
                         const float decode[4], const float* to_image, float mirror_width, float* kcrop2, float* k2d2, float* score,
                         double* blurred, float* fused) {
    capf::CpnPairArgs a{};
    static_cast<capf::CpnDecodeArgs&>(a) = cpn_decode_args(heat_nhwc, heat_dtype, Bsrc, H, W, C, J, decode, to_image, kcrop2, k2d2, score, blurred);
    if (!swap || !std::isfinite(mirror_width) || (reinterpret_cast<uintptr_t>(fused) & 3)) return CAPF_ERR_INVALID;
    const int rc = cpn_decode_check(a, decode);
    if (rc == CAPF_ERR_INVALID || !capf::swap_table_ok(swap, J)) return CAPF_ERR_INVALID;      // (a bad table outranks a plane too large for LDS)
    if (rc || (long)Bsrc * J >= (1L << 31)) return CAPF_ERR_UNSUPPORTED;       // (rc: cpn_decode_check answers OK, INVALID or UNSUPPORTED, nothing else)
    std::copy(swap, swap + J, a.swap.j);
    a.mirror_w = mirror_width; a.fused = fused;
    return capf::launch_cpn_decode_pair(a, static_cast<hipStream_t>(stream)) == hipSuccess ? CAPF_OK : CAPF_ERR_HIP;
}

int capf_num_ops(const capf_handle* h) { return h ? (int)h->e.ops.size() : CAPF_ERR_INVALID; }

int capf_op_info(const capf_handle* h, int index, int batch, const char** name, const char** kernel, double* flops) {
    if (!h || index < 0 || index >= (int)h->e.ops.size() || batch <= 0) return CAPF_ERR_INVALID;
    const capf::Op& op = h->e.ops[index];
    if (name) *name = op.name.c_str();
    if (flops) *flops = op.flops_per_frame * batch;
    if (kernel) {                                                  // (the ops of a fused launch are named by that launch)
        const capf::Engine::FusedLaunch f = h->e.fused_leader(index, batch);
        *kernel = f.kind == capf::Engine::Fusion::BNECK0 ? capf::bneck0_bf16_kernel_name(h->e.f16())
                  : f.kind == capf::Engine::Fusion::BNECK1 ? capf::bneck1_bf16_kernel_name(h->e.f16())
                  : f.kind == capf::Engine::Fusion::PWCHAIN ? (op.bf16 ? capf::gemm_bf16_pwchain_kernel_name(h->e.f16()) : capf::gemm_f32_pwchain_kernel_name())
                  : h->e.op_route(op, batch).kernel;
    }
    return CAPF_OK;
}

// FLOPs the MFMA pipe is asked to execute for one op at `batch` (Engine::op_route)
int capf_op_executed_flops(const capf_handle* h, int index, int batch, double* flops) {
    if (!h || index < 0 || index >= (int)h->e.ops.size() || batch <= 0 || !flops) return CAPF_ERR_INVALID;
    *flops = h->e.op_route(h->e.ops[index], batch).flops;
    return CAPF_OK;
}

// Algorithmic (compulsory) HBM bytes of one op at `batch`: every operand read once, the result written once.
int capf_op_bytes(const capf_handle* h, int index, int batch, double* bytes) {
    if (!h || index < 0 || index >= (int)h->e.ops.size() || batch <= 0 || !bytes) return CAPF_ERR_INVALID;
    const capf::Engine& e = h->e;
    const capf::Op& op = e.ops[index];
    const double B = batch, act = op.bf16 ? 2.0 : 4.0;
    const double fact = op.feat_bf16 ? 2.0 : 4.0;                             // the lifter samplers: bytes per context-map element
    const capf::Sampler& sm = op.smp;
    const capf::Attn& at = op.attn;
    double b = 0.0;
    switch (op.kind) {
        case capf::OP_GEMM: {
            const capf::Pack& pk = e.packs[op.pack];
            const double M = (double)op.rows_per_frame * B;
            const double in_elems = op.conv ? B * op.H * op.W * op.Cin : M * op.K;
            if (op.bf16 == 2) {          // lifter projection: bf16 operands, fp32 (or, after GELU, bf16) result
                b = in_elems * 2.0 + (double)pk.N * pk.K * 2.0 + (double)pk.N * 4.0 + M * op.N * (op.out_bf16 ? 2.0 : 4.0) +
                    (op.aux >= 0 ? M * op.N * 4.0 : 0.0);
                break;
            }
            b = in_elems * (op.conv && !op.bf16 ? 4.0 : act)                    // fp32 stem reads the fp32 image
                + (double)pk.N * pk.K * (pk.bf16 ? 2.0 : 4.0) + (double)pk.N * 4.0
                + M * op.N * (op.st_f32 ? 4.0 + (op.sh >= 0 ? 2.0 : 0.0) : op.out_bf16 ? 2.0 : act)   // (fp32 stream: fp32 result + bf16 shadow)
                + ((op.aux >= 0 || op.res_param >= 0) ? M * op.N * (op.f32s ? 4.0 : act) : 0.0)
                + ((op.conv && op.up_in >= 0) ? B * op.up_H * op.up_W * op.N * act : 0.0);    // (the low-resolution map added behind the activation)
            break;
        }
        case capf::OP_FUSE: {
            const double out = B * op.H * op.W * op.C;
            b = out * act + (op.sh >= 0 ? out * 2.0 : 0.0);
            for (int i = 0; i < op.n_in; ++i) b += out * act / (double)(1 << (2 * op.shift[i]));
            break;
        }
        case capf::OP_MAXPOOL:
        case capf::OP_RESIZE:
            b = B * op.C * act * ((double)op.H * op.W + (double)op.Ho * op.Wo * (op.aux >= 0 ? 2.0 : 1.0));   // (+ the added map)
            break;
        case capf::OP_CONCAT:
            b = 2.0 * B * op.H * op.W * op.n_in * op.C * act;                   // every source read once, the concatenation written once
            break;
        case capf::OP_LAYERNORM:
            b = (double)op.rows_per_frame * B * op.C * 4.0 * (op.aux >= 0 ? 3.0 : 2.0);
            break;
        case capf::OP_ATTENTION:
            b = (double)at.groups * B * at.tokens * at.heads * at.head_dim * 4.0 * 4.0;       // q, k, v in; o out
            break;
        case capf::OP_SAMPLE_REF:
            b = B * sm.J * op.C * (4.0 * fact + 4.0);                       // 4 corners per joint + the sampled row
            break;
        case capf::OP_DEFORM:
            for (int l = 0; l < sm.L; ++l) b += B * sm.J * sm.NH * op.lvlC[l] * (4.0 * sm.NS * fact + 4.0);
            b += B * sm.J * sm.L * 3.0 * sm.NH * sm.NS * 4.0;
            break;
        case capf::OP_HEAD:
            b = (double)op.rows_per_frame * B * (op.C + 3.0) * 4.0;
            break;
        case capf::OP_RES_CHAIN:                                                 // the token rows in and out, the blocks' weights once
            b = (double)op.rows_per_frame * B * op.C * 4.0 * 2.0 + (double)op.blocks.size() * 8.0 * op.C * op.C * 4.0;
            break;
        case capf::OP_MLP_CHAIN:
            b = (double)op.rows_per_frame * B * op.C * 4.0 * 2.0 + 4.0 * op.C * op.C * 4.0;
            break;
        case capf::OP_PREP_EMBED:
            b = B * sm.J * (op.C + 4.0) * 4.0;
            break;
        case capf::OP_EMBED:
            b = B * sm.J * (sm.L1 * op.C + 4.0) * 4.0;                       // tokens written
            for (int l = 0; l < sm.L; ++l) b += B * sm.J * op.lvlC[l] * 4.0 * fact + (double)op.C * op.lvlC[l] * 4.0;
            break;
        case capf::OP_CTX_ATTN:
            for (int l = 0; l < sm.L; ++l)
                b += B * sm.J * sm.NH * sm.NS * op.lvlC[l] * 4.0 * fact + (double)(op.C / sm.NH) * op.lvlC[l] * 4.0;
            b += B * sm.J * (sm.L + 1 + sm.L) * op.C * 4.0;                 // tokens read, tokens 1..L written
            break;
        default: break;
    }
    *bytes = b;
    return CAPF_OK;
}

int capf_op_schedule(const capf_handle* h, int index, int32_t* region, int32_t* level, int32_t* lane, int32_t* reads,
                     int32_t* writes) {
    if (!h || index < 0 || index >= (int)h->e.ops.size()) return CAPF_ERR_INVALID;
    const capf::Engine& e = h->e;
    const capf::Op& op = e.ops[index];
    const bool control = op.kind == capf::OP_FORK || op.kind == capf::OP_JOIN;
    if (region) *region = control ? -1 : op.region;
    if (lane) *lane = op.lane;
    if (level) *level = control ? -1 : op.level;
    // The ABI's layout is Op::reads() / writes() without their last slot, which has no column of its own here: the map a conv adds behind
    // its activation is reported as its second input (a conv has one), the bf16 shadow in the first outs[] column (a conv / fuse sum writes
    // no outs[])
    if (reads) {
        const auto r = op.reads();
        std::copy(r.begin(), r.begin() + 5, reads);
        if (r[5] >= 0) reads[1] = r[5];
    }
    if (writes) {
        const auto w = op.writes();
        std::copy(w.begin(), w.begin() + 6, writes);
        if (w[6] >= 0) writes[2] = w[6];
    }
    return CAPF_OK;
}

int capf_op_stream_class(const capf_handle* h, int index, int batch) {
    if (!h || index < 0 || index >= (int)h->e.ops.size() || batch <= 0) return CAPF_ERR_INVALID;
    const capf::Engine& e = h->e;
    const capf::Op& op = e.ops[index];
    if (op.region < 0 || op.kind == capf::OP_FORK || op.kind == capf::OP_JOIN || e.lanes == 0) return 0;
    if (e.lanes == 1) return op.lane > 0 ? 1 : 0;
    const bool two = e.two_chains(e.ops[e.regions[op.region].first], batch);
    return two && (op.lane == 1 || op.lane == 2) ? 1 : 0;
}

int capf_forward_prefix(capf_handle* h, void* stream, const float* images_nhwc, const float* k2d, float* kcrop_inout, int batch,
                        float* out, int n_ops) {
    if (!h || !images_nhwc) return CAPF_ERR_INVALID;
    Engine& e = h->e;
    if (n_ops < 0 || n_ops > (int)e.ops.size()) return CAPF_ERR_INVALID;
    if (n_ops > e.n_backbone_ops && (!k2d || !kcrop_inout || !out)) return CAPF_ERR_INVALID;
    return begin_and_run(e, stream, {"capf_forward_prefix", images_nhwc, k2d, kcrop_inout, out, batch, 0, n_ops});
}

int capf_op_describe(const capf_handle* h, int index, capf_op_desc* d) {
    if (!h || !d || index < 0 || index >= (int)h->e.ops.size()) return CAPF_ERR_INVALID;
    const Engine& e = h->e;
    const capf::Op& op = e.ops[index];
    memset(d, 0, sizeof(*d));
    d->kind = op.kind == capf::OP_GEMM ? 0 : op.kind == capf::OP_FUSE ? 1 : op.kind == capf::OP_MAXPOOL ? 2
              : op.kind == capf::OP_RESIZE ? 3 : op.kind == capf::OP_LAYERNORM ? 4 : op.kind == capf::OP_ATTENTION ? 5 : -1;
    if (op.debug_only) d->kind = -1;
    d->backbone = index < e.n_backbone_ops;
    d->p_weight = d->p_bn_weight = d->p_bias = d->p_ln_weight = d->p_ln_bias = -1;
    d->rows_per_frame = (int)op.rows_per_frame;
    d->eps = op.eps;
    {
        const capf::RowMap* m[3] = {&op.amap, &op.omap, &op.rmap};
        for (int k = 0; k < 3; ++k) { d->maps[k][0] = m[k]->G; d->maps[k][1] = m[k]->S1; d->maps[k][2] = m[k]->S2; d->maps[k][3] = m[k]->off; }
    }
    const int dt16 = e.dt16();                                 // what a 16-bit tensor of this handle holds: 2 bf16, 3 fp16
    const int act_dt = e.b16() ? dt16 : 0;
    d->in_dtype = d->out_dtype = (d->backbone ? act_dt : 0);
    d->H = op.H; d->W = op.W; d->Ho = op.Ho; d->Wo = op.Wo;
    if (op.kind == capf::OP_GEMM) {
        const capf::Pack& pk = e.packs[op.pack];
        d->conv = op.conv; d->Cin = op.conv ? op.Cin : op.K; d->Cout = op.N;
        d->ks = op.ks; d->stride = op.stride; d->pad = op.pad; d->act = op.act;
        d->has_residual = op.aux >= 0 || op.res_param >= 0;
        if (op.conv && op.up_in >= 0) { d->up_H = op.up_H; d->up_W = op.up_W; }
        d->mfma_bf16 = (op.bf16 || op.out_bf16) ? 1 : 0;
        if (op.conv) {
            d->in_dtype = op.in[0] == -2 ? 0 : (op.bf16 ? dt16 : 0);
            d->out_dtype = op.st_f32 ? 0 : (op.bf16 || op.out_bf16) ? dt16 : 0;
            d->p_weight = pk.w[0]; d->p_bn_weight = pk.bn.g;
        } else {
            d->in_dtype = op.bf16 == 2 ? dt16 : 0;
            d->out_dtype = op.out_bf16 ? dt16 : 0;
            d->p_weight = pk.n_lin == 1 ? pk.w[0] : -1;
            d->p_bias = pk.n_lin == 1 ? pk.b[0] : -1;
            d->p_ln_weight = op.ln.w; d->p_ln_bias = op.ln.b;
        }
    } else if (op.kind == capf::OP_LAYERNORM) {
        d->Cin = d->Cout = op.C;
        d->in_dtype = 0; d->out_dtype = op.out_bf16 ? dt16 : 0;
        d->has_residual = op.aux >= 0;
        d->p_ln_weight = op.ln.w; d->p_ln_bias = op.ln.b;
        d->maps[1][0] = 1; d->maps[1][1] = op.C; d->maps[1][2] = 0; d->maps[1][3] = 0;        // normalised rows are written densely
    } else if (op.kind == capf::OP_ATTENTION) {
        const capf::Attn& at = op.attn;
        d->attn[0] = at.groups; d->attn[1] = at.tokens; d->attn[2] = at.heads; d->attn[3] = at.head_dim;
        d->rows_per_frame = at.groups * at.tokens;
        d->Cin = 3 * at.heads * at.head_dim; d->Cout = at.heads * at.head_dim;
        d->in_dtype = 0; d->out_dtype = op.out_bf16 ? dt16 : 0;
        d->maps[0][0] = 1; d->maps[0][1] = d->Cin; d->maps[1][0] = 1; d->maps[1][1] = d->Cout;
    } else {
        d->Cin = d->Cout = op.C;
        d->n_in = op.n_in; d->relu = op.relu;
        d->has_residual = op.kind == capf::OP_RESIZE && op.aux >= 0;      // out = resize(in) + aux
        for (int i = 0; i < 4; ++i) d->shift[i] = op.shift[i];
        if (op.kind == capf::OP_FUSE) { d->Ho = op.H; d->Wo = op.W; }
        if (op.kind == capf::OP_FUSE && d->backbone) d->in_dtype = d->out_dtype = op.bf16 ? dt16 : 0;
    }
    d->checkpoint = (op.bneck_c3 >= 0 ? op.bneck_c3 : op.region >= 0 ? e.regions[op.region].second : index) + 1;
    return CAPF_OK;
}

int capf_op_describe_sized(const capf_handle* h, int index, void* desc, size_t desc_bytes) {
    if (!desc || desc_bytes == 0) return CAPF_ERR_INVALID;
    capf_op_desc full;
    const int rc = capf_op_describe(h, index, &full);
    if (rc != CAPF_OK) return rc;
    memset(desc, 0, desc_bytes);
    memcpy(desc, &full, desc_bytes < sizeof(full) ? desc_bytes : sizeof(full));
    return CAPF_OK;
}

int capf_op_tensor(const capf_handle* h, int index, int slot, const void** dev_ptr) {
    if (!h || !dev_ptr || index < 0 || index >= (int)h->e.ops.size() || slot < 0 || slot > 6) return CAPF_ERR_INVALID;
    const Engine& e = h->e;
    const capf::Op& op = e.ops[index];
    // slots 0..4: capf_op_schedule's reads (the map a conv adds behind its activation in slot 1), 5: the output, 6: its bf16 shadow
    const auto r = op.reads();
    const int buf = slot == 1 && r[5] >= 0 ? r[5] : slot < 5 ? r[slot] : slot == 5 ? op.out : op.sh;
    if (buf == -2) { *dev_ptr = e.ses.images(); return CAPF_OK; }
    if (buf < 0 || !e.ws || e.ses.last_batch <= 0) return CAPF_ERR_INVALID;
    *dev_ptr = e.bptr(buf, e.ses.last_batch);
    return CAPF_OK;
}

int capf_op_h2_planes(const capf_handle* h, int index, int batch, const void** exps, int32_t* tile_pixels) {
    if (!h || index < 0 || index >= (int)h->e.ops.size() || batch <= 0) return CAPF_ERR_INVALID;
    const Engine& e = h->e;
    const capf::Op& op = e.ops[index];
    if (!op.h2_role || !e.ws) return 0;
    const capf::GemmArgs a = e.gemm_args(op, batch);
    if (!a.h2_ein && !a.h2_eout) return 0;
    if (exps) *exps = a.h2_ein ? static_cast<const void*>(a.h2_ein) : static_cast<const void*>(a.h2_eout);
    int tp = 0;
    capf::f32h2_tiles_m(batch, op.H, op.W, &tp);
    if (tile_pixels) *tile_pixels = tp;
    return op.h2_role;
}

int capf_forward_profile(capf_handle* h, void* stream, const float* images_nhwc, const float* k2d, float* kcrop_inout,
                         int batch, float* out, float* op_ms, int n_ops) {
    if (!h || !images_nhwc || !k2d || !kcrop_inout || !out || !op_ms) return CAPF_ERR_INVALID;
    Engine& e = h->e;
    const int n = (int)e.ops.size();
    if (n_ops < n) return CAPF_ERR_INVALID;
    int rc = e.begin({"capf_forward_profile", images_nhwc, k2d, kcrop_inout, out, batch, 0, n});
    if (rc) return rc;
    std::vector<hipEvent_t> ev(n + 1, nullptr);
    for (auto& x : ev)
        if (rc == CAPF_OK && hipEventCreate(&x) != hipSuccess) rc = CAPF_ERR_HIP;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (rc == CAPF_OK) rc = e.run(s, batch, 0, n, ev.data());
    if (rc == CAPF_OK && hipStreamSynchronize(s) != hipSuccess) rc = CAPF_ERR_HIP;
    for (int i = 0; i < n && rc == CAPF_OK; ++i)
        if (hipEventElapsedTime(&op_ms[i], ev[i], ev[i + 1]) != hipSuccess) rc = CAPF_ERR_HIP;
    for (auto& x : ev)                                     // (on every path: the events made before one could not be)
        if (x) (void)hipEventDestroy(x);
    return rc;
}

int capf_forward_profile_launches(capf_handle* h, void* stream, const float* images_nhwc, const float* k2d,
                                  float* kcrop_inout, int batch, float* out, float* op_ms, int32_t* op_leader, int n_ops) {
    if (!h || !images_nhwc || !k2d || !kcrop_inout || !out || !op_ms || !op_leader) return CAPF_ERR_INVALID;
    Engine& e = h->e;
    const int n = (int)e.ops.size();
    if (n_ops < n) return CAPF_ERR_INVALID;
    int rc = e.begin({"capf_forward_profile_launches", images_nhwc, k2d, kcrop_inout, out, batch, 0, n});
    if (rc) return rc;
    capf::LaunchLog log;
    log.op_leader.assign(n, -1);
    log.op_variant.assign(n, -1);
    hipStream_t s = static_cast<hipStream_t>(stream);
    rc = e.run(s, batch, 0, n, nullptr, &log);
    e.ses.last_variants = log.op_variant;
    if (rc == CAPF_OK && hipStreamSynchronize(s) != hipSuccess) rc = CAPF_ERR_HIP;
    for (int i = 0; i < n; ++i) { op_ms[i] = 0.f; op_leader[i] = log.op_leader[i]; }
    for (size_t k = 0; k < log.leader.size() && rc == CAPF_OK; ++k)
        if (hipEventElapsedTime(&op_ms[log.leader[k]], log.ev[k], log.ev[k + 1]) != hipSuccess) rc = CAPF_ERR_HIP;
    return rc;
}

int capf_forward_profile_variants(const capf_handle* h, int32_t* op_variant, int n_ops) {
    if (!h || !op_variant || n_ops < (int)h->e.ses.last_variants.size()) return CAPF_ERR_INVALID;
    for (size_t i = 0; i < h->e.ses.last_variants.size(); ++i) op_variant[i] = h->e.ses.last_variants[i];
    return CAPF_OK;
}

int capf_forward_stats(const capf_handle* h, int batch, int64_t* launches, double* flops) {
    if (!h) return CAPF_ERR_INVALID;
    int64_t n = 0;
    double f = 0.0;
    for (const capf::Op& op : h->e.ops) {
        if (op.debug_only) continue;
        if (op.kind == capf::OP_FORK || op.kind == capf::OP_JOIN) continue;
        ++n;
        f += op.flops_per_frame * batch;
    }
    if (launches) *launches = n;
    if (flops) *flops = f;
    return CAPF_OK;
}

}  // extern "C"
