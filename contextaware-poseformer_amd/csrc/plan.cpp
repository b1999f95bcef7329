// Static layer plan + parameter schema of the hot path.
//
// Restates, as a flat list of kernel launches over NHWC buffers, the module graphs of
//   PoseHighResolutionNet   ContextPose/mvn/models/pose_hrnet.py:312-501
//   CPN50                   ContextPose/mvn/models/networks/{network,resnet,globalNet,refineNet}.py
//   PoseTransformer         ContextPose/mvn/models/pose_dformer.py:144-241
// and registers every state_dict entry under the reference's name, so that
// released checkpoints load strict=True into the host module built from this schema.
#include <limits.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <tuple>

#include "engine.h"

namespace capf {

static const int EXT_IMAGES = -2;

static size_t round64(size_t n) { return (n + 63) / 64 * 64; }
static int round32(int n) { return (n + 31) / 32 * 32; }
static int round64(int n) { return (n + 63) / 64 * 64; }

int Engine::add_param(const std::string& name, int kind, std::initializer_list<int64_t> shape) {
    auto it = param_index.find(name);
    if (it != param_index.end()) return it->second;
    Param p;
    p.name = name;
    p.kind = kind;
    p.ndim = (int)shape.size();
    int i = 0;
    for (int64_t s : shape) p.shape[i++] = s;
    params.push_back(p);
    param_index[name] = (int)params.size() - 1;
    return (int)params.size() - 1;
}

int Engine::new_buffer(size_t elems, const std::string& tag) {
    Buffer b;
    b.elems = round64(elems);
    b.def_op = (int)ops.size();
    b.last_op = (int)ops.size();
    b.tag = tag;
    bufs.push_back(b);
    return (int)bufs.size() - 1;
}

void Engine::use(int buf) {
    if (buf >= 0) bufs[buf].last_op = std::max(bufs[buf].last_op, (int)ops.size());
}

void Engine::push(Op op) {
    op.lane = cur_lane;
    op.region = cur_region;
    ops.push_back(op);
}

void Engine::fork(int n) {
    Op op;
    op.kind = OP_FORK;
    op.name = "fork";
    op.fork = Fork{n, n_events};          // (event ids of this region: 1 for the fork + (n-1) for the join)
    n_events += n;
    cur_region = n_regions++;
    cur_lane = 0;
    regions.push_back({(int)ops.size(), -1});
    push(op);
}

void Engine::join() {
    Op op;
    op.kind = OP_JOIN;
    op.name = "join";
    op.fork = ops[regions[cur_region].first].fork;
    cur_lane = 0;
    regions[cur_region].second = (int)ops.size();
    push(op);
    cur_region = -1;
}

static void keep(Engine& e, int buf) { e.bufs[buf].last_op = INT_MAX; }

static void name_tensor(Engine& e, const std::string& name, int buf, std::initializer_list<int64_t> shape,
                        int is_int = 0) {
    NamedTensor t{};
    t.buf = buf;
    t.ndim = (int)shape.size();
    int i = 0;
    for (int64_t s : shape) t.shape[i++] = s;
    t.is_int = is_int;
    e.named[name] = t;
    keep(e, buf);
}

static BnRef reg_bn(Engine& e, const std::string& bn, int C) {      // nn.BatchNorm2d's state_dict entries, in its order
    BnRef r;
    r.g = e.add_param(bn + ".weight", CAPF_P_BN_W, {C});
    r.b = e.add_param(bn + ".bias", CAPF_P_BN_B, {C});
    r.m = e.add_param(bn + ".running_mean", CAPF_P_BN_MEAN, {C});
    r.v = e.add_param(bn + ".running_var", CAPF_P_BN_VAR, {C});
    e.add_param(bn + ".num_batches_tracked", CAPF_P_BN_NBT, {});
    return r;
}

// conv (bias=False) + eval BatchNorm (+ residual) (+ ReLU) as ONE implicit-GEMM launch.
// pad_rows_to > Cout: the parameter and its BatchNorm keep their Cout rows, the pack, the op and the output map have pad_rows_to (rows and
// channels Cout .. pad_rows_to - 1: zero weights, zero bias -- exact zeros behind ACT_NONE), so that a width no kernel takes rides one that all do
Tensor Engine::conv_bn(const std::string& conv, const std::string& bn, const Tensor& x, int Cout, int ks,
                       int stride, int act, const Tensor* residual, int pad_rows_to) {
    const int pad = ks / 2;
    Tensor y;
    y.H = (x.H + 2 * pad - ks) / stride + 1;
    y.W = (x.W + 2 * pad - ks) / stride + 1;

    Pack pk;
    pk.kind = CONV_BN;
    pk.w[0] = add_param(conv + ".weight", CAPF_P_CONV_W, {Cout, x.C, ks, ks});
    pk.bn = reg_bn(*this, bn, Cout);
    const bool padded = pad_rows_to > Cout;
    if (padded) { pk.n_src = Cout; Cout = pad_rows_to; }
    y.C = Cout;
    pk.N = Cout;
    pk.Cin = x.C;
    pk.ks = ks;
    pk.K = ks * ks * x.C;
    const bool use_bf16 = b16() && x.C % 8 == 0;       // the Cin = 3 stem stays on the fp32 kernel
    pk.bf16 = use_bf16;
    pk.Kpad = use_bf16 ? round64(pk.K) : round32(pk.K);
    // The 3x3 stride-1 fp32 convs that may leave the direct kernel (Op::fast3x3; Engine::gemm_family routes them per batch): to the plan's
    // split-fp32 tile, or to Winograd along W (igemm_wino.hip: 1.5x fewer MFMAs with F(2,3)).  ONE eligibility rule for both routes, the
    // Winograd kernels': Cin % 32 == 0, Cout % 32 == 0, even W -- the tile is offered to no other conv (HRNet-48's 48-channel branch stays on
    // the direct kernel), and CAPF_PLAN_NO_WINOGRAD takes the tile away with the Winograd kernels
    const bool fast3x3 = plan.use_wino && !use_bf16 && ks == 3 && stride == 1 && x.C % 32 == 0 && x.W % 2 == 0 && Cout % 32 == 0 && !padded;
    pk.fast3x3 = fast3x3;
    // F(4,3) (half the MFMAs of the direct conv) where the row length allows four-pixel tiles, F(2,3) (two thirds) otherwise.
    // HRNet only: F(4,3) pays inside the grouped multi-branch launches (+3.2 % end to end), not for CPN's lone convs (-0.8 %).
    if (fast3x3) { pk.direct_Kpad = pk.Kpad; pk.Kpad = ((x.W % 4 == 0 && plan.wino_f43 && (cfg.backbone == CAPF_HRNET || plan.wino_f43_cpn) && x.H * x.W >= plan.wino_f43_min_hw && x.H * x.W <= plan.wino_f43_max_hw) ? 18 : 12) * x.C; }
    // bf16: the 3x3 stride-1 convs also keep their weights in the row-halo layout (igemm_bf16.hip: one staged activation tile
    // for the three kw taps); launches of >= 2048 tiles run that kernel, smaller ones the ring kernel on the standard layout
    if (use_bf16 && plan.use_rh && ks == 3 && stride == 1 && bf16_rh_width(x.C) && Cout % 4 == 0 && !padded) { pk.rh = true; pk.rh_Kpad = 9 * x.C; }
    // ... and in the layout of the 2-D halo tile (igemm_bf16_ws.hip), which runs them from 1 GFLOP per conv and batch 24 up (build() finds
    // the batches: tile_takes)
    if (use_bf16 && plan.use_ws && ks == 3 && stride == 1 && x.C % 16 == 0 && Cout % 8 == 0 && !padded) pk.ws = true;
    // fp32: the fast3x3 convs also keep their weights as the pieces the plan's split-fp32 tile takes (igemm_f32h2_ws.hip / igemm_f32x3_ws.hip),
    // which runs them from 370 MFLOP per conv and batch 5 up (build() finds the batches: tile_takes)
    if (fast3x3 && plan.use_x3 && x.W <= 256) pk.x3 = true;
    // fp32: every conv with 16-byte-aligned channel counts also keeps its weights as two block-scaled fp16 pieces in the direct layout's
    // geometry (igemm_f32h2.hip): what runs on the plain fp32 MFMA kernel at batch < 5 runs there from batch 5 (1x1 / stride-2 fuse and
    // transition convs, lone convs; the HBM-bound pointwise kernels of layer1 keep theirs)
    if (!use_bf16 && plan.use_h2g && x.C % 4 == 0 && Cout % 4 == 0 && !padded) { pk.h2g = true; pk.h2g_Kpad = fast3x3 ? pk.direct_Kpad : pk.Kpad; }
    packs.push_back(pk);

    Op op;
    op.kind = OP_GEMM;
    op.name = conv;
    op.conv = 1;
    op.pack = (int)packs.size() - 1;
    op.in[0] = x.buf;
    op.Cin = x.C; op.H = x.H; op.W = x.W; op.Ho = y.H; op.Wo = y.W;
    op.ks = ks; op.stride = stride; op.pad = pad;
    op.rows_per_frame = (long)y.H * y.W;
    op.N = Cout; op.K = pk.K; op.act = act;
    op.omap = row_ld(Cout);
    op.rmap = row_ld(Cout);
    op.flops_per_frame = 2.0 * y.H * y.W * (double)Cout * pk.K;
    use(x.buf);
    if (residual) {
        op.aux = residual->buf;
        use(residual->buf);
    }
    op.bf16 = use_bf16 ? 1 : 0;
    op.fast3x3 = fast3x3 ? 1 : 0;
    op.out_bf16 = (b16() && !use_bf16) ? 1 : 0;
    y.buf = new_buffer(act_elems((size_t)y.H * y.W * Cout), conv);
    op.out = y.buf;
    push(op);
    return y;
}

static Tensor fuse_sum(Engine& e, const std::string& name, const Tensor* terms, const int* shifts, int n,
                       const Tensor& like, int relu) {
    Op op;
    op.kind = OP_FUSE;
    op.name = name;
    op.n_in = n;
    for (int i = 0; i < n; ++i) {
        op.in[i] = terms[i].buf;
        op.shift[i] = shifts[i];
        e.use(terms[i].buf);
    }
    op.H = like.H; op.W = like.W; op.C = like.C; op.relu = relu;
    op.bf16 = e.b16() ? 1 : 0;
    Tensor y = like;
    y.buf = e.new_buffer(e.act_elems((size_t)like.H * like.W * like.C), name);
    op.out = y.buf;
    e.push(op);
    return y;
}

// ---------------------------------------------------------------------------------------------------
// HRNet (pose_hrnet.py)
// ---------------------------------------------------------------------------------------------------
static Tensor hr_basic_block(Engine& e, const std::string& p, const Tensor& x) {   // :66-95
    Tensor y = e.conv_bn(p + ".conv1", p + ".bn1", x, x.C, 3, 1, ACT_RELU, nullptr);
    const int i1 = (int)e.ops.size() - 1;
    Tensor out = e.conv_bn(p + ".conv2", p + ".bn2", y, x.C, 3, 1, ACT_RELU, &x);
    const int i2 = (int)e.ops.size() - 1;
    // conv1's output has ONE reader, conv2, and both convs have the same tiles: where both run the two-fp16-piece tile (a matter of the
    // batch, decided per launch in gemm_args) it travels as split fp16 planes + one scale exponent per (tile, 16-channel chunk) --
    // igemm_f32h2_ws_tile.h PLANES: the consumer's K loop loses its maximum / split / scale-exchange phase.  Same bytes, same buffer.
    if (e.plan.use_h2_planes && e.plan.x3_h2 && !e.b16() && x.C % 16 == 0 && e.packs[e.ops[i1].pack].x3 && e.packs[e.ops[i2].pack].x3) {
        const int tiles_pf = f32h2_tiles_m(1, x.H, x.W);
        if (tiles_pf > 0) {
            const int b = e.new_buffer((size_t)tiles_pf * (x.C / 16) + 16, p + ".conv1.exps");
            e.bufs[b].def_op = i1;
            e.bufs[b].last_op = i2;
            e.ops[i1].h2_exps = b; e.ops[i1].h2_role = 1; e.ops[i1].h2_peer = i2;
            e.ops[i2].h2_exps = b; e.ops[i2].h2_role = 2; e.ops[i2].h2_peer = i1;
        }
    }
    return out;
}

// A first bottleneck whose five ops may run as ONE kernel (bneck_bf16.hip; Engine::fused_at decides per batch): that kernel reads x while it
// writes y and -- in the variant the layer-wise tests run -- conv1's, conv2's and the shortcut's outputs too, so all five tensors stay alive
// (no two of them share workspace) from conv1 to conv3; the ops remember conv3 (capf_op_describe: their checkpoint is the whole block).
// `fork` = index of the region's fork op: fork, conv1, conv2, downsample, join, conv3.
static void bneck0_mark(Engine& e, int fork) {
    if (!e.plan.use_bneck || !e.b16() || fork + 5 >= (int)e.ops.size()) return;
    const int c1 = fork + 1, c2 = fork + 2, ds = fork + 3, c3 = fork + 5;
    const Op &o1 = e.ops[c1], &o3 = e.ops[c3];
    if (e.ops[fork].kind != OP_FORK || e.ops[fork + 4].kind != OP_JOIN || o1.Cin != 64 || o1.N != 64 || o3.N != 256 || e.ops[c2].stride != 1 || e.ops[c2].ks != 3) return;
    for (int b : {o1.in[0], o1.out, e.ops[c2].out, e.ops[ds].out, o3.out}) {
        if (b < 0) continue;
        e.bufs[b].def_op = std::min(e.bufs[b].def_op, c1);
        e.bufs[b].last_op = std::max(e.bufs[b].last_op, c3);
    }
    for (int k : {c1, c2, ds}) e.ops[k].bneck_c3 = c3;
}

// ... and an identity bottleneck (conv1 at `c1`, conv2, conv3 + x): x, conv1's and conv2's outputs and y alive from conv1 to conv3
static void bneck1_mark(Engine& e, int c1) {
    if (!e.plan.use_bneck || !e.b16() || c1 + 2 >= (int)e.ops.size()) return;
    const Op &o1 = e.ops[c1], &o2 = e.ops[c1 + 1], &o3 = e.ops[c1 + 2];
    if (o1.kind != OP_GEMM || o2.kind != OP_GEMM || o3.kind != OP_GEMM || o1.Cin != 256 || o1.N != 64 || o2.ks != 3 || o2.stride != 1 || o3.N != 256 || o3.aux != o1.in[0]) return;
    for (int b : {o1.in[0], o1.out, o2.out, o3.out}) {
        if (b < 0) continue;
        e.bufs[b].def_op = std::min(e.bufs[b].def_op, c1);
        e.bufs[b].last_op = std::max(e.bufs[b].last_op, c1 + 2);
    }
    e.ops[c1].bneck_c3 = c1 + 2;
    e.ops[c1 + 1].bneck_c3 = c1 + 2;
}

static Tensor hr_bottleneck(Engine& e, const std::string& p, const Tensor& x, int planes, bool down) {  // :98-136
    const int fork_at = (int)e.ops.size();
    if (down) e.fork(2);             // the projection shortcut only reads x: independent of conv1 / conv2
    Tensor y = e.conv_bn(p + ".conv1", p + ".bn1", x, planes, 1, 1, ACT_RELU, nullptr);
    y = e.conv_bn(p + ".conv2", p + ".bn2", y, planes, 3, 1, ACT_RELU, nullptr);
    Tensor r = x;
    if (down) {
        e.set_lane(1);
        r = e.conv_bn(p + ".downsample.0", p + ".downsample.1", x, planes * 4, 1, 1, ACT_NONE, nullptr);
        e.join();
    }
    Tensor out = e.conv_bn(p + ".conv3", p + ".bn3", y, planes * 4, 1, 1, ACT_RELU, &r);
    if (down) bneck0_mark(e, fork_at);
    else bneck1_mark(e, fork_at);
    return out;
}

// HighResolutionModule (:139-303).  xs: in/out; branch_out (optional) receives the branch outputs.
static void hr_module(Engine& e, const std::string& p, std::vector<Tensor>& xs, int n_out, int blocks,
                      std::vector<Tensor>* branch_out) {
    const int nb = (int)xs.size();
    std::vector<Tensor> br(nb);
    e.fork(nb);                      // the branches are independent until the fuse: one stream lane each
    for (int i = 0; i < nb; ++i) {
        e.set_lane(i);
        Tensor y = xs[i];
        for (int k = 0; k < blocks; ++k)
            y = hr_basic_block(e, p + ".branches." + std::to_string(i) + "." + std::to_string(k), y);
        br[i] = y;
    }
    e.join();
    if (branch_out) *branch_out = br;
    std::vector<Tensor> outs(n_out);
    e.fork(n_out);                   // each fused output only reads the branch outputs: independent lanes again
    for (int i = 0; i < n_out; ++i) {
        e.set_lane(i);
        Tensor terms[4];
        int shifts[4] = {0, 0, 0, 0};
        for (int j = 0; j < nb; ++j) {
            const std::string fp = p + ".fuse_layers." + std::to_string(i) + "." + std::to_string(j);
            if (j == i) {
                terms[j] = br[j];
            } else if (j > i) {   // 1x1 conv + BN at low resolution; nearest x2^(j-i) applied by the fuse kernel
                terms[j] = e.conv_bn(fp + ".0", fp + ".1", br[j], br[i].C, 1, 1, ACT_NONE, nullptr);
                shifts[j] = j - i;
            } else {              // (i-j) stride-2 3x3 convs, ReLU on all but the last
                Tensor t = br[j];
                for (int k = 0; k < i - j; ++k) {
                    const bool last = (k == i - j - 1);
                    const std::string cp = fp + "." + std::to_string(k);
                    t = e.conv_bn(cp + ".0", cp + ".1", t, last ? br[i].C : br[j].C, 3, 2,
                                  last ? ACT_NONE : ACT_RELU, nullptr);
                }
                terms[j] = t;
            }
        }
        outs[i] = fuse_sum(e, p + ".fuse" + std::to_string(i), terms, shifts, nb, br[i], 1);
    }
    e.join();
    xs = outs;
}

void Engine::build_hrnet(Tensor img, Tensor feats[4]) {
    const std::string B = "backbone";
    Tensor x = conv_bn(B + ".conv1", B + ".bn1", img, 64, 3, 2, ACT_RELU, nullptr);     // :465-467
    x = conv_bn(B + ".conv2", B + ".bn2", x, 64, 3, 2, ACT_RELU, nullptr);              // :468-470
    for (int k = 0; k < 4; ++k) x = hr_bottleneck(*this, B + ".layer1." + std::to_string(k), x, 64, k == 0);

    std::vector<Tensor> ys = {x};
    std::vector<int> pre_ch = {256};
    for (int stage = 2; stage <= 4; ++stage) {
        const int nb = stage;
        // transition (:377-411)
        std::vector<Tensor> xs(nb);
        const std::string tp = B + ".transition" + std::to_string(stage - 1) + ".";
        const int npre = (int)pre_ch.size();
        fork(nb);                    // every transition path reads the previous stage's outputs only
        for (int i = 0; i < nb; ++i) {
            set_lane(std::min(i, 3));
            const int ch = cfg.hr_channels[i];
            if (i < npre) {
                if (ch != pre_ch[i])
                    xs[i] = conv_bn(tp + std::to_string(i) + ".0", tp + std::to_string(i) + ".1", ys[i], ch, 3, 1,
                                    ACT_RELU, nullptr);
                else
                    xs[i] = ys[i];
            } else {
                Tensor t = ys[npre - 1];
                for (int j = 0; j < i + 1 - npre; ++j) {
                    const int oc = (j == i - npre) ? ch : pre_ch[npre - 1];
                    const std::string cp = tp + std::to_string(i) + "." + std::to_string(j);
                    t = conv_bn(cp + ".0", cp + ".1", t, oc, 3, 2, ACT_RELU, nullptr);
                }
                xs[i] = t;
            }
        }
        join();
        const int nmod = cfg.hr_modules[stage - 2];
        for (int m = 0; m < nmod; ++m) {
            const bool last = (stage == 4 && m == nmod - 1);          // multi_scale_output=False (:359-360)
            std::vector<Tensor> br;
            hr_module(*this, B + ".stage" + std::to_string(stage) + "." + std::to_string(m), xs, last ? 1 : nb,
                      cfg.hr_blocks, (stage == 4 && m == 0) ? &br : nullptr);
            if (stage == 4 && m == 0) {
                // forward() returns x_list[1..3], which stage4[0] overwrote in place with its BRANCH
                // outputs (:289-290, :501).
                for (int i = 1; i < 4; ++i) feats[i] = br[i];
            }
        }
        ys = xs;
        pre_ch.assign(cfg.hr_channels, cfg.hr_channels + nb);
    }
    feats[0] = ys[0];
}

// ---------------------------------------------------------------------------------------------------
// CPN-50 (networks/)
// ---------------------------------------------------------------------------------------------------
static Tensor pool_or_resize(Engine& e, OpKind kind, const std::string& name, const Tensor& x, int Ho, int Wo,
                             const Tensor* add = nullptr) {
    Op op;
    op.kind = kind;
    op.name = name;
    op.in[0] = x.buf;
    e.use(x.buf);
    if (add) { op.aux = add->buf; e.use(add->buf); }           // resize only: out = resize(x) + add
    op.H = x.H; op.W = x.W; op.C = x.C; op.Ho = Ho; op.Wo = Wo;
    op.bf16 = e.b16() ? 1 : 0;
    Tensor y{-1, Ho, Wo, x.C};
    y.buf = e.new_buffer(e.act_elems((size_t)Ho * Wo * x.C), name);
    op.out = y.buf;
    e.push(op);
    return y;
}

static void register_unused_conv_bn(Engine& e, const std::string& conv, const std::string& bn, int Cout, int Cin,
                                    int ks) {
    e.add_param(conv + ".weight", CAPF_P_CONV_W, {Cout, Cin, ks, ks});
    reg_bn(e, bn, Cout);
}

void Engine::build_cpn(Tensor img, Tensor feats[4]) {
    const std::string R = "backbone.resnet";
    Tensor x = conv_bn(R + ".conv1", R + ".bn1", img, 64, 7, 2, ACT_RELU, nullptr);       // resnet.py:137-139
    x = pool_or_resize(*this, OP_MAXPOOL, R + ".maxpool", x, (x.H + 2 - 3) / 2 + 1, (x.W + 2 - 3) / 2 + 1);
    const int nblk[4] = {3, 4, 6, 3}, planes[4] = {64, 128, 256, 512}, strides[4] = {1, 2, 2, 2};
    Tensor c[4];
    for (int li = 0; li < 4; ++li) {
        for (int k = 0; k < nblk[li]; ++k) {                                               // :58-93, :119-133
            const std::string p = R + ".layer" + std::to_string(li + 1) + "." + std::to_string(k);
            const int st = (k == 0) ? strides[li] : 1;
            const int fork_at = (int)ops.size();
            if (k == 0) fork(2);         // projection shortcut: independent of conv1 / conv2
            Tensor y = conv_bn(p + ".conv1", p + ".bn1", x, planes[li], 1, 1, ACT_RELU, nullptr);
            y = conv_bn(p + ".conv2", p + ".bn2", y, planes[li], 3, st, ACT_RELU, nullptr);
            Tensor r = x;
            if (k == 0) {
                set_lane(1);
                r = conv_bn(p + ".downsample.0", p + ".downsample.1", x, planes[li] * 4, 1, st, ACT_NONE, nullptr);
                join();
            }
            x = conv_bn(p + ".conv3", p + ".bn3", y, planes[li] * 4, 1, 1, ACT_RELU, &r);
            if (k == 0 && st == 1) bneck0_mark(*this, fork_at);
            if (k > 0) bneck1_mark(*this, fork_at);
        }
        c[li] = x;
    }
    // globalNet.forward (globalNet.py:61-83); res_out = [x4,x3,x2,x1]
    const std::string G = "backbone.global_net";
    Tensor fms[4];
    for (int i = 0; i < 4; ++i) {
        const Tensor& src = c[3 - i];
        const std::string lp = G + ".laterals." + std::to_string(i);
        if (i > 0 && b16() && plan.use_upadd) {
            // bf16: the low-resolution conv of the upsampled path first, then the lateral conv with `+ bilinear_x2(t)` behind its ReLU in the
            // epilogue (igemm_bf16_kernel<.., UPADD>): no resize-add launch, the lateral map never travels to HBM and back on its own
            // (lateral: write + read of 453 MB at the largest level and batch 128), and it meets the upsampled term in fp32
            const std::string upn = G + ".upsamples." + std::to_string(i - 1);
            Tensor t = conv_bn(upn + ".1", upn + ".2", fms[i - 1], 256, 1, 1, ACT_NONE, nullptr);
            ops.back().flops_per_frame *= 4.0;
            fms[i] = conv_bn(lp + ".0", lp + ".1", src, 256, 1, 1, ACT_RELU, nullptr);
            Op& lop = ops.back();
            lop.up_in = t.buf; lop.up_H = t.H; lop.up_W = t.W;
            bufs[t.buf].last_op = std::max(bufs[t.buf].last_op, (int)ops.size() - 1);
            const std::string pp = G + ".predict." + std::to_string(i);
            register_unused_conv_bn(*this, pp + ".0", pp + ".1", 256, 256, 1);
            register_unused_conv_bn(*this, pp + ".3", pp + ".5", 17, 256, 3);
            continue;
        }
        Tensor lat = conv_bn(lp + ".0", lp + ".1", src, 256, 1, 1, ACT_RELU, nullptr);
        if (i == 0) {
            fms[i] = lat;
        } else {
            // reference: up = BN(conv1x1(bilinear x2(feature_{i-1}))), feature_i = lateral_i + up (globalNet.py:40-46, :66).  A
            // 1x1 conv without bias + eval-mode BN is a per-pixel affine map and bilinear interpolation is a convex combination
            // of pixels, so the two COMMUTE exactly in real arithmetic: the conv runs on the LOW-resolution map (a quarter of
            // the pixels: 116 -> 29 GFLOP and 300 -> 75 us for the largest level at batch 128), the resize adds the lateral.
            const std::string upn = G + ".upsamples." + std::to_string(i - 1);
            Tensor t = conv_bn(upn + ".1", upn + ".2", fms[i - 1], 256, 1, 1, ACT_NONE, nullptr);
            ops.back().flops_per_frame *= 4.0;       // ALGORITHMIC FLOPs stay the reference's (conv at the upsampled resolution,
                                                     // SURVEY 8d); capf_op_executed_flops reports what runs (rows_per_frame)
            fms[i] = pool_or_resize(*this, OP_RESIZE, upn + ".0", t, t.H * 2, t.W * 2, &lat);
        }
        // predict heads: computed-then-discarded by the reference (:71) -> parameters only
        const std::string pp = G + ".predict." + std::to_string(i);
        register_unused_conv_bn(*this, pp + ".0", pp + ".1", 256, 256, 1);
        register_unused_conv_bn(*this, pp + ".3", pp + ".5", 17, 256, 3);
    }
    // refineNet.forward (refineNet.py:72-88)
    const std::string F = "backbone.refine_net";
    const int oh = 64, ow = 48;   // cpn/test_config.py:24 output_shape
    fork(4);                      // the four cascades are independent
    for (int i = 0; i < 4; ++i) {
        set_lane(i);
        Tensor y = fms[i];
        for (int k = 0; k < 3 - i; ++k) {
            const std::string p = F + ".cascade." + std::to_string(i) + "." + std::to_string(k);
            Tensor t = conv_bn(p + ".conv1", p + ".bn1", y, 128, 1, 1, ACT_RELU, nullptr);
            t = conv_bn(p + ".conv2", p + ".bn2", t, 128, 3, 1, ACT_RELU, nullptr);
            Tensor r = conv_bn(p + ".downsample.0", p + ".downsample.1", y, 256, 1, 1, ACT_NONE, nullptr);
            y = conv_bn(p + ".conv3", p + ".bn3", t, 256, 1, 1, ACT_RELU, &r);
        }
        // cascade 3 is nn.Upsample alone (refineNet.py:58-64 with num = 0) on a map that already has output_shape: under align_corners the
        // source index of output pixel i is i * (H - 1) / (H - 1) = i with weight 1 (ATen: lambda 0 -> 1 * x[i] + 0 * x[i + 1]), the identity for
        // finite values -- the level IS the lateral map; no launch, no second copy of it (201 MB written + read back at batch 128)
        if (y.H == oh && y.W == ow) { feats[i] = y; continue; }
        feats[i] = pool_or_resize(*this, OP_RESIZE, F + ".cascade." + std::to_string(i) + ".resize", y, oh, ow);
    }
    join();
    const std::string fp = F + ".final_predict";
    if (cfg.plan_flags & CAPF_PLAN_CPN_PREDICT) {
        // CPN's own detector head (refineNet.py:64-70, :86-88): final_predict(torch.cat(refine_fms, 1)) = Bottleneck(1024 -> 128 -> 256), then
        // conv3x3(256 -> 17) + BatchNorm, no activation.  The parameters register in the order of the unflagged plan (same schema).
        // The concatenation is a copy into a buffer of its own: feat0..3 stay where and what they are (the lifter samples them)
        Tensor cat{-1, oh, ow, 0};
        Op op;
        op.kind = OP_CONCAT;
        op.name = fp + ".cat";
        op.n_in = 4;
        for (int i = 0; i < 4; ++i) {
            op.in[i] = feats[i].buf;
            use(feats[i].buf);
            cat.C += feats[i].C;
        }
        op.H = oh; op.W = ow; op.C = feats[0].C; op.Ho = oh; op.Wo = ow;
        op.bf16 = b16() ? 1 : 0;
        cat.buf = new_buffer(act_elems((size_t)oh * ow * cat.C), op.name);
        op.out = cat.buf;
        push(op);
        fork(2);                  // the projection shortcut only reads the concatenation
        Tensor t = conv_bn(fp + ".0.conv1", fp + ".0.bn1", cat, 128, 1, 1, ACT_RELU, nullptr);
        t = conv_bn(fp + ".0.conv2", fp + ".0.bn2", t, 128, 3, 1, ACT_RELU, nullptr);
        // (conv3 is REGISTERED ahead of the downsample pair, as nn.Module orders a Bottleneck's children and the unflagged plan does)
        const std::string c3 = fp + ".0.conv3", b3 = fp + ".0.bn3";
        add_param(c3 + ".weight", CAPF_P_CONV_W, {256, 128, 1, 1});
        reg_bn(*this, b3, 256);
        set_lane(1);
        Tensor r = conv_bn(fp + ".0.downsample.0", fp + ".0.downsample.1", cat, 256, 1, 1, ACT_NONE, nullptr);
        join();
        t = conv_bn(c3, b3, t, 256, 1, 1, ACT_RELU, &r);
        // 17 output channels fit no conv kernel's width rule (N % 4 == 0): the pack carries 20 rows, three of them zero, and the map 20 channels
        Tensor heat = conv_bn(fp + ".1", fp + ".2", t, 17, 3, 1, ACT_NONE, nullptr, 20);
        name_tensor(*this, "heat", heat.buf, {-1, heat.H, heat.W, heat.C}, maps_bf16() ? dt16() : 0);
        return;
    }
    // final_predict is never called (:76-88): parameters only
    register_unused_conv_bn(*this, fp + ".0.conv1", fp + ".0.bn1", 128, 1024, 1);
    register_unused_conv_bn(*this, fp + ".0.conv2", fp + ".0.bn2", 128, 128, 3);
    register_unused_conv_bn(*this, fp + ".0.conv3", fp + ".0.bn3", 256, 128, 1);
    register_unused_conv_bn(*this, fp + ".0.downsample.0", fp + ".0.downsample.1", 256, 1024, 1);
    register_unused_conv_bn(*this, fp + ".1", fp + ".2", 17, 256, 3);
}

// ---------------------------------------------------------------------------------------------------
// lifter (pose_dformer.py)
// ---------------------------------------------------------------------------------------------------
static LinearRef reg_linear(Engine& e, const std::string& p, int N, int K) {
    LinearRef r;
    r.w = e.add_param(p + ".weight", CAPF_P_LIN_W, {N, K});
    r.b = e.add_param(p + ".bias", CAPF_P_LIN_B, {N});
    r.N = N;
    r.K = K;
    return r;
}

static LnRef reg_ln(Engine& e, const std::string& p, int C) {
    LnRef r;
    r.w = e.add_param(p + ".weight", CAPF_P_LN_W, {C});
    r.b = e.add_param(p + ".bias", CAPF_P_LN_B, {C});
    return r;
}

static int make_linear_pack(Engine& e, std::initializer_list<LinearRef> lins, bool as_bf16 = false, bool quad = false) {
    Pack pk;
    pk.kind = LINEAR;
    pk.quad = quad;
    int N = 0, K = 0;
    for (const LinearRef& r : lins) {
        pk.w[pk.n_lin] = r.w;
        pk.b[pk.n_lin++] = r.b;
        N += r.N;
        K = r.K;
    }
    pk.N = N;
    pk.K = K;
    pk.Kpad = as_bf16 ? round64(K) : round32(K);
    if (quad) pk.Kpad = K;                     // (K % 4 == 0: embed dims and level channel counts)
    pk.in_place = !as_bf16 && !quad && (pk.n_lin == 1 && pk.Kpad == K);
    pk.bf16 = as_bf16;                         // bf16 copy [N][Kpad] for the bf16 MFMA projections (compute_dtype = bf16)
    // the fp32 projections also as two fp16 pieces for igemm_f32h2.hip, packed LAZILY (Engine::ensure_h2g_lifter): a training loop changes the
    // weights every step and its forward runs train.cpp's GEMMs, so the copy is rebuilt only when an inference forward needs it
    if (!as_bf16 && !quad && e.plan.use_h2g && !e.b16() && K % 4 == 0 && N % 4 == 0) { pk.h2g = true; pk.h2g_Kpad = round32(K); }
    e.packs.push_back(pk);
    return (int)e.packs.size() - 1;
}

static int make_chain_pack(Engine& e, const LinearRef& lin) {   // a linear of lifter_chain.hip: the two-piece copy in fragment order as well
    const int pk = make_linear_pack(e, {lin});
    e.packs[pk].chain = true;
    return pk;
}

// rows-mode GEMM:  out[omap(m) + n] = act(A[amap(m)] . W[n] + b[n] + res[rmap(m) + n])
static void gemm_rows(Engine& e, const std::string& name, int pack, int a_buf, RowMap amap, long rows_pf, int out_buf,
                      RowMap omap, int act, int res_buf, RowMap rmap, int res_param = -1, LnRef ln = LnRef{}, float ln_eps = 0.f) {
    const Pack& pk = e.packs[pack];
    Op op;
    op.kind = OP_GEMM;
    op.name = name;
    op.conv = 0;
    op.pack = pack;
    op.in[0] = a_buf;
    op.amap = amap;
    op.rows_per_frame = rows_pf;
    op.N = pk.N; op.K = pk.K; op.act = act;
    op.out = out_buf;
    op.omap = omap;
    op.aux = res_buf;
    op.rmap = rmap;
    op.res_param = res_param;
    if (ln.w >= 0) {                         // LayerNorm(A rows) folded into the GEMM's fragment path (igemm_f32.hip, LNA)
        op.ln = ln;
        op.eps = ln_eps;
    }
    op.flops_per_frame = 2.0 * rows_pf * (double)pk.N * pk.K;
    if (pk.kind == LINEAR && pk.bf16) {           // bf16 operands (A buffer holds bf16 rows), fp32 accumulate
        op.bf16 = 2;
        op.out_bf16 = act == ACT_GELU ? 1 : 0;   // fc1: GELU, bf16 hidden rows; everything else lands in the fp32 stream
    }
    e.use(a_buf);
    e.use(res_buf);
    e.use(out_buf);
    e.push(op);
}

static void layernorm(Engine& e, const std::string& name, LnRef ln, float eps, int in_buf, RowMap imap,
                      int add_buf, RowMap amap, int out_buf, long rows_pf, int C, bool out_bf16 = false) {
    Op op;
    op.kind = OP_LAYERNORM;
    op.name = name;
    op.in[0] = in_buf;
    op.amap = imap;
    op.aux = add_buf;
    op.rmap = amap;
    op.out = out_buf;
    op.ln = ln;
    op.eps = eps;
    op.rows_per_frame = rows_pf;
    op.C = C;
    op.out_bf16 = out_bf16 ? 1 : 0;
    e.use(in_buf);
    e.use(add_buf);
    e.use(out_buf);
    e.push(op);
}

static void debug_copy(Engine& e, const std::string& name, int src, size_t elems, std::initializer_list<int64_t> shape) {
    Op op;
    op.kind = OP_FUSE;       // a 1-input fuse without ReLU is a plain copy
    op.name = "copy." + name;
    op.n_in = 1;
    op.in[0] = src;
    op.H = 1; op.W = 1; op.C = (int)elems; op.relu = 0;
    op.debug_only = true;
    e.use(src);
    op.out = e.new_buffer(elems, name);
    e.push(op);
    name_tensor(e, name, op.out, shape);
}

void Engine::build_lifter(const Tensor feats[4]) {
    const std::string V = "volume_net";
    const int J = cfg.num_joints, L = cfg.levels, L1 = L + 1, C = cfg.embed_dim_ratio, D = C * L1;
    const int NH = cfg.deform_heads, NS = cfg.deform_samples, HD = C / NH;
    int Cl[4];
    for (int l = 0; l < L; ++l) Cl[l] = feats[l].C;

    // ---- schema, in the reference's registration order (pose_dformer.py:174-208), resolved into `lifter`: the only place that spells the
    // lifter's parameter names -- everything below, and the training step (train.cpp), goes by the indices kept here
    LifterSchema& net = lifter;
    net = LifterSchema{};
    net.pos = add_param(V + ".Spatial_pos_embed", CAPF_P_RAW, {1, L1, J, C});
    net.coord = reg_linear(*this, V + ".coord_embed", C, 2);
    for (int l = 0; l < L; ++l) net.feat_embed[l] = reg_linear(*this, V + ".feat_embed." + std::to_string(l), C, Cl[l]);
    auto reg_mlp = [&](const std::string& p, int dim) {
        LifterMlp m;
        m.norm2 = reg_ln(*this, p + ".norm2", dim);
        m.fc1 = reg_linear(*this, p + ".mlp.fc1", 2 * dim, dim);
        m.fc2 = reg_linear(*this, p + ".mlp.fc2", dim, 2 * dim);
        return m;
    };
    auto reg_block = [&](const std::string& p, int dim) {
        LifterAtt a;
        a.norm1 = reg_ln(*this, p + ".norm1", dim);
        a.qkv = reg_linear(*this, p + ".attn.qkv", 3 * dim, dim);
        a.proj = reg_linear(*this, p + ".attn.proj", dim, dim);
        a.mlp = reg_mlp(p, dim);
        return a;
    };
    const int DEP = depth();                               // blocks per group (ContextPose_mpi pose_dformer.py:199)
    for (int i = 0; i < DEP; ++i) net.joint[i] = reg_block(V + ".joint_blocks." + std::to_string(i), D);
    for (int i = 0; i < DEP; ++i) net.res[i] = reg_block(V + ".res_blocks." + std::to_string(i), C);
    if (cfg.context_blocks) {
        for (int i = 0; i < L; ++i) {
            const std::string p = V + ".context_blocks." + std::to_string(i);
            LifterCtx& c = net.ctx[i];
            c.norm1 = reg_ln(*this, p + ".norm1", C);
            c.aw = reg_linear(*this, p + ".attention_weights", NH * NS, C);
            c.so = reg_linear(*this, p + ".sampling_offsets", 2 * NH * NS, C);
            for (int l = 0; l < L; ++l) c.embed_proj[l] = reg_linear(*this, p + ".embed_proj." + std::to_string(l), HD, Cl[l]);
            c.mlp = reg_mlp(p, C);
        }
    }
    net.head_ln = reg_ln(*this, V + ".head.0", D);
    net.head = reg_linear(*this, V + ".head.1", 3, D);

    // ---- buffers (per frame)
    const int X = new_buffer((size_t)J * D, "tokens");            // [J, L1, C]  ("b p l c")
    const int Q = new_buffer((size_t)J * D, "ln_out");
    const int Hb = new_buffer((size_t)J * 2 * D, "mlp_hidden");
    const int QKV = new_buffer((size_t)J * 3 * D, "qkv");
    const int O = new_buffer((size_t)J * D, "attn_out");
    keep(*this, X); keep(*this, Q); keep(*this, Hb); keep(*this, QKV); keep(*this, O);

    // ---- embedding + reference-point sampling (pose_dformer.py:214-226)
    // LayerNorm folded into the following GEMM (igemm_f32.hip, LNA) where the normalised width is small: every block
    // recomputes the statistics of its own rows, which is free at K = 128 (norm + GEMM 22.7 -> 18.3 us at batch 64) and
    // a loss at K = 640, where 30 column tiles would each re-read 160 KB of rows (29 + 9.5 -> 44 us): the joint
    // blocks keep their LayerNorm launch
    // (compute_dtype = bf16: the projections take bf16 A rows, which the LayerNorm kernel writes directly)
    // lifter projections (qkv / proj / fc1 / fc2) on the bf16 MFMA path; CAPF_PLAN_LIFTER_FP32 keeps them (and their LayerNorm folding) fp32
    const bool lb = b16() && !(cfg.plan_flags & CAPF_PLAN_LIFTER_FP32);
    auto ln_fold_ok = [&](int dim) { return plan.fused_lifter && dim <= 256 && !lb; };
    const bool ln_fold = ln_fold_ok(C);
    // the MLP half of a block on the rows `xm` of X, x += fc2(gelu(fc1(norm2(x)))), in the form the caller chose: one launch (lifter_chain.hip,
    // ATTN = false), else norm2 folded into fc1, else a LayerNorm launch in front of fc1.  fc1 and fc2 get their packs in this order in every form
    auto mlp_half = [&](const LifterMlp& m, const std::string& n, RowMap xm, long rows_pf, int dim, float eps, bool chain, bool ln_fold) {
        if (chain) {
            Op op;
            op.kind = OP_MLP_CHAIN;
            op.name = n + ".mlp";
            op.in[0] = X;
            op.out = X;
            op.amap = xm;
            op.C = dim;
            op.eps = eps;
            op.rows_per_frame = rows_pf;
            ChainBlock blk;
            blk.fc1 = make_chain_pack(*this, m.fc1);
            blk.fc2 = make_chain_pack(*this, m.fc2);
            blk.norm2 = m.norm2;
            op.blocks.push_back(blk);
            op.flops_per_frame = 2.0 * rows_pf * (double)dim * (2 * dim + 2 * dim);
            use(X);
            push(op);
            has_res_chain = true;
            return;
        }
        if (ln_fold) {
            gemm_rows(*this, n + ".fc1", make_linear_pack(*this, {m.fc1}), X, xm, rows_pf, Hb, row_ld(2 * dim), ACT_GELU, -1, row_ld(0), -1,
                      m.norm2, eps);
        } else {
            layernorm(*this, n + ".norm2", m.norm2, eps, X, xm, -1, row_ld(0), Q, rows_pf, dim, lb);
            gemm_rows(*this, n + ".fc1", make_linear_pack(*this, {m.fc1}, lb), Q, row_ld(dim), rows_pf, Hb, row_ld(2 * dim), ACT_GELU, -1,
                      row_ld(0));
        }
        gemm_rows(*this, n + ".fc2", make_linear_pack(*this, {m.fc2}, lb), Hb, row_ld(2 * dim), rows_pf, X, xm, ACT_NONE, X, xm);
    };
    if (plan.fused_lifter) {
        Op op;
        op.kind = OP_EMBED;
        op.name = "embed";
        op.out = X;
        op.coord = net.coord;
        op.pos = net.pos;
        op.smp.J = J; op.smp.L = L; op.smp.L1 = L1; op.C = C;
        op.bf16 = b16() ? 1 : 0;
        op.feat_bf16 = feat_fmt();
        use(X);
        for (int l = 0; l < L; ++l) {
            const std::string ls = std::to_string(l);
            op.in[l] = feats[l].buf;
            op.lvlH[l] = feats[l].H; op.lvlW[l] = feats[l].W; op.lvlC[l] = Cl[l];
            use(feats[l].buf);
            op.pb[l] = net.feat_embed[l].b;
            op.pq[l] = make_linear_pack(*this, {net.feat_embed[l]}, false, true);
            op.outs[l] = new_buffer((size_t)J * Cl[l], "sampled" + ls);
            op.idx_lvl[l] = new_buffer((size_t)J * 2, "idx" + ls);
            name_tensor(*this, "sampled" + ls, op.outs[l], {-1, J, Cl[l]});
            name_tensor(*this, "idx" + ls, op.idx_lvl[l], {-1, J, 2}, 1);
            op.flops_per_frame += 2.0 * J * (double)C * Cl[l];
        }
        push(op);
    } else {
    {
        Op op;
        op.kind = OP_PREP_EMBED;
        op.name = "prep_embed";
        op.out = X;
        op.coord = net.coord;
        op.pos = net.pos;
        op.smp.J = J; op.smp.L1 = L1; op.C = C;
        use(X);
        push(op);
    }
    for (int l = 0; l < L; ++l) {
        const std::string ls = std::to_string(l);
        Op op;
        op.kind = OP_SAMPLE_REF;
        op.name = "sample_ref." + ls;
        op.in[0] = feats[l].buf;
        op.H = feats[l].H; op.W = feats[l].W; op.C = Cl[l]; op.smp.J = J;
        op.bf16 = b16() ? 1 : 0;
        op.feat_bf16 = feat_fmt();
        use(feats[l].buf);
        const int S = new_buffer((size_t)J * Cl[l], "sampled" + ls);
        const int I = new_buffer((size_t)J * 2, "idx" + ls);
        op.out = S;
        op.idx_out = I;
        push(op);
        name_tensor(*this, "sampled" + ls, S, {-1, J, Cl[l]});
        name_tensor(*this, "idx" + ls, I, {-1, J, 2}, 1);
        const int pk = make_linear_pack(*this, {net.feat_embed[l]});
        // out X[b,p,1+l,:] = S W^T + b + pos[0,1+l,p,:]
        gemm_rows(*this, "feat_embed." + ls, pk, S, row_ld(Cl[l]), J, X, row_ld(D, (long)(1 + l) * C), ACT_NONE, -1,
                  RowMap{J, 0, C, (long)(1 + l) * J * C}, net.pos);
    }
    }

    // ---- deformable context blocks (pose_dformer.py:115-141), tokens 1..L with token 0 as query bias
    if (cfg.context_blocks) {
        const int AO = new_buffer((size_t)J * L * 3 * NH * NS, "attn_off");
        keep(*this, AO);
        int U[4];
        for (int l = 0; l < L; ++l) {
            U[l] = new_buffer((size_t)J * NH * Cl[l], "deform_u" + std::to_string(l));
            keep(*this, U[l]);
        }
        const RowMap tok{L, D, C, C};           // row (b,p,l') -> X[b,p,1+l',:]
        const RowMap tok0{L, D, 0, 0};          // row (b,p,l') -> X[b,p,0,:]
        for (int i = 0; i < L; ++i) {
            LifterCtx& c = net.ctx[i];
            const std::string n = "ctx" + std::to_string(i);
            const int pk_ao = c.ao_pack = make_linear_pack(*this, {c.aw, c.so});   // (row layout: the training step's GEMMs, train.cpp)
            // debug taps of the border-mode sampling site (pose_dformer.py:126-128): positions and NW corner indices
            const int tap_pos = c.tap_pos = new_buffer((size_t)J * L * NH * NS * 2, "cpos" + std::to_string(i));
            const int tap_idx = c.tap_idx = new_buffer((size_t)J * L * NH * NS * 2, "cidx" + std::to_string(i));
            name_tensor(*this, "cpos" + std::to_string(i), tap_pos, {-1, J, L * NH * NS, 2});
            name_tensor(*this, "cidx" + std::to_string(i), tap_idx, {-1, J, L * NH * NS, 2}, 1);
            if (plan.fused_lifter) {
                Op op;
                op.kind = OP_CTX_ATTN;
                op.name = n + ".attn";
                op.pack = make_linear_pack(*this, {c.aw, c.so}, false, true);
                op.out = X;
                use(X);
                op.ln = c.norm1;
                op.eps = 1e-5f;
                for (int l = 0; l < L; ++l) {
                    op.in[l] = feats[l].buf;
                    op.lvlH[l] = feats[l].H; op.lvlW[l] = feats[l].W; op.lvlC[l] = Cl[l];
                    use(feats[l].buf);
                    op.pb[l] = c.embed_proj[l].b;
                    op.pq[l] = make_linear_pack(*this, {c.embed_proj[l]}, false, true);
                    op.outs[l] = U[l];           // (the sample sums cross HBM to the embed_proj launch: lifter_fused.hip ctx_proj_kernel)
                    use(U[l]);
                    op.flops_per_frame += 2.0 * J * NH * (double)HD * Cl[l];
                }
                op.flops_per_frame += 2.0 * J * L * (double)C * 3 * NH * NS;
                op.smp.J = J; op.smp.L = L; op.smp.NH = NH; op.smp.NS = NS; op.C = C;
                op.bf16 = b16() ? 1 : 0;
                op.feat_bf16 = feat_fmt();
                op.tap_pos = tap_pos; op.tap_idx = tap_idx;
                push(op);
            } else {
            layernorm(*this, n + ".norm1", c.norm1, 1e-5f, X, tok, X, tok0, Q, (long)J * L, C);
            gemm_rows(*this, n + ".attn_off", pk_ao, Q, row_ld(C), (long)J * L, AO, row_ld(3 * NH * NS), ACT_NONE, -1,
                      row_ld(0));
            {
                Op op;
                op.kind = OP_DEFORM;
                op.name = n + ".deform";
                op.aux = AO;
                use(AO);
                for (int l = 0; l < L; ++l) {
                    op.in[l] = feats[l].buf;
                    op.lvlH[l] = feats[l].H; op.lvlW[l] = feats[l].W; op.lvlC[l] = Cl[l];
                    op.outs[l] = U[l];
                    use(feats[l].buf);
                    use(U[l]);
                }
                op.smp.J = J; op.smp.L = L; op.smp.NH = NH; op.smp.NS = NS;
                op.bf16 = b16() ? 1 : 0;
                op.feat_bf16 = feat_fmt();
                op.tap_pos = tap_pos; op.tap_idx = tap_idx;
                push(op);
            }
            for (int l = 0; l < L; ++l) {
                const int pk = make_linear_pack(*this, {c.embed_proj[l]});
                const RowMap dst{NH, D, HD, (long)(1 + l) * C};    // row (b,p,h) -> X[b,p,1+l,h*HD:]
                gemm_rows(*this, n + ".embed_proj." + std::to_string(l), pk, U[l], row_ld(Cl[l]), (long)J * NH, X, dst,
                          ACT_NONE, X, dst);
            }
            }
            // the MLP half as one launch on the context tokens' rows where the chain kernel takes the width
            const bool mlp_chain = plan.fused_lifter && plan.use_h2g && !lb && !b16() && res_chain_ok(C, 5, 8, 1);
            mlp_half(c.mlp, n, tok, (long)J * L, C, 1e-5f, mlp_chain, ln_fold);
        }
    }
    debug_copy(*this, "tok_ctx", X, (size_t)J * D, {-1, J, L1, C});

    // ---- Block x L over the L1 level-tokens of each joint, then over the J joint tokens (:231-238)
    auto attn_blocks = [&](const LifterAtt* blocks, const std::string& tag, int dim, long rows_pf, int tokens, int groups_pf) {
        const bool ln_fold = ln_fold_ok(dim);
        const int nblk = DEP;
        // the res blocks (tokens of ONE joint, 128 wide) as one launch: a workgroup takes 6 joints through every block without leaving
        // the CU (lifter_chain.hip); fp32 lifter on the two-piece packs only -- the bf16 plan and CAPF_PLAN_NO_FUSED_LIFTER /
        // CAPF_PLAN_NO_F32H2_GEMM keep one launch per op
        if (plan.fused_lifter && plan.use_h2g && !lb && !b16() && groups_pf > 1 && res_chain_ok(dim, tokens, cfg.num_heads, nblk)) {
            Op op;
            op.kind = OP_RES_CHAIN;
            op.name = tag + ".chain";
            op.in[0] = X;
            op.out = X;
            op.attn.tokens = tokens; op.attn.heads = cfg.num_heads; op.C = dim;
            op.eps = 1e-6f;
            op.rows_per_frame = rows_pf;
            for (int i = 0; i < nblk; ++i) {
                const LifterAtt& a = blocks[i];
                ChainBlock blk;
                blk.qkv = make_chain_pack(*this, a.qkv);
                blk.proj = make_chain_pack(*this, a.proj);
                blk.fc1 = make_chain_pack(*this, a.mlp.fc1);
                blk.fc2 = make_chain_pack(*this, a.mlp.fc2);
                blk.norm1 = a.norm1;
                blk.norm2 = a.mlp.norm2;
                op.blocks.push_back(blk);
                op.flops_per_frame += 2.0 * rows_pf * (double)dim * (3 * dim + dim + 2 * dim + 2 * dim) + 4.0 * groups_pf * tokens * tokens * dim;
            }
            use(X);
            push(op);
            has_res_chain = true;
            return;
        }
        for (int i = 0; i < nblk; ++i) {
            const LifterAtt& a = blocks[i];
            const std::string n = tag + std::to_string(i);
            if (ln_fold) {
                gemm_rows(*this, n + ".qkv", make_linear_pack(*this, {a.qkv}), X, row_ld(dim), rows_pf, QKV,
                          row_ld(3 * dim), ACT_NONE, -1, row_ld(0), -1, a.norm1, 1e-6f);
            } else {
                layernorm(*this, n + ".norm1", a.norm1, 1e-6f, X, row_ld(dim), -1, row_ld(0), Q, rows_pf, dim, lb);
                gemm_rows(*this, n + ".qkv", make_linear_pack(*this, {a.qkv}, lb), Q, row_ld(dim), rows_pf, QKV,
                          row_ld(3 * dim), ACT_NONE, -1, row_ld(0));
            }
            {
                Op op;
                op.kind = OP_ATTENTION;
                op.name = n + ".attn";
                op.in[0] = QKV;
                op.out = O;
                op.attn = Attn{groups_pf, tokens, cfg.num_heads, dim / cfg.num_heads};
                op.flops_per_frame = 4.0 * groups_pf * tokens * tokens * dim;
                op.out_bf16 = lb ? 1 : 0;      // the attention output is only ever the A operand of proj
                use(QKV); use(O);
                push(op);
            }
            gemm_rows(*this, n + ".proj", make_linear_pack(*this, {a.proj}, lb), O, row_ld(dim), rows_pf, X,
                      row_ld(dim), ACT_NONE, X, row_ld(dim));
            mlp_half(a.mlp, n, row_ld(dim), rows_pf, dim, 1e-6f, false, ln_fold);   // (never a chain of its own: inside OP_RES_CHAIN, or unfused)
        }
    };
    attn_blocks(net.res, "res", C, (long)J * L1, L1, J);
    debug_copy(*this, "tok_res", X, (size_t)J * D, {-1, J, L1, C});
    attn_blocks(net.joint, "joint", D, (long)J, J, 1);
    debug_copy(*this, "tok_joint", X, (size_t)J * D, {-1, J, L1, C});

    {   // head (:240)
        Op op;
        op.kind = OP_HEAD;
        op.name = "head";
        op.in[0] = X;
        op.ln = net.head_ln;
        op.head = net.head;
        op.eps = 1e-5f;
        op.rows_per_frame = J;
        op.C = D;
        op.flops_per_frame = 2.0 * J * D * 3;
        use(X);
        push(op);
    }
}

// CAPF_PLAN_BF16_F32_STREAM: where each backbone tensor lives, decided from its readers ("bf16 only as MFMA operands, residual stream
// fp32").  A tensor every reader of which is a conv's operand stays bf16 (conv1 of a BasicBlock, the stem, the ReLU'd middle links of the fuse
// layers' stride-2 chains, layer1's conv1 / conv2): nobody reads its fp32 value.  A tensor with any other reader -- a residual add, a fuse-sum
// input, a context map of the lifter -- is stored fp32 by its producer; if convs read it too, the producer also writes its bf16 rounding (the
// "shadow") in the same epilogue and those convs take that as their operand.  So every conv keeps its bf16 operand path (the 2-D halo tile
// stages bf16 pixels by LDS-DMA, which cannot convert); only epilogues change.  Every backbone bf16 conv runs the fp32-stream epilogue.
bool Engine::plan_f32_stream(const Tensor feats[4]) {
    const int n = (int)ops.size(), nb = (int)bufs.size();
    std::vector<int> prod(nb, -1), conv_last(nb, -1);
    std::vector<char> other(nb, 0);
    for (int i = 0; i < n; ++i) {
        const Op& op = ops[i];
        if (op.kind == OP_FORK || op.kind == OP_JOIN) continue;
        if (op.kind != OP_GEMM && op.kind != OP_FUSE) {
            err = "CAPF_PLAN_BF16_F32_STREAM: unexpected backbone op " + op.name;
            return false;
        }
        if (op.out >= 0) prod[op.out] = i;
        const auto rd = op.reads();                      // a conv's first read is its operand; every other read wants the fp32 value
        for (size_t k = 0; k < rd.size(); ++k) {
            if (rd[k] < 0) continue;
            if (op.kind == OP_GEMM && k == 0) conv_last[rd[k]] = i;
            else other[rd[k]] = 1;
        }
    }
    for (int l = 0; l < 4; ++l) other[feats[l].buf] = 1;
    for (int b = 0; b < nb; ++b) {
        if (!other[b]) continue;
        if (prod[b] < 0 || !(ops[prod[b]].kind == OP_FUSE || ops[prod[b]].bf16 == 1)) {
            err = "CAPF_PLAN_BF16_F32_STREAM: a residual / fuse / context-map tensor without a bf16 conv or fuse-sum producer";
            return false;
        }
        Op& p = ops[prod[b]];
        const size_t elems = p.kind == OP_FUSE ? (size_t)p.H * p.W * p.C : (size_t)p.Ho * p.Wo * p.N;
        p.st_f32 = 1;
        bufs[b].elems = round64(elems);
        if (conv_last[b] < 0) continue;
        const int sh = new_buffer((elems + 1) / 2, bufs[b].tag + ".bf16");
        bufs[sh].def_op = prod[b];
        bufs[sh].last_op = conv_last[b];
        p.sh = sh;
        for (int i = prod[b] + 1; i <= conv_last[b]; ++i)
            if (ops[i].kind == OP_GEMM && ops[i].in[0] == b) ops[i].in[0] = sh;
    }
    for (Op& op : ops) {
        if (op.kind == OP_GEMM && op.bf16 == 1) op.f32s = 1;
        if (op.kind == OP_FUSE) op.bf16 = 0;             // fp32 terms in, fp32 sum out (+ shadow)
    }
    return true;
}

// Greedy offset assignment over buffer lifetimes (ops run in order on one stream).
void Engine::assign_offsets() {
    struct Live { size_t off, size; int last; };
    std::vector<int> order(bufs.size());
    for (size_t i = 0; i < bufs.size(); ++i) order[i] = (int)i;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return bufs[a].def_op < bufs[b].def_op; });
    // Ops of different lanes of a fork/join region run concurrently: a buffer whose life touches a region
    // stays allocated for the whole region (no reuse across lanes while they may overlap).
    for (Buffer& b : bufs)
        for (const auto& rg : regions) {
            const bool touches = b.def_op <= rg.second && b.last_op >= rg.first;
            if (touches && b.last_op < rg.second) b.last_op = rg.second;
            if (touches && b.def_op > rg.first) b.def_op = rg.first;
        }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return bufs[a].def_op < bufs[b].def_op; });
    std::vector<Live> live;
    size_t top = 0;
    for (int id : order) {
        Buffer& b = bufs[id];
        live.erase(std::remove_if(live.begin(), live.end(), [&](const Live& l) { return l.last < b.def_op; }), live.end());
        std::sort(live.begin(), live.end(), [](const Live& x, const Live& y) { return x.off < y.off; });
        size_t off = 0;
        for (const Live& l : live) {
            if (off + b.elems <= l.off) break;
            off = std::max(off, l.off + l.size);
        }
        b.offset = off;
        live.push_back(Live{off, b.elems, b.last_op});
        top = std::max(top, off + b.elems);
    }
    ws_elems_per_frame = top;
}

// Dependency levels of every fork/join region (run_region_grouped): an op's level is one more than the
// highest level of any earlier op of the region it conflicts with on a buffer (read-after-write,
// write-after-read, write-after-write).
void Engine::schedule_regions() {
    region_levels.assign(regions.size(), {});
    for (size_t r = 0; r < regions.size(); ++r) {
        const int lo = regions[r].first + 1, hi = regions[r].second;
        std::vector<int> level(hi - lo, 0);
        auto has = [](const auto& slots, int b) { return std::find(slots.begin(), slots.end(), b) != slots.end(); };
        auto reads = [&](const Op& o, int b) { return has(o.reads(), b); };
        auto writes = [&](const Op& o, int b) { return has(o.writes(), b); };
        auto touched = [&](const Op& o) {
            std::vector<int> v;
            for (int b : o.reads()) if (b >= 0) v.push_back(b);
            for (int b : o.writes()) if (b >= 0) v.push_back(b);
            return v;
        };
        int max_level = 0;
        for (int i = lo; i < hi; ++i) {
            const Op& oi = ops[i];
            for (int j = lo; j < i; ++j) {
                const Op& oj = ops[j];
                bool dep = false;
                for (int b : touched(oi))
                    if ((writes(oj, b)) || (reads(oj, b) && writes(oi, b))) { dep = true; break; }
                if (dep) level[i - lo] = std::max(level[i - lo], level[j - lo] + 1);
            }
            max_level = std::max(max_level, level[i - lo]);
        }
        // A fuse sum nothing else in the region depends on (the HRNet fuse: its outputs are read after the join) moves to the
        // LAST level, where run_region_grouped issues all of a module's sums as one launch instead of 2-4 small ones.
        for (int i = lo; i < hi; ++i) {
            const Op& oi = ops[i];
            if (oi.kind != OP_FUSE || oi.debug_only) continue;
            bool sink = true;
            for (int j = i + 1; j < hi && sink; ++j) {
                const Op& oj = ops[j];
                for (int b : touched(oj))
                    if (writes(oi, b) || (reads(oi, b) && writes(oj, b))) { sink = false; break; }
            }
            if (sink) level[i - lo] = max_level;
        }
        region_levels[r].assign(max_level + 1, {});
        for (int i = lo; i < hi; ++i) {
            ops[i].level = level[i - lo];
            region_levels[r][level[i - lo]].push_back(i);
        }
    }
}

// The plan switches, in this precedence: cfg.plan_flags; what CAPF_PLAN_BF16_F32_STREAM implies; the diagnostic build's knobs; what the
// configuration's widths rule out
bool Engine::set_plan_switches() {
    PlanSwitches& p = plan;
    if (cfg.plan_flags & CAPF_PLAN_NO_FUSED_LIFTER) p.fused_lifter = false;
    if (cfg.plan_flags & CAPF_PLAN_NO_WINOGRAD) p.use_wino = false;
    if (cfg.plan_flags & CAPF_PLAN_NO_ROW_HALO) p.use_rh = false;
    if (cfg.plan_flags & CAPF_PLAN_WINOGRAD_F23_ONLY) p.wino_f43 = false;
    if (cfg.plan_flags & CAPF_PLAN_NO_PWCHAIN) p.use_pwchain = false;
    if (cfg.plan_flags & CAPF_PLAN_NO_UPADD) p.use_upadd = false;
    if (cfg.plan_flags & CAPF_PLAN_NO_BNECK) p.use_bneck = false;
    if (cfg.plan_flags & CAPF_PLAN_NO_BATCHED_REDUCE) p.batch_reduce = false;
    if (cfg.plan_flags & CAPF_PLAN_H2_PLANES) p.use_h2_planes = true;
    if (cfg.plan_flags & CAPF_PLAN_NO_WS) p.use_ws = false;
    if (cfg.plan_flags & CAPF_PLAN_NO_F32X3) p.use_x3 = false;
    if (cfg.plan_flags & CAPF_PLAN_F32X3_EXACT) p.x3_h2 = false;
    if (cfg.plan_flags & CAPF_PLAN_NO_F32H2_GEMM) p.use_h2g = false;
    if (cfg.plan_flags & CAPF_PLAN_BF16_F32_STREAM) {
        if (!b16()) { err = "CAPF_PLAN_BF16_F32_STREAM needs compute_dtype = CAPF_BF16 (not CAPF_F32; CAPF_F16 is refused at capf_create)"; return false; }
        if (cfg.backbone != CAPF_HRNET) { err = "CAPF_PLAN_BF16_F32_STREAM is an HRNet plan (CPN50 is not supported)"; return false; }
        if (cfg.plan_flags != CAPF_PLAN_BF16_F32_STREAM) { err = "CAPF_PLAN_BF16_F32_STREAM cannot be combined with other plan flags"; return false; }
        p.f32_stream = true;
        // layer1 runs as one launch per conv: the fused bottleneck kernels (bneck_bf16.hip) and the chained pointwise pair have no fp32-stream
        // epilogue (EXPERIMENTS R7.1 prices it)
        p.use_bneck = false;
        p.use_pwchain = false;
    }
    if (cfg.plan_flags & CAPF_PLAN_BN_BATCH_STATS) p.bn_batch = true;      // (capf_create has refused what the route does not cover)
    // tuning knobs of the diagnostic build only (diag_env is a constant nullptr in the product library)
    if (const char* fz = diag_env("CAPF_LIFTER_FUSED")) p.fused_lifter = atoi(fz) != 0;
    if (const char* wz = diag_env("CAPF_WINO")) p.use_wino = atoi(wz) != 0;
    if (const char* rz = diag_env("CAPF_BF16_RH")) p.use_rh = atoi(rz) != 0;
    if (const char* wb = diag_env("CAPF_WINO_MIN_BATCH")) p.wino_min_batch = atoi(wb);
    if (const char* wf = diag_env("CAPF_WINO_F43")) p.wino_f43 = atoi(wf) != 0;
    if (const char* wf = diag_env("CAPF_WINO_F43_MINHW")) p.wino_f43_min_hw = atoi(wf);
    if (const char* wf = diag_env("CAPF_WINO_F43_CPN")) p.wino_f43_cpn = atoi(wf) != 0;
    if (const char* wf = diag_env("CAPF_WINO_F43_MAXHW")) p.wino_f43_max_hw = atoi(wf);
    // the fused front half (lifter_fused.hip) holds a token row in 4 values per lane and a sampled row in 2 KiB of LDS: wider
    // configurations (embed_dim_ratio 272 / 288 / ..., > 512-channel context maps) take the one-kernel-per-op plan instead
    if (cfg.embed_dim_ratio > 256) p.fused_lifter = false;
    if (cfg.backbone == CAPF_HRNET && cfg.hr_channels[3] > 512) p.fused_lifter = false;
    return true;
}

// The batches [*lo, *hi] at which a halo tile takes a conv (false: none), from `takes` -- the tile's size rule and its launcher's own test
// (Engine::tile_takes) -- and `cap`, the batch at which the largest tensor the tile addresses with 31-bit byte offsets reaches 2 GB (exclusive).
// The accepted set is an interval: the size rules only fail downwards; the tiles' geometry (ws_plan) does not depend on the batch, and their
// 2 GB tests and ws_args_ok's only fail upwards.  So: the last accepted batch, just under the cap, then the first by bisection
template <class Takes>
static bool tile_batches(double cap, const Takes& takes, int* lo, int* hi) {
    int last = (int)std::min(1.0e6, cap);
    while (last >= 1 && last > (int)cap - 4 && !takes(last)) --last;   // (the limit itself is exclusive)
    if (last < 1 || !takes(last)) return false;
    int first = 1, top = last;
    while (first < top) {
        const int mid = first + (top - first) / 2;
        if (takes(mid)) top = mid; else first = mid + 1;
    }
    *lo = first; *hi = last;
    return true;
}

bool Engine::build() {
    if (cfg.height % 32 != 0 || cfg.width % 32 != 0) {
        err = "height and width must be multiples of 32";
        return false;
    }
    if (cfg.levels != 4 || cfg.deform_samples != 4 || cfg.deform_heads != 4 || cfg.embed_dim_ratio <= 0 ||
        cfg.embed_dim_ratio % (4 * cfg.deform_heads) != 0) {
        err = "unsupported lifter configuration (levels must be 4, 4x4 deformable sampling, embed_dim_ratio % 16 == 0)";
        return false;
    }
    if (cfg.num_heads < 1 || cfg.embed_dim_ratio % (4 * cfg.num_heads) != 0) {
        err = "num_heads must be at least 1 and divide embed_dim_ratio / 4 (the attention kernels read a head's embed_dim_ratio / num_heads "
              "values four at a time): got num_heads " + std::to_string(cfg.num_heads) + " at embed_dim_ratio " + std::to_string(cfg.embed_dim_ratio);
        return false;
    }
    // the attention launchers' own conditions (attention_ok, attention_bwd_ok: kernels.h) at the two shapes the lifter runs -- the res blocks
    // over the levels + 1 tokens of a joint, the joint blocks over the num_joints tokens of a frame -- refused here, not by a launcher in the
    // middle of a forward or of a backward.  Inference plans keep every head count: only the backward stages a head in LDS
    {
        const int res_d = cfg.embed_dim_ratio / cfg.num_heads, joint_d = (cfg.levels + 1) * res_d;
        if (cfg.num_joints < 1 || !attention_ok(cfg.num_joints, joint_d) || !attention_ok(cfg.levels + 1, res_d)) {
            err = "num_joints must be 1.." + std::to_string(ATTENTION_MAX_TOKENS) + " (the attention kernels hold at most " +
                  std::to_string(ATTENTION_MAX_TOKENS) + " tokens): got " + std::to_string(cfg.num_joints);
            return false;
        }
        if (cfg.training && (!attention_bwd_ok(cfg.num_joints, joint_d) || !attention_bwd_ok(cfg.levels + 1, res_d))) {
            const bool joint = !attention_bwd_ok(cfg.num_joints, joint_d);
            err = "num_heads " + std::to_string(cfg.num_heads) + " with training = 1: the attention backward stages a head of the " +
                  (joint ? "joint" : "res") + " blocks (" + std::to_string(joint ? cfg.num_joints : cfg.levels + 1) + " tokens, head dimension " +
                  std::to_string(joint ? joint_d : res_d) + ") in " +
                  std::to_string(joint ? attention_bwd_lds_bytes(cfg.num_joints, joint_d) : attention_bwd_lds_bytes(cfg.levels + 1, res_d)) +
                  " bytes of LDS, over the limit of " + std::to_string(ATTENTION_BWD_MAX_LDS) + ": use more heads, or an inference plan";
            return false;
        }
    }
    // the LayerNorm and head kernels (lifter.hip, train_kernels.hip) hold a joint row of (levels + 1) * embed_dim_ratio values in 24 values
    // per lane of one wave: 1536 at the most, i.e. embed_dim_ratio <= 288 -- refused here, not by a launcher in the middle of a forward
    if (cfg.embed_dim_ratio * (cfg.levels + 1) > 1536) {
        err = "embed_dim_ratio * (levels + 1) must not exceed 1536 (embed_dim_ratio <= 288 at 4 levels): the LayerNorm and head kernels hold a "
              "joint row in 24 values per lane of a 64-lane wave";
        return false;
    }
    // depth != levels: the variant without context blocks (ContextPose_mpi, pose_dformer.py:199).  Inference plans at any width up to that
    // limit; training plans at the widths that app builds (run_3dhp.py:219-232 and common/cfg.py:81-82: embed_dim_ratio 64 over base_dim 32,
    // 96 over 48), whose head dims (8 / 12 res, 40 / 60 joint) tests/test_gpu_mpi_train.py holds to fp64 at depths 1..8.  "Other widths train
    // at depth == levels": tests/test_gpu_train_widths.py holds a step of the H36M model to fp64 at 32, 64, 96, 160, 256 and 288
    if (cfg.depth != 0 && cfg.depth != cfg.levels) {
        const bool mpi_width = (cfg.base_dim == 32 && cfg.embed_dim_ratio == 64) || (cfg.base_dim == 48 && cfg.embed_dim_ratio == 96);
        if (cfg.depth < 1 || cfg.depth > 8 || cfg.context_blocks || (cfg.training && !mpi_width)) {
            err = cfg.context_blocks ? "depth != levels: 1..8 blocks per group, only for the variant without context blocks (ContextPose_mpi) and only for "
                                       "inference plans"
                  : (cfg.depth < 1 || cfg.depth > 8) ? "depth != levels: 1..8 blocks per group (the variant without context blocks, ContextPose_mpi)"
                  : "depth != levels with training = 1: only at the ContextPose_mpi widths (embed_dim_ratio 64 over base_dim 32, 96 over 48); "
                    "other widths train at depth == levels";
            return false;
        }
    }
    if (!set_plan_switches()) return false;
    Tensor img{EXT_IMAGES, cfg.height, cfg.width, 3};
    Tensor feats[4];
    if (cfg.backbone == CAPF_HRNET) {
        for (int i = 0; i < 4; ++i)
            if (cfg.hr_channels[i] <= 0 || cfg.hr_channels[i] % 4 != 0) {
                err = "HRNet branch widths must be positive multiples of 4";
                return false;
            }
        build_hrnet(img, feats);
        if (plan.f32_stream && !plan_f32_stream(feats)) return false;
    } else if (cfg.backbone == CAPF_CPN50) {
        build_cpn(img, feats);
    } else {
        err = "unknown backbone";
        return false;
    }
    for (int l = 0; l < 4; ++l) {
        name_tensor(*this, "feat" + std::to_string(l), feats[l].buf, {-1, feats[l].H, feats[l].W, feats[l].C}, maps_bf16() ? dt16() : 0);
        const int expect = cfg.backbone == CAPF_CPN50 ? cfg.base_dim : cfg.base_dim << l;
        if (feats[l].C != expect) {
            err = "poseformer.base_dim does not match the backbone's context-map widths";
            return false;
        }
    }
    for (const Op& op : ops)        // "stem": the output of the conv that reads the image.  NOT kept alive (name_tensor would pin 64 channels at half
        if (op.kind == OP_GEMM && op.in[0] == EXT_IMAGES) {       // resolution per frame in every workspace): later ops of a run reuse its memory, so what it
            NamedTensor t{};                                       // holds after a run is a function of the run alone -- two routes of one plan compare bit for bit
            stem_op = stem_op == -1 ? (int)(&op - ops.data()) : -2;
            t.buf = op.out;
            t.ndim = 4;
            t.shape[0] = -1; t.shape[1] = op.Ho; t.shape[2] = op.Wo; t.shape[3] = op.N;
            t.is_int = op.st_f32 ? 0 : (op.out_bf16 ? dt16() : 0);
            named["stem"] = t;
        }
    n_backbone_ops = (int)ops.size();
    for (int l = 0; l < 4; ++l) {
        feat_buf[l] = feats[l].buf; feat_H[l] = feats[l].H; feat_W[l] = feats[l].W; feat_C[l] = feats[l].C;
    }
    build_lifter(feats);
    // flat gradient layout: the volume_net.* parameters in schema (= registration) order
    grad_off.assign(params.size(), -1);
    grad_elems = 0;
    for (size_t i = 0; i < params.size(); ++i)
        if (params[i].name.rfind("volume_net.", 0) == 0) {
            grad_off[i] = grad_elems;
            grad_elems += params[i].numel();
        }
    assign_offsets();
    schedule_regions();
    // the GEMM kernels address a whole activation tensor (and a conv's input window) with 32-bit offsets
    // (launch_gemm_f32: M * ld < 4e9 elements of out / res, < 4e9 bytes of a rows-mode operand)
    {
        double worst = 1.0;          // largest per-frame tensor, in elements
        for (const Op& op : ops)
            if (op.kind == OP_GEMM) {
                worst = std::max(worst, (double)op.rows_per_frame * (double)std::max(op.omap.S1, (long)op.N));
                if (op.conv) worst = std::max(worst, (double)op.H * op.W * op.Cin);
                else worst = std::max(worst, (double)op.rows_per_frame * (double)std::max(op.amap.S1, (long)op.K) * 4.0 / (op.amap.G > 0 ? op.amap.G : 1));
            }
        batch_limit = (int)std::min(2.0e9, 3.9e9 / worst);
    }
    // the layer1 bottleneck pairs (conv3 -> next block's conv1) the pointwise-chain kernel takes: structural half of gemm_f32_pwchain_ok
    for (size_t i = 0; i + 1 < ops.size(); ++i) {
        Op& a = ops[i];
        Op& b = ops[i + 1];
        if (a.kind != OP_GEMM || b.kind != OP_GEMM || !a.conv || !b.conv || a.bf16 || b.bf16) continue;
        if (a.ks != 1 || b.ks != 1 || a.stride != 1 || b.stride != 1 || a.Cin != 64 || a.N != 256 || b.Cin != 256 || b.N != 64) continue;
        if (b.in[0] != a.out || b.region != a.region || b.lane != a.lane || a.aux < 0 || b.aux >= 0) continue;
        a.pw_pair = b.pw_pair = 1;
    }
    // at which batches a 3x3 stride-1 conv runs its plan's halo tile (Engine::gemm_family): the split-fp32 tile for a fast3x3 conv, the 2-D
    // halo tile for a 16-bit one
    for (Op& op : ops) {
        if (op.kind != OP_GEMM || !(op.bf16 == 1 ? packs[op.pack].ws : op.fast3x3 && packs[op.pack].x3)) continue;
        // bytes per pixel of the largest tensor the tile addresses with 31-bit offsets: the 2-D halo tile whole tensors of 16-bit rows (the
        // fp32-stream epilogue's output and residual rows count 4 bytes an element), the three-piece tile whole fp32 tensors; the two-piece
        // tile only counts pixels
        const double eb = op.f32s ? 4.0 : 2.0;
        const double row = op.bf16 ? std::max({2.0 * op.Cin, 2.0 * op.N, eb * op.omap.S1, op.aux >= 0 || op.res_param >= 0 ? eb * op.rmap.S1 : 0.0})
                           : plan.x3_h2 ? 1.0 : 4.0 * std::max(op.Cin, op.N);
        if (!tile_batches(2.0e9 / ((double)op.H * op.W * row), [&](int batch) { return tile_takes(op, batch); }, &op.tile_lo, &op.tile_hi)) continue;
        // the Winograd layout of this conv is dead weight when the tile covers every batch the Winograd kernels could be asked for
        if (op.fast3x3 && op.tile_lo <= plan.wino_min_batch && op.tile_hi >= cfg.max_batch) packs[op.pack].wino_skip = true;
    }
    // unit tables of the two-fp16-piece conv tile: one per map geometry among the convs it can take (igemm_f32h2_ws_tile.h, UNIT TABLE)
    utab_host.clear();
    if (plan.x3_h2 && plan.use_x3) {
        std::map<std::tuple<int, int, int>, long> seen;
        for (Op& op : ops) {
            if (op.kind != OP_GEMM || !op.fast3x3 || !packs[op.pack].x3 || op.tile_hi < op.tile_lo) continue;
            const auto key = std::make_tuple(op.H, op.W, op.Cin);
            auto it = seen.find(key);
            if (it == seen.end()) {
                std::vector<unsigned> t(F32H2_UNIT_TABLE_WORDS);
                long at = -1;
                if (f32h2_unit_table(op.H, op.W, op.Cin, t.data())) {
                    at = (long)utab_host.size();
                    utab_host.insert(utab_host.end(), t.begin(), t.end());
                }
                it = seen.emplace(key, at).first;
            }
            op.h2_utab = it->second;
        }
    }
    // pack arena layout
    size_t off = 0;
    for (Pack& pk : packs) {
        if (pk.in_place) continue;
        pk.w_off = off;
        off += pk.wino_skip ? 64 : round64(pk.bf16 ? ((size_t)pk.N * pk.Kpad + 1) / 2 : (size_t)pk.N * pk.Kpad);
        if (pk.fast3x3) {
            pk.direct_off = off;
            off += round64((size_t)pk.N * pk.direct_Kpad);
        }
        if (pk.rh) {
            pk.rh_off = off;
            off += round64(((size_t)pk.N * pk.rh_Kpad + 1) / 2);
        }
        if (pk.ws) {
            pk.ws_off = off;
            off += round64(((size_t)bf16_ws_pack_elems(pk.N, pk.Cin) + 1) / 2);
        }
        if (pk.x3) {
            pk.x3_off = off;
            off += round64(((size_t)(plan.x3_h2 ? f32h2_pack_elems(pk.N, pk.Cin) : f32x3_pack_elems(pk.N, pk.Cin)) + 1) / 2);
        }
        pk.b_off = off;
        off += round64((size_t)pk.N);
    }
    for (Pack& pk : packs)                  // (direct linears included: the h2 copy is a pack of its own)
        if (pk.h2g) {
            pk.h2g_off = off;
            off += round64((size_t)f32h2_gemm_pack_elems(pk.N, pk.h2g_Kpad));
            if (pk.chain) {
                pk.chain_off = off;
                off += round64((size_t)f32h2_gemm_pack_elems(pk.N, pk.h2g_Kpad));
            }
        }
    {   // room for the bias-copy table: one CopySegment per linear of every packed (non-direct) linear pack
        size_t nseg = 0;
        for (const Pack& pk : packs)
            if (pk.kind == LINEAR && !pk.in_place) nseg += (size_t)pk.n_lin;
        bias_tab_off = off;
        off += round64(nseg * (sizeof(CopySegment) / sizeof(float)));
    }
    t_h2_plan();                            // the training step's weight table (train.cpp); its device image lives in the arena
    t_h2_tab_off = off;
    off += round64(t_h2_specs.size() * (sizeof(H2TrainW) / sizeof(float)) + 16);
    utab_off = off;
    off += round64(utab_host.size() + 16);
    // CAPF_PLAN_BN_BATCH_STATS: the backbone's second op list -- one unit per conv of the plan -- and the unfolded packs its raw convs read, in
    // every layout the plan keeps for that conv (the route per geometry and batch stays the plan's), behind everything the plan itself packs
    if (plan.bn_batch) {
        bn_unit_of.assign(ops.size(), -1);
        raw_packs = packs;
        for (int i = 0; i < n_backbone_ops; ++i) {
            const Op& op = ops[i];
            if (op.kind == OP_FORK || op.kind == OP_JOIN || op.kind == OP_FUSE) continue;
            if (op.kind != OP_GEMM || !op.conv || op.bf16 || op.up_in >= 0 || packs[op.pack].kind != CONV_BN || packs[op.pack].in_place) {
                err = "CAPF_PLAN_BN_BATCH_STATS: unexpected backbone op " + op.name;
                return false;
            }
            bn_unit_of[i] = (int)bn_units.size();
            bn_units.push_back(BnUnit{i, packs[op.pack].bn});
            Pack& pk = raw_packs[op.pack];
            pk.raw = true;
            pk.w_off = off;
            off += pk.wino_skip ? 64 : round64((size_t)pk.N * pk.Kpad);
            if (pk.fast3x3) {
                pk.direct_off = off;
                off += round64((size_t)pk.N * pk.direct_Kpad);
            }
            if (pk.x3) {
                pk.x3_off = off;
                off += round64(((size_t)(plan.x3_h2 ? f32h2_pack_elems(pk.N, pk.Cin) : f32x3_pack_elems(pk.N, pk.Cin)) + 1) / 2);
            }
            pk.b_off = off;
            off += round64((size_t)pk.N);
            if (pk.h2g) {
                pk.h2g_off = off;
                off += round64((size_t)f32h2_gemm_pack_elems(pk.N, pk.h2g_Kpad));
            }
        }
    }
    pack_elems = off;
    return true;
}

}  // namespace capf
