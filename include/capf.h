/*
 * capf.h — C ABI of the MI355X-native Context-Aware PoseFormer hot path.
 *
 * The reference (QitaoZhao/ContextAware-PoseFormer) is pure Python/PyTorch: it has no FFI, plugin or
 * operator registry.  Its hot path sits behind one nn.Module call,
 *
 *     CA_PF.forward(images[B,H,W,3], keypoints_2d[B,17,2], keypoints_2d_crop[B,17,2]) -> [B,1,17,3]
 *                                                   ContextPose/mvn/models/conpose.py:30-42
 *
 * so the "binding a maintainer would add" is a ctypes stub inside that forward.
 * Every entry point below names the reference code it replaces.  Conventions:
 *   - plain C types only; device memory is caller-owned (the PyTorch host module keeps owning
 *     parameters, so optimizers / DDP / checkpoints keep working); the library borrows pointers.
 *   - every call returns 0 on success or a negative capf_status; capf_last_error() has the text.
 *   - stream-ordered, no hidden synchronisation, no allocation inside capf_forward.
 *   - a handle is not thread-safe; one handle per (process, device).
 */
#ifndef CAPF_H
#define CAPF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* libcapf.so is built with -fvisibility=hidden: the functions declared in this header are its whole dynamic symbol table */
#pragma GCC visibility push(default)

typedef struct capf_handle capf_handle;

enum capf_status {
    CAPF_OK = 0,
    CAPF_ERR_INVALID = -1,     /* bad argument / unknown name / shape mismatch */
    CAPF_ERR_UNSUPPORTED = -2, /* configuration the kernels do not cover */
    CAPF_ERR_HIP = -3,         /* a HIP runtime call or kernel launch failed */
    CAPF_ERR_STATE = -4        /* call order: params / workspace not set */
};

enum capf_backbone { CAPF_HRNET = 0, CAPF_CPN50 = 1 };
/* CAPF_F16 (HRNet inference plans): the CAPF_BF16 plan -- the same ops, kernels, routing thresholds and plan flags -- with IEEE fp16 in
 * place of bf16 as the 16-bit element of every activation, weight pack and matrix-pipe operand (11 significand bits instead of 8; see
 * "fp16 storage" at capf_op_conv_16).  capf_create refuses it for CAPF_CPN50, with CAPF_PLAN_BF16_F32_STREAM and with training = 1. */
enum capf_dtype { CAPF_F32 = 0, CAPF_BF16 = 1, CAPF_F16 = 2 };

/* parameter kinds reported by capf_param_info (lets the host build matching leaf modules) */
enum capf_param_kind {
    CAPF_P_CONV_W = 0,   /* nn.Conv2d.weight  [Cout,Cin,kh,kw]  (bias=False everywhere) */
    CAPF_P_BN_W = 1, CAPF_P_BN_B = 2, CAPF_P_BN_MEAN = 3, CAPF_P_BN_VAR = 4, CAPF_P_BN_NBT = 5,
    CAPF_P_LIN_W = 6, CAPF_P_LIN_B = 7,     /* nn.Linear [out,in], [out] */
    CAPF_P_LN_W = 8, CAPF_P_LN_B = 9,       /* nn.LayerNorm */
    CAPF_P_RAW = 10                         /* bare nn.Parameter (Spatial_pos_embed) */
};

/*
 * Model description == the subset of the reference's global config that CA_PF.__init__ reads:
 *   config.model.backbone.{type,STAGE2..4.NUM_CHANNELS,NUM_MODULES,NUM_BLOCKS}  (conpose.py:14-20,
 *       pose_hrnet.py:330-370, mvn/utils/cfg.py:24-66)
 *   config.model.poseformer.{base_dim,embed_dim_ratio,levels}                    (pose_dformer.py:167-172)
 */
typedef struct capf_config {
    int32_t backbone;          /* capf_backbone */
    int32_t hr_channels[4];    /* HRNet branch widths: {32,64,128,256} (W32) / {48,96,192,384} (W48) */
    int32_t hr_modules[3];     /* NUM_MODULES of stage2..4: {1,4,3} */
    int32_t hr_blocks;         /* NUM_BLOCKS per branch: 4 */
    int32_t base_dim;          /* poseformer.base_dim: 32 / 48 / 256(cpn) */
    int32_t embed_dim_ratio;   /* 128.  A multiple of 32 with embed_dim_ratio * (levels + 1) <= 1536, i.e. at most 288: the LayerNorm and head
                                  kernels hold a joint row in 24 values per lane of a 64-lane wave; capf_create refuses a wider one */
    int32_t levels;            /* 4 feature levels (H36M model: also the depth of every block group, pose_dformer.py:169) */
    int32_t num_joints;        /* 17.  1..17: the attention kernels hold at most 17 tokens; capf_create refuses more */
    int32_t num_heads;         /* 8  (Block).  Any count that divides embed_dim_ratio / 4.  With training = 1 the attention backward stages a head
                                  (q, k, v, dO) in LDS: capf_create refuses a count whose joint-block head dimension, (levels + 1) * embed_dim_ratio /
                                  num_heads, needs more than 64 KiB there (above 230 at 6..17 joints, above 815 at 1..5); inference plans keep it */
    int32_t deform_heads;      /* 4  (DeformableBlock, pose_dformer.py:202) */
    int32_t deform_samples;    /* 4 */
    int32_t context_blocks;    /* 1 = H36M model; 0 = MPI-INF-3DHP variant without DeformableBlocks */
    int32_t compute_dtype;     /* capf_dtype: MFMA operand type of the backbone convs / lifter GEMMs (CAPF_BF16 / CAPF_F16: also their activations' storage) */
    int32_t max_batch;         /* workspace is sized for this many frames */
    int32_t height, width;     /* input image size (256x256, 256x192, 384x288, ...) */
    int32_t training;          /* 1: size the workspace for capf_forward_train / capf_backward as well */
    int32_t plan_flags;        /* 0 = the product plan.  capf_plan_flag bits take one kernel family out of the plan (parity
                                  tests compare the two routes; nothing else -- no environment variable -- changes a plan) */
    int32_t depth;             /* blocks per group (res_blocks / joint_blocks).  0 = levels.  The MPI-INF-3DHP variant reads it from
                                  config.model.poseformer.depth (ContextPose_mpi/model/pose_dformer.py:199, 217-227; 1..8).  Inference plans
                                  at any accepted width; training plans at that app's widths (run_3dhp.py:219-232: embed_dim_ratio 64 over base_dim
                                  32, 96 over 48), other widths train at depth == levels.  The H36M model (context_blocks = 1) has
                                  depth == levels by construction */
} capf_config;

enum capf_plan_flag {
    CAPF_PLAN_NO_FUSED_LIFTER = 1,  /* one kernel per lifter op instead of embed_kernel / ctx_attn_kernel / LayerNorm-in-GEMM */
    CAPF_PLAN_NO_WINOGRAD = 2,      /* fp32 3x3 stride-1 convs on the direct MFMA kernel */
    CAPF_PLAN_NO_ROW_HALO = 4,      /* bf16 3x3 stride-1 convs on the direct bf16 kernel */
    CAPF_PLAN_WINOGRAD_F23_ONLY = 8, /* F(2,3) where F(4,3) would be chosen */
    CAPF_PLAN_NO_PWCHAIN = 16,      /* layer1's conv3 -> next conv1 pairs as two pointwise launches instead of one chained kernel */
    CAPF_PLAN_NO_WS = 32,           /* bf16 3x3 stride-1 convs without the 2-D halo tile (row-halo / direct kernels as in round 3) */
    CAPF_PLAN_LIFTER_FP32 = 64,     /* compute_dtype = CAPF_BF16: keep the lifter's qkv / proj / fc1 / fc2 on the fp32 kernels (bf16 backbone only);
                                     * the accuracy / speed trade bench.py reports as `vs_fp32_oracle`                                    */
    CAPF_PLAN_NO_F32X3 = 128,       /* fp32 3x3 stride-1 convs without either split-fp32 tile (igemm_f32h2_ws.hip / igemm_f32x3_ws.hip):
                                     * the Winograd kernels on the fp32 matrix pipe (from batch 24; the direct kernel below)              */
    CAPF_PLAN_NO_F32H2_GEMM = 512,  /* every OTHER fp32 conv / linear (1x1, stride 2, lone convs, the lifter's projections -- forward, input and weight
                                     * gradients of a training step included) on the fp32 matrix pipe at every batch (igemm_f32.hip) instead of the
                                     * two-fp16-piece GEMM from batch 5 (igemm_f32h2.hip)                                                        */
    CAPF_PLAN_NO_UPADD = 1024,      /* compute_dtype = CAPF_BF16, CPN: globalNet's `lateral + upsampled path` (globalNet.py:66) as a resize-add launch behind the
                                     * lateral conv (round 5's plan) instead of inside the conv's epilogue (igemm_bf16_kernel<.., UPADD>)        */
    CAPF_PLAN_H2_PLANES = 2048,     /* OPT-IN (measured slower, EXPERIMENTS R6.5): a BasicBlock's conv1 output travels to conv2 as split fp16 planes
                                     * (capf_op_conv_f32h2_planes) where both convs run the two-fp16-piece tile; default: plain fp32 tensors          */
    CAPF_PLAN_NO_BNECK = 4096,      /* compute_dtype = CAPF_BF16: the first bottleneck of layer1 (conv1 / conv2 / downsample / conv3; networks/resnet.py:58-93,
                                     * pose_hrnet.py:98-136) as its five launches instead of ONE kernel with t1 / t2 / the shortcut on chip (bneck_bf16.hip) */
    CAPF_PLAN_NO_BATCHED_REDUCE = 8192, /* training: every weight gradient's slab sum and every bias / LayerNorm gradient's second reduction stage as its
                                     * own launch behind its producer (96 launches per step) instead of a handful of batched ones when the scratch
                                     * fills and at the end of capf_backward (csrc/train.cpp t_slab_flush / t_col_flush).  Same summation order per
                                     * element either way: bit-identical gradients (tests/test_gpu_train.py); an A/B aid                        */
    /* (1 << 14 is unassigned and rejected: tests/test_abi.py pins that an unknown bit is refused) */
    CAPF_PLAN_BF16_F32_STREAM = 32768, /* OPT-IN, compute_dtype = CAPF_BF16, HRNet (W32 / W48) only: bf16 only as conv operands, every other backbone tensor fp32
                                     * (capf_oracle BF16_STREAM_FP32).  Weights fold and round as in the default bf16 plan; every activation a conv reads is
                                     * rounded to bf16 once (RNE); residual adds, ReLU, fuse sums, nearest upsampling and the four context maps stay fp32,
                                     * the lifter keeps the default bf16 placement and its samplers read the fp32 maps.  Storage is decided per tensor from
                                     * its readers: conv operands only -> bf16; any residual / fuse-sum / lifter reader -> fp32, plus a bf16 "shadow" written
                                     * by the same epilogue when convs read it too (capf_op_tensor slot 6; convs take the shadow, every residual is fp32).
                                     * layer1 runs one launch per conv (no bneck_bf16.hip / pointwise chain).  capf_create refuses it with CAPF_F32, with
                                     * CAPF_CPN50 and together with any other plan flag (CAPF_ERR_UNSUPPORTED).                                        */
    CAPF_PLAN_BN_BATCH_STATS = 65536, /* OPT-IN, CAPF_HRNET + CAPF_F32 + training = 1 only (anything else: CAPF_ERR_UNSUPPORTED): the handle also carries the
                                     * BATCH-STATISTICS route of the backbone, capf_backbone_forward_bn -- what a frozen backbone computes when it is
                                     * left in train mode (ContextPose_mpi/run_3dhp.py:31-35 never calls backbone.eval()).  The plan itself -- ops,
                                     * capf_num_ops, capf_op_info, the accounting entries, every other entry's bits -- is the flagless handle's and
                                     * describes the running-statistics route; capf_workspace_bytes grows by the statistics scratch and the pack arena
                                     * by an unfolded copy of every conv pack.  Cannot be combined with CAPF_PLAN_BF16_F32_STREAM.                  */
    CAPF_PLAN_CPN_PREDICT = 131072, /* OPT-IN, CAPF_CPN50 with CAPF_F32 or CAPF_BF16 (CAPF_HRNET: CAPF_ERR_UNSUPPORTED): the backbone also runs the detector head a
                                     * CPN checkpoint was trained with, backbone.refine_net.final_predict (refineNet.py:64-70, :86-88), behind the four cascades:
                                     * a channel concatenation of feat0..3 into a [B, 64, 48, 1024] buffer of its own (torch.cat(refine_fms, 1); feat0..3 are
                                     * neither moved nor aliased), the Bottleneck's four conv + BatchNorm ops (final_predict.0.conv1 / conv2 / downsample.0 /
                                     * conv3, the shortcut on a second lane) and final_predict.1 / .2, conv3x3(256 -> 17) + BatchNorm without activation, whose
                                     * pack carries 20 rows (17..19: zero weights, zero folded bias) because no conv kernel takes N % 4 != 0.  Result: the
                                     * named tensor "heat" [B, 64, 48, 20] in the plan's activation dtype, channels 17..19 exact zeros, alive to the end of the
                                     * run like feat0..3 -- the input of capf_cpn_decode.  These are backbone ops: capf_backbone_forward(_u8) and capf_forward*
                                     * run them.  The schema (names, order, shapes) is the unflagged plan's; the unflagged plan itself is unchanged and keeps
                                     * the head as parameters only.  capf_workspace_bytes grows by the concatenation, the head's intermediates and heat.   */
    CAPF_PLAN_F32X3_EXACT = 256    /* ... on round 4's tile instead of the default one: every operand split EXACTLY into three bf16 pieces,
                                     * six piece products per fp32 MAC (igemm_f32x3_ws.hip).  The default (ABI 5) carries an operand as two
                                     * block-scaled fp16 pieces (to 2^-23) and issues three products: half the MFMAs, the same measured
                                     * distance to an fp64 evaluation (see capf_op_conv_f32h2_group)                                      */
};

/* ---- lifetime -------------------------------------------------------------------------------
 * Replaces CA_PF.__init__ (conpose.py:10-27): builds the layer plan (pose_hrnet.py:312-462 /
 * networks/network.py:9-28 / pose_dformer.py:144-208) and the parameter schema.
 * device < 0: "plan only" — no HIP call is made; schema / workspace queries work (CPU tests).   */
int capf_create(const capf_config* cfg, int device, capf_handle** out);
void capf_destroy(capf_handle* h);
/* Largest batch one call accepts: min(cfg.max_batch, what the kernels' 32-bit tensor addressing allows at this input
 * size — about 3800 frames for HRNet at 256x256).  Larger batches return CAPF_ERR_UNSUPPORTED with a clear message. */
int capf_max_batch(const capf_handle* h);
const char* capf_last_error(const capf_handle* h);  /* h may be NULL: last create error */
const char* capf_version(void);
/* ABI revision of THIS header.  A caller compiled against capf.h checks capf_abi_version() == CAPF_ABI_VERSION before it passes structs
 * (capf_config, capf_conv_desc, capf_op_desc) across the boundary: revision 5 = round 5 (capf_op_desc as declared below -- 240 bytes since
 * revision 4, 104 before --, plan flags up to CAPF_PLAN_F32X3_EXACT, the capf_op_*_f32h2 entry points, capf_op_describe_sized).  The
 * version string carries the same number ("capf 0.5 (gfx950)").  Revision 7 (additive): CAPF_PLAN_BF16_F32_STREAM and capf_op_tensor slot 6
 * (an op's bf16 shadow output); struct layouts unchanged.  Revision 8 (additive): the batched JPEG decode (capf_jpeg_batch_info,
 * capf_jpeg_decode_batch, capf_jpeg_coefficients_subseq); struct layouts unchanged.  Revision 9 (additive): training plans of the variant
 * without context blocks at any depth 1..8 (its two widths) (its DropPath layout at capf_forward_train), capf_fliptest_fuse_swap, capf_pck_counts; struct
 * layouts unchanged.  Revision 10 (additive): the crop-aware JPEG route (capf_jpeg_crop_rect, capf_jpeg_crop_batch_info,
 * capf_jpeg_decode_crop_batch); struct layouts unchanged.  Revision 11 (additive): the guarded AdamW step (capf_optim_ctrl_bytes,
 * capf_optim_ctrl_init, capf_grad_sumsq, capf_adamw_step_guarded; new structs capf_optim_report, capf_optim_segment); existing struct
 * layouts unchanged.  Revision 12 (additive): compute_dtype = CAPF_F16, tensor dtype code 3 (fp16) in capf_tensor / capf_op_desc, the
 * capf_op_*_16 entry points (the 16-bit kernels for either element format) and capf_debug_f16_round; struct layouts unchanged
 * (additive: capf_set_map_grad_mode, capf_map_grad_mode; CAPF_PLAN_BN_BATCH_STATS, capf_backbone_forward_bn, capf_op_bn_stats_scratch_bytes,
 * capf_op_bn_stats, capf_op_bn_apply; capf_backward_points; capf_kp_head_scratch_bytes, capf_kp_head_forward, capf_kp_head_backward;
 * capf_kp_head_pair_scratch_bytes, capf_kp_head_forward_pair; CAPF_PLAN_CPN_PREDICT, the named tensor "heat", capf_cpn_decode,
 * capf_cpn_decode_taps, capf_cpn_decode_lds_bytes; capf_cpn_decode_pair; capf_kp_heatmap_loss_scratch_bytes, capf_kp_heatmap_loss;
 * capf_pck2d_counts; capf_erase_scratch_bytes, capf_erase_patches).                                                                         */
#define CAPF_ABI_VERSION 12
int capf_abi_version(void);

/* ---- parameter schema == the reference's state_dict ------------- */
int capf_num_params(const capf_handle* h);
int capf_param_info(const capf_handle* h, int index, const char** name, int64_t shape[4],
                    int* ndim, int* kind);

/* Borrow a device pointer for one state_dict entry (fp32; BN num_batches_tracked is ignored).
 * On a handle with CAPF_PLAN_BN_BATCH_STATS the backbone's running_mean / running_var buffers must be WRITABLE: capf_backbone_forward_bn
 * updates them in place through these pointers.
 * Replaces nn.Module parameter lookup during forward.  The pointer must stay valid until the
 * next capf_set_param for that name or capf_destroy. */
int capf_set_param(capf_handle* h, const char* name, const void* dev_ptr, const int64_t* shape,
                   int ndim);

/* Re-derive the private packed copies (BN folded into conv weights+bias, weights re-laid out
 * K-major for the MFMA kernels, bf16 copies).  Call after load_state_dict / optimizer.step().
 * Stream-ordered on `stream` (hipStream_t passed as void*). */
int capf_params_changed(capf_handle* h, void* stream);

/* Same, restricted to the private copies derived from volume_net.* parameters (the frozen backbone's
 * folded conv weights are left alone): what a training step needs after its optimizer update. */
int capf_lifter_params_changed(capf_handle* h, void* stream);

/* ---- workspace (activations); caller-owned so the host allocator (torch) stays in charge ----- */
size_t capf_workspace_bytes(const capf_handle* h, int batch);
int capf_set_workspace(capf_handle* h, void* dev_ptr, size_t bytes);

/* ---- the hot path ----------------------------------------------------------------------------
 * Replaces CA_PF.forward (conpose.py:30-42) = NHWC->NCHW permute (:32, folded into the stem conv's
 * loads), in-place crop-keypoint normalisation (:34-35, done in place on kcrop_inout exactly like
 * the reference), backbone forward (:38, pose_hrnet.py:464-501 / networks/network.py:16-22) and
 * PoseTransformer.forward (:40, pose_dformer.py:210-241).
 *   images_nhwc [B,H,W,3] fp32, k2d [B,17,2] fp32, kcrop_inout [B,17,2] fp32 (MUTATED),
 *   out [B,1,17,3] fp32.  All device pointers.  Enqueued on `stream`; returns immediately.      */
int capf_forward(capf_handle* h, void* stream, const float* images_nhwc, const float* k2d,
                 float* kcrop_inout, int batch, float* out);

/* Backbone only: writes nothing to `out`; the four context maps stay in the workspace (NHWC) and
 * can be read through capf_tensor("feat0".."feat3").  Replaces self.backbone(images) conpose.py:38. */
int capf_backbone_forward(capf_handle* h, void* stream, const float* images_nhwc, int batch);

/* capf_backbone_forward with BATCH statistics in every BatchNorm2d: replaces self.backbone(images) while the backbone is in train mode
 * (nn.BatchNorm2d.forward with self.training: F.batch_norm(..., training=True, momentum, eps = 1e-5)), for a handle created with
 * CAPF_PLAN_BN_BATCH_STATS (any other handle: CAPF_ERR_STATE).  It leaves feat0..3 in the workspace, valid for `batch`, exactly as
 * capf_backbone_forward does: capf_lifter_forward / capf_lifter_forward_train / capf_backward / capf_backward_maps run on them unchanged,
 * and like every backbone run it invalidates a saved training step.  Batch range, workspace, unpacked parameters and plan-only handles are
 * refused as by the other run entries.  Gradients do not reach the backbone (it stays frozen).
 * Per BatchNorm, with n = batch * H * W values per channel of the raw conv output x:
 *     mean, var (biased) over the batch;   y = (x - mean) / sqrt(var + 1e-5) * gamma + beta  (+ residual) (ReLU);
 *     running_mean <- (1 - momentum) * running_mean + momentum * mean;
 *     running_var  <- (1 - momentum) * running_var  + momentum * var * n / (n - 1).
 * THE RUNNING STATISTICS ARE WRITTEN IN PLACE through the pointers capf_set_param borrowed: on such a handle the running_mean / running_var
 * buffers must be writable device memory.  num_batches_tracked stays ignored; the host counts it.  The folded packs of the plan are NOT
 * refreshed: the next running-statistics run (capf_forward, capf_backbone_forward, ...) sees the moved statistics only after
 * capf_params_changed.  If a BatchNorm has n < 2 at this batch and input size (batch 1 at a 32x32 input: the deepest map is 1x1) the call
 * returns CAPF_ERR_INVALID -- torch's "Expected more than 1 value per channel when training" -- and nothing is launched or written.
 * Every unit conv -> BatchNorm (-> + residual) (-> ReLU) runs as the raw convolution (unfolded weights, on the kernel family and in the
 * grouped launch per dependency level that the plan routes its geometry and batch to), the statistics (two launches, no atomics, one fixed
 * summation order: the same inputs give the same bits on every run, handle and capf_set_lanes mode) and one normalise pass in place; the
 * launches that cross a BatchNorm (chained pointwise pairs, CAPF_PLAN_H2_PLANES) are not used.  Everything is enqueued on `stream` alone.
 * Measured (EXPERIMENTS R22.1, HRNet-32, 256x256): the backbone takes 24.6 against 14.7 ms at batch 160 and 11.2 against 5.7 ms at batch 64
 * (491 / 427 launches against 170 / 184; 106 launches each of the two statistics stages and of the apply pass), a training step 1.58x / 1.62x. */
int capf_backbone_forward_bn(capf_handle* h, void* stream, const float* images_nhwc, int batch, float momentum);

/* ---- training step of the lifter (the backbone is frozen, conpose.py:22-25) --
 * capf_forward_train: capf_forward that keeps the lifter's intermediates for capf_backward.
 *     Replaces model(images, k2d, kcrop) under model.train() (train.py:183; run_3dhp.py:79 for the variant without context blocks).
 *     drop_masks: the DropPath multipliers (0 or 1/keep_prob; timm DropPath, pose_dformer.py:71,101) laid out as
 *       context_blocks = 1: ctx[i]{m1[B],m2[B]} | res[i]{m1[B*17],m2[B*17]} | joint[i]{m1[B],m2[B]}, i = 0..levels-1;
 *       context_blocks = 0: res[i]{m1[B*17],m2[B*17]} | joint[i]{m1[B],m2[B]}, i = 0..depth-1 (no context segment; ContextPose_mpi
 *                           pose_dformer.py:215: res block i and joint block i share rate i of linspace(0, drop_path_rate, depth));
 *     NULL = no drop.
 * capf_backward: replaces loss.backward() through the lifter (train.py:195): grad_out [B,1,17,3] ->
 *     flat_grad, one fp32 buffer holding the gradient of every volume_net.* parameter in schema order
 *     (capf_grad_info), each written exactly once (no atomics) — so ONE all-reduce covers DDP's traffic.
 * capf_mpjpe: MPJPE.forward (loss.py:16-22) + its gradient w.r.t. pred (scaled by grad_scale).
 * capf_adamw_step: torch.optim.AdamW update (train.py:345) of one flat parameter buffer.            */
int capf_forward_train(capf_handle* h, void* stream, const float* images_nhwc, const float* k2d,
                       float* kcrop_inout, int batch, float* out, const float* drop_masks);
int capf_backward(capf_handle* h, void* stream, const float* grad_out, int batch, float* flat_grad,
                  const float* drop_masks);
/* Saved activations live in the workspace: ANY later capf_forward* / capf_backbone_forward / capf_lifter_forward /
 * capf_set_workspace invalidates them, and capf_backward then returns CAPF_ERR_STATE instead of differentiating the
 * wrong step.  capf_train_generation changes with every such run: a host autograd node records it after its
 * capf_forward_train and compares before capf_backward (two forwards followed by one combined backward).
 * The PARAMETERS must not change between a capf_forward_train and its capf_backward either (an optimizer step belongs after the
 * backward, as in train.py:195-201): the backward multiplies by the packs of W^T that the forward built from the parameters it saw. */
int64_t capf_train_generation(const capf_handle* h);
int64_t capf_grad_elems(const capf_handle* h);
int capf_grad_info(const capf_handle* h, int param_index, int64_t* offset);   /* -1: not a lifter parameter */
/* How many of the lifter's nn.Linear matrices a training step at batch >= 5 multiplies by on the two-fp16-piece GEMM (forward y = x W^T
 * and / or backward dX = dY W; packs of W and W^T are rebuilt from the current parameters at the start of every capf_forward_train).
 * 0: every product of the step runs on the fp32 matrix pipe (CAPF_PLAN_NO_F32H2_GEMM, compute_dtype = bf16, training = 0). */
int capf_train_h2_matrices(const capf_handle* h);
int capf_mpjpe(void* stream, const float* pred, const float* gt, int rows, float* loss, float* dpred,
               float grad_scale);
/* the same loss for rows of any width `dim` (MPJPE.forward accepts [..., D]: 2-D keypoints as well, loss.py:16-22) */
int capf_mpjpe_nd(void* stream, const float* pred, const float* gt, int rows, int dim, float* loss, float* dpred,
                  float grad_scale);
/* grad_scale multiplies every gradient element on the way in: 1 / world_size turns the SUM all-reduce of the flat
 * gradient into DDP's average (train.py:361-362) without a separate pass over the 56 MB buffer; 1.0f is exact. */
int capf_adamw_step(void* stream, float* params, const float* grads, float* exp_avg, float* exp_avg_sq,
                    int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                    float grad_scale);

/* ---- guarded AdamW step: global-norm clipping, non-finite skip, lr groups, device-side step count ---------------------------------
 * Replaces the optimizer end of one_epoch_full (train.py:187-206) on the flat gradient of capf_backward, after the all-reduce:
 *     if not torch.isnan(loss):                                   train.py:194
 *         clip_grad_norm_(params, grad_clip / volume_net_lr)      train.py:196-200
 *         optimizer.step()                                        train.py:201, AdamW with per-group lr: run_3dhp.py:260-277
 *     epoch_loss_3d += rows * loss.item(); N += rows              train.py:191-192
 * without a host read: two launches over the buffer, decisions taken on the device from a caller-owned control block.
 * THE GUARD LOOKS AT THE GRADIENT, NOT AT THE LOSS.  A NaN loss means NaN in pred, hence in dpred, hence in the head's gradients, so the
 * gradient test subsumes train.py:194; after the all-reduce the flat gradient is bit-identical on every rank, so every rank takes the
 * same decision with no extra collective (the reference's rank-local test lets DDP ranks diverge); and it also catches the NaN / Inf
 * gradient under a finite loss, which the reference would clip into NaN parameters.
 * What the guard cannot see is a NaN that never reaches the gradient.  The ReLU of every conv / GEMM epilogue hands a NaN on (relu_f), so
 * a NaN pixel reaches the loss through the HRNet backbones; the CPN-50 backbone's max pool (elementwise.hip) and the block maximum that
 * scales the planes-out tile of igemm_f32h2_ws still take fmaxf, which returns the other operand for a NaN: behind those two a poisoned
 * pixel can be swallowed in front of the lifter, the loss stays finite and the step is taken, as it was before revision 11.
 * Everything below enqueues on `stream`, allocates nothing and never synchronises. */
typedef struct capf_optim_report {   /* the first sizeof(capf_optim_report) bytes of the control block: copy them back whenever you like */
    int64_t steps_taken;             /* updates applied: AdamW's `step` (bias correction is computed from this count, on the device) */
    int64_t steps_skipped;           /* attempts whose gradient was not finite: parameters and both moments left untouched */
    int64_t nonfinite_losses;        /* attempts whose `loss` was NaN / Inf (counted, kept out of loss_sum) */
    int64_t grad_nonfinite;          /* last attempt: 1 when an element of grad_scale * g was NaN / Inf */
    double grad_sumsq;               /* last attempt: sum of (grad_scale * g[i])^2, fp64 */
    double grad_norm;                /* last attempt: sqrt(grad_sumsq) */
    double clip_coef;                /* last attempt: min(1, max_norm / (grad_norm + 1e-6)); 1 without clipping */
    double loss_sum, loss_rows;      /* sums over attempts with a finite loss: loss * rows, rows (epoch_loss_3d, N of train.py:191-192) */
} capf_optim_report;
/* one AdamW parameter group's stretch of the flat buffer (run_3dhp.py:260-277: sampling_offsets at 0.1 x lr) */
typedef struct capf_optim_segment {
    int64_t begin, end;              /* elements [begin, end); any offsets, begin == end allowed */
    float lr, weight_decay;
} capf_optim_segment;
#define CAPF_OPTIM_MAX_SEGMENTS 64
/* bytes of the control block (device memory, 8-byte aligned, caller-owned) */
size_t capf_optim_ctrl_bytes(void);
/* zero the block and set the step count (0 for a new run; the `step` of a loaded optimizer.state_dict(), train.py:398-407) */
int capf_optim_ctrl_init(void* stream, void* ctrl, int64_t steps_taken);
/* first launch: per-block fp64 sums of (grad_scale * g[i])^2 and non-finite flags into the control block.  The grid is fixed (not
 * sized by the device), every reduction has a fixed order: the same buffer gives the same bits on every box, rank and run. */
int capf_grad_sumsq(void* stream, const float* grads, int64_t n, float grad_scale, void* ctrl);
/* second launch, after capf_grad_sumsq of the same grads / n / grad_scale: every block adds the partial sums in the same order,
 *     norm = sqrt(sum), coef = min(1, max_norm / (norm + 1e-6)) in fp64 (max_norm <= 0: no clipping),
 *     skip = a non-finite element was seen or norm is not finite;
 * skip: params, exp_avg, exp_avg_sq are not written and steps_taken stays; otherwise capf_adamw_step's arithmetic on
 * (g * grad_scale) * (float)coef with the lr / weight_decay of the element's segment and step = steps_taken + 1.
 * segments: 1 .. CAPF_OPTIM_MAX_SEGMENTS (more: CAPF_ERR_UNSUPPORTED) sorted, disjoint, covering [0, n) (else CAPF_ERR_INVALID); copied
 * by value.  attempt: the caller's count of calls on this control block, 1, 2, ... (its parity picks the state slot that is written,
 * the other one is read).  loss (device, may be NULL) and rows feed loss_sum / loss_rows / nonfinite_losses whether or not the step
 * is skipped. */
int capf_adamw_step_guarded(void* stream, float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                            const capf_optim_segment* segments, int n_segments, float beta1, float beta2, float eps,
                            float grad_scale, float max_norm, int64_t attempt, const float* loss, int rows, void* ctrl);

/* Lifter only, on the context maps left in the workspace by the last capf_backbone_forward /
 * capf_forward of the same batch (or copied there by capf_set_features).  Replaces self.volume_net(...) conpose.py:40
 * (PoseTransformer.forward pose_dformer.py:210-241).  kcrop_inout is normalised in place.
 * CAPF_ERR_STATE (capf_last_error says why), like capf_lifter_forward_train, when the workspace holds no whole set of maps of THIS batch:
 * after a run of another batch (every buffer lives at offset * batch), after a capf_forward_prefix that ended inside the backbone, after
 * capf_set_workspace.  A refused call launches nothing and leaves the saved training step and capf_train_generation as they were. */
int capf_lifter_forward(capf_handle* h, void* stream, const float* k2d, float* kcrop_inout, int batch,
                        float* out);

/* ---- the lifter on caller-supplied context maps, with gradients to the maps ---------------------------------------------------------
 * What CA_PF with config.model.backbone.fix_weights = False needs from the lifter (conpose.py:22-25: the backbone is trained through
 * volume_net, i.e. autograd through the two F.grid_sample sites pose_dformer.py:128 and :217): PoseTransformer.forward on maps that a
 * backbone OUTSIDE this library produced, and dL/d(maps) next to the parameter gradients.  The native backbone stays frozen.
 * fp32 plans only: on a handle with compute_dtype bf16 / fp16 capf_set_features and capf_backward_maps return CAPF_ERR_UNSUPPORTED
 * (capf_last_error says why).
 *
 * capf_set_features: replaces `features_list = self.backbone(images)` (conpose.py:38) by a copy of the caller's maps: feat_nhwc[l] is
 *     fp32 NHWC [batch, H_l, W_l, C_l] of the plan's geometry (capf_tensor("feat0".."feat3") reports it), copied into the workspace's
 *     feat0..3 on `stream`.  The maps are then valid for `batch`: capf_lifter_forward and capf_lifter_forward_train run on them.
 *     Like every run it invalidates saved training activations.  NULL pointers, batch < 1 or > capf_max_batch: CAPF_ERR_INVALID.
 * capf_lifter_forward_train: replaces self.volume_net(...) (conpose.py:40) under model.train(): the lifter half of capf_forward_train
 *     (same code, same bits: capf_backbone_forward + capf_lifter_forward_train IS capf_forward_train) on the maps in the workspace,
 *     which capf_set_features or a whole backbone run (capf_backbone_forward, capf_forward*) of the same batch left there; otherwise
 *     CAPF_ERR_STATE.  drop_masks as capf_forward_train takes them; works without context blocks (`depth` blocks) too.
 * capf_backward_maps: replaces loss.backward() through volume_net INTO features_list (train.py:195 with a trainable backbone):
 *     capf_backward -- flat_grad gets the same bits -- plus dfeat_nhwc[l] = dL/d(feat_l), caller-owned fp32 NHWC
 *     [batch, H_l, W_l, C_l], 16-byte aligned, zeroed and overwritten by this call (garbage on entry is fine).  Valid after
 *     capf_forward_train or capf_lifter_forward_train, under capf_backward's generation / CAPF_ERR_STATE rules.
 *     Many samples meet in one pixel, and capf_set_map_grad_mode picks how their contributions are summed; flat_grad has the same,
 *     reproducible bits in both modes.  Mode 0 (default): fp32 atomic adds, whose order is not fixed -- dfeat_nhwc is NOT bit-reproducible
 *     from run to run (last-bit differences).  Mode 1: the ordered sum below -- bit-identical from run to run and from handle to handle
 *     on the same inputs.
 * capf_set_map_grad_mode: 0 = atomic (default), 1 = ordered; any other value CAPF_ERR_INVALID.  A state change only (plan-only handles
 *     take it too); it affects nothing but the dfeat_nhwc half of capf_backward_maps.  CAPF_ERR_UNSUPPORTED on a bf16 / fp16 handle.
 *     The ordered sum: an item is one corner (dy, dx) of one bilinear sample, numbered it = ((p * heads + h) * samples + s) * 4 + dy * 2 + dx
 *     at a deformable sampler (joint p, head h, sample s; weight softmax_s * wx * wy, source row dL/dU[b, p, h]) and it = p * 4 + dy * 2 + dx
 *     at the reference-point sampler (weight wx * wy, source row dL/dS_l[b, p]; corners outside the map dropped).  For one sampler pass,
 *     S[pixel][c] = sum over the items that fall into the pixel, in ascending it, in fp32, of weight_it * row_it[c], and
 *         dfeat = ((((0 + S_ctx[levels-1]) + S_ctx[levels-2]) + ...) + S_ctx[0]) + S_ref
 *     (context blocks in the order the backward visits them, then the reference pass; without context blocks dfeat = 0 + S_ref).  No
 *     atomics, no extra workspace: capf_workspace_bytes is the same in both modes.  The kernel's key space is 2048 items per frame and level
 *     in a pass (joints * heads * samples * 4); every configuration capf_create accepts stays within it (64 items a joint, at most 17 joints:
 *     1088 at the most, at the shipped configurations too).
 * capf_map_grad_mode: the current mode (-1 for a NULL handle). */
int capf_set_features(capf_handle* h, void* stream, const float* const feat_nhwc[4], int batch);
int capf_lifter_forward_train(capf_handle* h, void* stream, const float* k2d, float* kcrop_inout, int batch, float* out,
                              const float* drop_masks);
int capf_backward_maps(capf_handle* h, void* stream, const float* grad_out, int batch, float* flat_grad, const float* drop_masks,
                       float* const dfeat_nhwc[4]);
int capf_set_map_grad_mode(capf_handle* h, int mode);
int capf_map_grad_mode(const capf_handle* h);

/* ---- gradients w.r.t. the keypoints ---------------------------------------------------------------------------------------------------
 * PoseTransformer.forward is differentiable in its two keypoint inputs as well: coord_embed(keypoints_2d) (pose_dformer.py:214),
 * grid_sample(features, ref) (:217) and pos = offsets + ref in every DeformableBlock (:125).  A model whose keypoints come out of a
 * trainable network (a soft-argmax head on the backbone that capf_set_features serves) needs them.
 * capf_backward_points: capf_backward -- flat_grad gets the same bits -- plus up to three optional outputs, each NULL or caller-owned:
 *     dfeat_nhwc  NULL, or the four maps of capf_backward_maps, with its bits (exactly in map_grad_mode 1, the same sums in mode 0);
 *     dk2d        [batch, joints, 2] fp32: dL/d(k2d) = dL/dX[b, p, 0, :] coord_embed.weight, overwritten;
 *     dref        [batch, joints, 2] fp32: dL/d(ref), the gradient w.r.t. the NORMALISED reference points, i.e. the values kcrop_inout
 *                 holds after the forward; overwritten.  The caller who wants the gradient w.r.t. the crop pixels it passed divides by
 *                 (96, 128), the constants of conpose.py:34 (CA_PF does).
 *     With all three NULL the call is capf_backward, launch for launch.  Valid after capf_forward_train / capf_forward_train_u8 /
 *     capf_lifter_forward_train under capf_backward's rules (generation, CAPF_ERR_STATE, batch); NULL grad_out / flat_grad, a NULL
 *     among the four dfeat_nhwc pointers or a misaligned one: CAPF_ERR_INVALID.  fp32 plans only: CAPF_ERR_UNSUPPORTED on a bf16 / fp16
 *     handle (capf_last_error names the entry and the dtype).  No extra workspace; second derivatives are not provided.
 *     dref is ONE fixed fp32 expression, bit-identical from run to run and from handle to handle on the same inputs (no atomics):
 *         dref = ((((0 + c[levels-1]) + c[levels-2]) + ...) + c[0]) + r_ref              (without context blocks: dref = 0 + r_ref)
 *     c[i][b, p]: context block i's samplers, a running sum from 0 over level l ascending and, inside a level, k = head * samples + sample
 *         ascending of dL/dpos[l][k] = softmax weight * (size_l - 1) / 2 * [coordinate not clipped by the border] * sum_c dL/dU * dv/dpos
 *         (ATen's clip_coordinates_set_grad mask; the blocks in the order the backward visits them);
 *     r_ref[b, p] = ((g_0 + g_1) + g_2) + g_3, g_l = (size_l - 1) / 2 * sum_c dL/dS_l[c] * d(bilinear, zeros padding)/d(ref): a corner
 *         outside the map reads 0, no clip mask; a point wholly outside a map, or a 1 x 1 map, contributes exactly 0.
 *     dk2d is a fixed expression too (lane i of 64 sums channels i, i + 64, ... ascending, then an xor tree).
 *     grid_sample's derivative w.r.t. a position is one-sided at cell boundaries and at the border clip: dref is the derivative in the
 *     cells and on the clip sides the forward used.
 *     Cost (MI355X, HRNet-32 fp32 256 x 256, medians of 20, tools/bench_points_grad.py, EXPERIMENTS.md R23.1): with all three outputs
 *     3.929 ms against capf_backward_maps' 3.910 ms at batch 64 and 12.260 against 11.986 ms at batch 512 (atomic mode; ordered: 3.568
 *     against 3.542 and 10.323 against 10.024); with dk2d and dref alone 3.188 ms against capf_backward's 3.137 ms at batch 64 and 8.589
 *     against 8.282 ms at batch 512 (feat_embed's input gradient, one small launch, a block barrier in four launches).  capf_backward
 *     itself, this revision against the one before it in alternating processes of one session: 3.127 - 3.133 against 3.136 - 3.151 ms at
 *     batch 64, 8.716 - 8.747 against 8.759 - 8.764 ms at batch 512 (spread of a series 1.3 - 2.1 %): unchanged. */
int capf_backward_points(capf_handle* h, void* stream, const float* grad_out, int batch, float* flat_grad, const float* drop_masks,
                         float* const dfeat_nhwc[4], float* dk2d, float* dref);

/* How the independent branches of the backbone (the 2-4 resolution branches of an HRNet module, the
 * fused outputs, the CPN refine cascades) are issued:
 *   0 = everything in program order on the caller's stream;
 *   1 = on library-owned side streams, forked from / joined to the caller's stream with events;
 *   2 = by dependency level on the caller's stream, the convolutions of a level sharing ONE grouped launch;
 *   3 = (default) as 2, but at batch 16..128 the lanes of a region form TWO such chains -- lanes 0 + 3 on the caller's stream,
 *       1 + 2 on a library-owned side stream (fork / join with events) -- so that one chain's launch ramp and tail overlap
 *       the other's body.
 * The results are bit-identical in modes 0, 2 and 3 (mode 1 has no split-K scratch: equal to roundoff at small batches). */
int capf_set_lanes(capf_handle* h, int on);

/* When on, forward also snapshots the token buffer after each block group (tok_ctx/tok_res/tok_joint). */
int capf_set_debug(capf_handle* h, int on);

/* Intermediates of the LAST forward, for stage-level parity tests.  Names:
 *   feat0..feat3   context maps, NHWC [B,h,w,C_l]
 *   heat           CAPF_PLAN_CPN_PREDICT handles only: final_predict's heatmaps, NHWC [B,64,48,20] in the context maps' format (fp32 / bf16),
 *                  channels 17..19 exact zeros; reserved to the end of the run like feat0..3 (the input of capf_cpn_decode)
 *   sampled0..3    reference-point samples [B,17,C_l]          (pose_dformer.py:216-218)
 *   idx0..idx3     int32 [B,17,2] (ix0, iy0) bilinear NW corner of those samples (bit-exact check)
 *   cpos0..3       with capf_set_debug: sampling positions of DeformableBlock i, fp32 [B,17,L*16,2] (level, head*4+sample)
 *   cidx0..3       ... and the int32 NW corner (ix0, iy0) of each, padding_mode='border' (pose_dformer.py:126-128)
 *   tok_ctx / tok_res / tok_joint   token buffer [B,17,L+1,c] after each block group (layout b p l c)
 *   stem           where the conv that reads the image writes, NHWC [B,H/2,W/2,64] in the plan's activation format.  Unlike the names above
 *                  its memory is NOT reserved: later ops of the same run reuse it, so after a run it holds a function of that run alone
 *                  (two routes of one plan and batch -- capf_forward / capf_forward_u8 -- compare bit for bit; it is not the conv's output)
 * Pointers are into the workspace and valid until the next forward on this handle.
 * Returns 0 for an fp32 tensor, 1 for an int32 tensor, 2 for a bf16 tensor (context maps of a
 * CAPF_BF16 handle; fp32 under CAPF_PLAN_BF16_F32_STREAM), 3 for an fp16 tensor (context maps of a
 * CAPF_F16 handle), negative on error. */
int capf_tensor(const capf_handle* h, const char* name, const void** dev_ptr, int64_t shape[4],
                int* ndim);

/* Number of kernel launches and algorithmic FLOPs (2*MAC of convs + GEMMs) of one forward at
 * `batch`; used by bench.py for the roofline line. */
/* after capf_forward_profile_launches: for every leader op of a grouped bf16 conv launch, which device kernel the launch ran
 * (0 igemm_bf16_group_kernel: ring schedule, 1 igemm_bf16_group_pp_kernel: ping-pong, 2 igemm_bf16_group_rh_kernel: ping-pong
 * with row-halo tiles, 3 igemm_bf16_group_ws_kernel: the 2-D halo tile, a launch of one conv included); -1 for every other op.  Lets bench.py
 * name launches the way rocprofv3 does.                                                                                          */
int capf_forward_profile_variants(const capf_handle* h, int32_t* op_variant, int n_ops);
int capf_forward_stats(const capf_handle* h, int batch, int64_t* launches, double* flops);

/* ---- stateless operator entry points (op-level parity tests and micro-benchmarks) ---------------
 * capf_op_pack_conv : fold eval-mode BatchNorm into a conv weight and re-lay it out K-major:
 *     w_packed[Cout][Kpad] (Kpad = ks*ks*Cin rounded up to 32), bias[Cout]; gamma == NULL -> no BN.
 * capf_op_conv      : y = act(conv2d(x; w_packed) + bias (+ residual)), NHWC, padding = ks/2.
 *     == nn.Conv2d(bias=False) + nn.BatchNorm2d(eval) (+ residual add) (+ ReLU) of
 *     pose_hrnet.py:66-136 / networks/resnet.py:58-93 as ONE implicit-GEMM launch.
 * capf_op_linear    : y[M,N] = act(x[M,K] @ w[N,K]^T + bias (+ residual)); act 0 none, 1 ReLU, 2 GELU(erf)
 *     == nn.Linear (+GELU) of pose_dformer.py:15-31; K % 32 == 0.                                      */
int capf_op_pack_conv(void* stream, const float* w_oihw, const float* gamma, const float* beta,
                      const float* mean, const float* var, float eps, float* w_packed, float* bias,
                      int Cout, int Cin, int ks);
int capf_op_conv(void* stream, const float* x_nhwc, const float* w_packed, const float* bias,
                 const float* residual, float* y_nhwc, int B, int H, int W, int Cin, int Cout, int ks,
                 int stride, int act);
/* capf_op_conv_group : up to 8 INDEPENDENT capf_op_conv problems (Cin % 4 == 0, ks <= 5) as ONE grouped
 *     launch -- what the engine issues for the same-depth convs of the HRNet branches
 *     (pose_hrnet.py:242-255: the branches of a HighResolutionModule do not depend on each other) and of
 *     a fuse layer (:257-303).  Results are bit-identical to n capf_op_conv calls. */
typedef struct capf_conv_desc {
    const float* x;         /* [B,H,W,Cin] NHWC */
    const float* w_packed;  /* capf_op_pack_conv output */
    const float* bias;
    const float* residual;  /* [B,Ho,Wo,Cout] or NULL */
    float* y;               /* [B,Ho,Wo,Cout] */
    int32_t B, H, W, Cin, Cout, ks, stride, act;
} capf_conv_desc;
int capf_op_conv_group(void* stream, int n, const capf_conv_desc* convs);
/* The same 3x3 / stride-1 / pad-1 convolution through the Winograd-along-W kernels (csrc/igemm_wino.hip), results equal to
 * the direct kernel's to fp32 roundoff.  variant 23: F(2,3), 1.5x fewer MFMAs, wp [Cout][12 * Cin], even W;  variant 43:
 * F(4,3), 2x fewer MFMAs, wp [Cout][18 * Cin], W % 4 == 0.  capf_op_pack_conv_wino folds BatchNorm like capf_op_pack_conv
 * and applies the weight transform.  Needs Cin % 32 == 0, Cout % 4 == 0 (CAPF_ERR_UNSUPPORTED otherwise).
 * capf_op_conv_wino_group: up to 8 such convs of one variant in one grid (capf_conv_desc with ks 3, stride 1). */
int capf_op_pack_conv_wino(void* stream, const float* w, const float* gamma, const float* beta, const float* mean,
                           const float* var, float eps, float* wp, float* bias, int Cout, int Cin, int variant);
int capf_op_conv_wino(void* stream, const float* x, const float* wp, const float* bias, const float* residual, float* y, int B,
                      int H, int W, int Cin, int Cout, int act, int variant);
int capf_op_conv_wino_group(void* stream, int n, const capf_conv_desc* d, int variant);
int capf_op_linear(void* stream, const float* x, const float* w, const float* bias, const float* residual,
                   float* y, int M, int N, int K, int act);
/* Training-mode BatchNorm2d as capf_backbone_forward_bn runs it (csrc/bn_train.hip), on x [rows = B * H * W, C] NHWC fp32; C % 4 == 0, C <= 1024.
 * capf_op_bn_stats: the batch statistics of x -- per-slab fp64 partial means / sums of squared deviations, combined by a second launch in a
 *     fixed order, no atomics: bit-identical from run to run -- into scale[c] = gamma[c] / sqrt(var[c] + eps) and
 *     shift[c] = beta[c] - mean[c] * scale[c]; running_mean / running_var (each may be NULL) are updated in place with `momentum` as above.
 *     scratch: capf_op_bn_stats_scratch_bytes(rows, C) bytes of device memory, 8-byte aligned (0: a shape the kernels do not take).
 *     rows < 2: CAPF_ERR_INVALID.
 * capf_op_bn_apply: y = act(x * scale[c] + shift[c] + residual); y may be x, residual may be NULL; act 0 none, 1 ReLU (a NaN stays a NaN). */
size_t capf_op_bn_stats_scratch_bytes(int64_t rows, int C);
int capf_op_bn_stats(void* stream, const float* x, int64_t rows, int C, const float* gamma, const float* beta, float eps, float momentum,
                     float* running_mean, float* running_var, float* scale, float* shift, void* scratch, size_t scratch_bytes);
int capf_op_bn_apply(void* stream, const float* x, const float* scale, const float* shift, const float* residual, float* y, int64_t rows, int C,
                     int act);
/* capf_op_bilinear_corners: the corner rule of both sampling sites (F.grid_sample, bilinear, align_corners=True) on
 * caller-supplied normalised coordinates grid [n,2] = (x, y): idx [n,2] = NW corner (x0, y0), frac [n,2] = weights of the
 * +1 corners.  border = 1: padding_mode='border' (DeformableBlock, pose_dformer.py:128), 0: 'zeros' (:217).  The same
 * device function serves capf_forward; inside a forward the corners actually used are exposed through capf_tensor
 * ("idx{l}" / "cidx{i}" under capf_set_debug).  Must equal ATen's index arithmetic bit for bit.                     */
int capf_op_bilinear_corners(void* stream, const float* grid, int n, int H, int W, int border, int32_t* idx, float* frac);
/* bf16 twins (igemm_bf16.hip, v_mfma_f32_32x32x16_bf16): x / residual / y are bf16 NHWC, w_packed is bf16
 * [Cout][Kpad] with Kpad = ks*ks*Cin rounded up to 64, bias stays fp32.  Cin % 8 == 0, Cout % 4 == 0. */
int capf_op_pack_conv_bf16(void* stream, const float* w_oihw, const float* gamma, const float* beta,
                           const float* mean, const float* var, float eps, void* w_packed_bf16, float* bias,
                           int Cout, int Cin, int ks);
int capf_op_conv_bf16(void* stream, const void* x_nhwc_bf16, const void* w_packed_bf16, const float* bias,
                      const void* residual_bf16, void* y_nhwc_bf16, int B, int H, int W, int Cin, int Cout,
                      int ks, int stride, int act);

/* "Row-halo" variant of the 3x3 / stride-1 / pad-1 bf16 conv (what capf_forward runs for the BasicBlock convs of a bf16 model
 * from 2048 tiles per launch): K order (kh, Cin / cw, kw, cw) so that one staged activation tile serves the three kw taps.
 * cw = capf_op_conv_bf16_rh_width(Cin) (64, 48 or 32; 0 = Cin not supported); w_packed is bf16 [Cout][9 * Cin].            */
int capf_op_conv_bf16_rh_width(int Cin);
int capf_op_pack_conv_bf16_rh(void* stream, const float* w_oihw, const float* gamma, const float* beta, const float* mean,
                              const float* var, float eps, void* w_packed_bf16, float* bias, int Cout, int Cin);
int capf_op_conv_bf16_rh(void* stream, const void* x_nhwc_bf16, const void* w_packed_bf16, const float* bias,
                         const void* residual_bf16, void* y_nhwc_bf16, int B, int H, int W, int Cin, int Cout, int act);

/* "2-D halo" tile of the 3x3 / stride-1 / pad-1 bf16 conv (csrc/igemm_bf16_ws.hip; what capf_forward runs for the BasicBlock convs
 * of a bf16 model, pose_hrnet.py:66-95, and the 3x3 of the ResNet / refine bottlenecks, networks/resnet.py:58-93, from 512 tiles
 * per launch): a block keeps 256 output pixels x 32 / 64 / 96 channels in its accumulators for the whole K and stages every
 * 16-channel chunk of its pixels (with halo) once for all nine taps.  Cin % 16 == 0, Cout % 8 == 0, (rows + 2) x (W + 2) <= 416
 * for some row count dividing H.  w_packed holds capf_op_conv_bf16_ws_pack_elems(Cout, Cin) bf16 elements written by
 * capf_op_pack_conv_bf16_ws (BatchNorm folded as in capf_op_pack_conv_bf16; bias fp32 [Cout], may be NULL).
 * capf_op_conv_bf16_ws_group: up to 8 such convs in ONE grid, the way capf_forward issues a level; capf_conv_desc with bf16 x /
 * residual / y and w_packed in this layout (ks = 3, stride = 1).                                                                                              */
int64_t capf_op_conv_bf16_ws_pack_elems(int Cout, int Cin);
int capf_op_pack_conv_bf16_ws(void* stream, const float* w_oihw, const float* gamma, const float* beta, const float* mean,
                              const float* var, float eps, void* w_packed_bf16, float* bias, int Cout, int Cin);
int capf_op_conv_bf16_ws_group(void* stream, int n, const capf_conv_desc* convs);

/* Split-fp32 tile of the 3x3 / stride-1 / pad-1 fp32 conv (csrc/igemm_f32x3_ws.hip; what capf_forward runs for the BasicBlock convs of
 * an fp32 model, pose_hrnet.py:66-95, from 370 MFLOP per conv and batch 5): fp32 tensors in and out; every operand is split, exactly, into three
 * bf16 numbers and the six piece products of weight >= 2^-18 run on the bf16 matrix pipe with fp32 accumulation -- the dropped
 * products are below the rounding of one fp32 multiply, so results agree with the direct fp32 kernel to accumulation order.
 * (Non-finite / denormal operands: an infinite input gives NaN -- Inf - Inf in the split -- where the fp32 pipe gives +-Inf; fp32 denormals are
 * flushed.)  Cin % 16 == 0, Cout % 4 == 0, W <= 256.  w_packed holds capf_op_conv_f32x3_pack_elems(Cout, Cin) bf16 elements written by
 * capf_op_pack_conv_f32x3 (BatchNorm folded as in capf_op_pack_conv, then split; bias fp32 [Cout], may be NULL).
 * capf_op_conv_f32x3_group: up to 8 such convs in ONE grid (capf_conv_desc with w_packed in this layout, ks = 3, stride = 1).       */
int64_t capf_op_conv_f32x3_pack_elems(int Cout, int Cin);
int capf_op_pack_conv_f32x3(void* stream, const float* w_oihw, const float* gamma, const float* beta, const float* mean,
                            const float* var, float eps, void* w_packed_bf16, float* bias, int Cout, int Cin);
int capf_op_conv_f32x3_group(void* stream, int n, const capf_conv_desc* convs);

/* The default split-fp32 tile (csrc/igemm_f32h2_ws.hip; what capf_forward runs for those convs unless CAPF_PLAN_F32X3_EXACT / _NO_F32X3):
 * fp32 tensors in and out; an operand a travels as two fp16 numbers a1 = fp16(s a), a2 = fp16(s a - a1) under an exact power-of-two scale s
 * (weights: one per output channel, fixed at pack time; pixels: one per block of 256 output pixels and 16-channel chunk, found inside the
 * kernel from the values it staged -- nothing outside the kernel sees a scale), |s a - a1 - a2| <= 2^-23 |s a|; the three products
 * a1 w1 + a1 w2 + a2 w1 run on the 16-bit matrix pipe with fp32 accumulation (dropped: a2 w2 <= 2^-22 |a w|).  One term is therefore within
 * 2^-21 of the fp32 product, which over a dot product of 9 Cin terms is below the fp32 accumulation error of ANY fp32 evaluation: the tests
 * hold this tile to the same bound as the three-piece tile (<= 1e-6 of the sum of |terms| against fp64, <= 2 x this library's direct fp32
 * MFMA kernel on the same problem).  Ranges: values whose magnitude is below 2^-18 of their block's largest lose relative precision
 * (absolute error <= 2^-39 of that largest value); scales are kept within 2^+-63: block maxima in [2^-49, 2^77) = 1.8e-15 .. 1.5e23 get
 * their exact scale, smaller ones lose precision gradually (all-zero blocks are exact), a block maximum of 2^77 or more overflows fp16
 * (Inf, then NaN); Inf / NaN inputs give NaN for their whole block and chunk (CAPF_PLAN_NO_F32X3 keeps the fp32 pipe's IEEE behaviour).
 * THE BOUND, per output y = sum_k a_k w_k, with M_c the largest |a| among the values its block staged for 16-channel chunk c (256 output
 * pixels + their 1-pixel halo; for capf_op_*_f32h2_gemm: the 32 rows x 32-deep chunk of a wave) and W_c = sum over that chunk of |w_k|:
 *     |y - exact| <= 2.5e-6 sum_k |a_k w_k|  +  2^-38 sum_c M_c W_c
 * -- the first term is an fp32 accumulation's own (observed <= 1e-6 on every fuzzed problem, and at most 2 x this library's fp32-pipe kernel
 * on the same operands everywhere; a sum dominated by ONE term costs any fp32 evaluation 1 - 2e-6); the second only shows when a block holds
 * values more than 2^18 apart (one outlier pixel 2^20 above a flat tile costs the flat tile's outputs ~2e-6 of THEIR sum of |terms|).
 * tests/test_gpu_ops.py test_f32h2_dynamic_range_inside_a_block asserts exactly this with outliers of 2^8 .. 2^20 for the conv tile, the GEMM
 * (conv and rows mode; 3e-6 there) and the weight gradient (5e-6: 2048-term sums), and the plain 1e-6 for blocks that hold no outlier.
 * A scale follows the data downwards without limit and upwards by at most 2^80 above the smallest scale its tile has used (the accumulators
 * must not overflow behind a chunk of zeros).
 * BATCH COMPOSITION: a block's scale depends on everything the block stages.  Conv tiles never span frames unless H W < 256 (8x8 maps: four
 * frames per tile); the GEMM's 32-row blocks of the lifter's [B 17, K] operands do.  A frame's output BITS may therefore depend on its
 * neighbours in the batch (within the bound above); CAPF_PLAN_NO_F32X3 | CAPF_PLAN_NO_F32H2_GEMM gives batch-independent bits.  Same shapes
 * as above; w_packed holds capf_op_conv_f32h2_pack_elems(Cout, Cin) 16-bit elements (pieces, then the fp32 inverse channel scales).
 * Tensor sizes: a tile addresses its pixels and its output rows from per-tile bases, so x / y / residual may exceed 2 GiB (only B * H * W
 * has to stay below 2^31): conv2 and both transition1 convs at 512 frames (2.1 GB of fp32 each) run here.                                  */
int64_t capf_op_conv_f32h2_pack_elems(int Cout, int Cin);
int capf_op_pack_conv_f32h2(void* stream, const float* w_oihw, const float* gamma, const float* beta, const float* mean,
                            const float* var, float eps, void* w_packed_f16, float* bias, int Cout, int Cin);
int capf_op_conv_f32h2_group(void* stream, int n, const capf_conv_desc* convs);

/* PLANES (round 6): a tensor that only travels from one two-fp16-piece tile conv to the next -- a BasicBlock's conv1 -> conv2, pose_hrnet.py:78-88 --
 * can stay SPLIT in memory: per pixel and 16-channel chunk [piece 0: 16 fp16 | piece 1: 16 fp16], the same 64 bytes at the same addresses as the fp32
 * values, under one power-of-two scale per (256-pixel tile, chunk) whose biased exponent is kept in a [tiles][channels / 16] int32 table.  The consumer
 * stages the pieces as they are (no maximum, no split, no scale exchange in its K loop) and only moves the two halo rows that came from the neighbouring
 * tiles onto the smallest of the three scales (a power of two: exact).  Stored values are fp32 numbers of 22 significant bits (|v - stored| <= 2^-23 |v|,
 * what the consumer's own split would have made of them); THE BOUND above holds with M_c = the largest value of the three tiles a tile's rows come from.
 * capf_op_conv_f32h2_planes: one such conv.  exps_in != NULL: conv->x holds planes (Cin % 16 == 0) and exps_in their table; exps_out != NULL: conv->y
 * is written as planes (Cout % 16 == 0, no residual) and exps_out receives capf_op_conv_f32h2_tiles(B, H, W, ..) x Cout / 16 exponents.  Producer and
 * consumer must have the same B, H, W (same tiles).  capf_forward uses the pair for every BasicBlock whose two convs run this tile
 * ONLY under CAPF_PLAN_H2_PLANES: the split moves, it does not disappear, and the forward measured 3 % slower with it (EXPERIMENTS R6.5).                                                                               */
int capf_op_conv_f32h2_tiles(int B, int H, int W, int* tile_pixels);     /* tiles; *tile_pixels (may be NULL): output pixels per tile, flat pixel p -> tile p / that */
int capf_op_conv_f32h2_planes(void* stream, const capf_conv_desc* conv, const int32_t* exps_in, int32_t* exps_out);

/* The two-fp16-piece arithmetic for every OTHER fp32 conv / linear (csrc/igemm_f32h2.hip; what capf_forward runs from batch 5 for the 1x1 and
 * stride-2 convs of the fuse / transition layers, pose_hrnet.py:225-303, lone convs, and -- in inference plans -- the lifter's nn.Linear layers,
 * pose_dformer.py:15-59): the activation tile is staged as fp32 and split by the wave that consumes it (one power-of-two scale per wave,
 * 32 rows and 32-deep K chunk), the weights are split at pack time (one scale per output channel); same ranges and the same accuracy
 * statement as capf_op_conv_f32h2_group.  capf_op_pack_f32h2_gemm writes capf_op_f32h2_gemm_pack_elems(N, K) floats: the fp32 pack's
 * [N][Kpad] geometry (Kpad = K rounded up to 32; conv: ks >= 1, w OIHW, K = ks * ks * Cin, BatchNorm folded, bias written if not NULL;
 * linear: ks = 0, Cin ignored, w [N][K], bias untouched) holding [piece 0: 32 fp16 | piece 1: 32 fp16] per 32-deep chunk, then the N
 * fp32 inverse channel scales.  capf_op_conv_f32h2g / capf_op_linear_f32h2g: capf_op_conv / capf_op_linear on that pack (Cin % 4 == 0,
 * Cout % 4 == 0, ks <= 5; K % 32 == 0, N % 4 == 0); capf_op_conv_f32h2g_group: up to 8 such convs in one grid.  A conv's input may exceed
 * 2 GiB (offsets count from the tile's first input pixel); outputs and rows-mode operands below 4e9 elements / bytes as for capf_op_conv.
 * The training step uses the same kernel for y = x W^T and dX = dY W (packs of W and W^T rebuilt from the parameters at the start of every
 * capf_forward_train, DropPath's per-row branch scale in the epilogue) and its sibling wgrad_tn_h2_kernel for dW = dY^T x (both operands
 * split in the kernel): capf_train_h2_matrices().                                                                                       */
int64_t capf_op_f32h2_gemm_pack_elems(int N, int K);
int capf_op_pack_f32h2_gemm(void* stream, const float* w, const float* gamma, const float* beta, const float* mean, const float* var,
                            float eps, float* w_packed, float* bias, int N, int Cin, int ks, int K);
int capf_op_conv_f32h2g(void* stream, const float* x_nhwc, const float* w_packed, const float* bias, const float* residual, float* y,
                        int B, int H, int W, int Cin, int Cout, int ks, int stride, int act);
int capf_op_conv_f32h2g_group(void* stream, int n, const capf_conv_desc* convs);
int capf_op_linear_f32h2g(void* stream, const float* x, const float* w_packed, const float* bias, const float* residual, float* y,
                          int M, int N, int K, int act);
/* ... with LayerNorm(x rows over their K <= 256 columns; gamma, beta [K], eps) folded in front of the product -- Block.norm1 -> attn.qkv and
 * norm2 -> mlp.fc1 of the res blocks, norm2 -> mlp.fc1 of the DeformableBlocks (pose_dformer.py:62-79, 137-138): statistics in fp32 per row
 * (two passes), x_hat = ((x - mean) * rstd) * gamma + beta in fp32, and THAT value is split into the two fp16 pieces.                  */
/* The training step's weight gradient as an operator (train.py:195, loss.backward() through an nn.Linear): dW[N, K] = dY[M, N]^T X[M, K] and
 * db[N] = column sums of dY, written to dw_db[N K + N], straight from the row-major operands (csrc/train_kernels.hip).  two_piece = 1: BOTH
 * operands as two block-scaled fp16 pieces (wgrad_tn_h2_kernel: N, K multiples of 128; one scale per wave, operand and 32-row chunk that only
 * ever goes down along M -- the bound above with M_c = the largest value of the operand block so far); 0: the fp32 matrix pipe
 * (wgrad_tn_kernel: N, K multiples of 4).  One row slice, i.e. the summation order of a training step whose slab buffer holds one slab. */
int capf_op_wgrad(void* stream, const float* dY, const float* X, int M, int N, int K, float* dw_db, int two_piece);
int capf_op_linear_ln_f32h2g(void* stream, const float* x, const float* ln_gamma, const float* ln_beta, float eps, const float* w_packed,
                             const float* bias, const float* residual, float* y, int M, int N, int K, int act);

/* Up to 8 independent bf16 convs in one grid (what capf_forward issues per dependency level of the HRNet branches of a bf16 model):
 * capf_conv_desc with bf16 x / w_packed / residual / y.  w_row_halo[i] (optional array, entries may be NULL): the same weights
 * from capf_op_pack_conv_bf16_rh; launches of >= 2048 tiles then run the row-halo tiles for those problems, exactly as the
 * engine does.  *variant (optional) = the device kernel chosen (see capf_forward_profile_variants).                           */
int capf_op_conv_bf16_group(void* stream, int n, const capf_conv_desc* convs, const void* const* w_row_halo, int32_t* variant);

/* nn.Linear on the bf16 MFMA path (the lifter's qkv / proj / fc1 / fc2 under compute_dtype = CAPF_BF16, pose_dformer.py:15-59):
 * x bf16 [M,K], w bf16 [N,K] (K % 64 == 0), bias fp32; gelu_bf16_out = 0: y fp32 [M,N] = x w^T + bias (+ fp32 residual);
 * gelu_bf16_out = 1: y bf16 [M,N] = GELU(x w^T + bias) (exact erf).  fp32 accumulation in both.                        */
int capf_op_linear_bf16(void* stream, const void* x_bf16, const void* w_bf16, const float* bias, const float* residual, void* y,
                        int M, int N, int K, int gelu_bf16_out);

/* The 16-bit kernel families for EITHER element format: dtype = CAPF_BF16 (then exactly the capf_op_*_bf16 entries above, bit for bit) or
 * CAPF_F16 (what a CAPF_F16 handle launches; same tiles, same layouts, same routing, v_mfma_f32_32x32x16_f16 at the bf16 instruction's rate).
 * Kernel names reported for fp16 launches say f16 where the bf16 ones say bf16 ("igemm_f16_ws<w4,256x96,conv>", "bneck0_f16<8x8>").
 *   capf_op_pack_conv_16       BatchNorm fold + pack; layout 0: [Cout][Kpad64] (capf_op_pack_conv_bf16), 1: row-halo (.._bf16_rh, ks = 3),
 *                              2: the 2-D halo tile's (.._bf16_ws, ks = 3).  Weights are the folded fp32 values rounded once to the format.
 *   capf_op_conv_16            capf_op_conv_bf16; with Cin % 8 != 0 the STEM of a 16-bit plan (csrc/igemm_bf16.hip stem kernels): x is the fp32 image,
 *                              w_packed the fp32 pack of capf_op_pack_conv, no residual -- image and weights are rounded to the format on their way
 *                              into LDS (an fp16 stem clamps a pixel value beyond +-65504), y is 16-bit;  capf_op_conv_16_group: capf_op_conv_bf16_group;  capf_op_conv_16_ws_group: .._bf16_ws_group
 *   capf_op_linear_16          capf_op_linear_bf16 (gelu_out16: GELU, then a 16-bit result)
 *   capf_op_bneck_16           a layer1 bottleneck as ONE kernel (csrc/bneck_bf16.hip; networks/resnet.py:58-93): w / bias = {conv1, conv2, conv3,
 *                              downsample} from layout 0.  w[3] != NULL: the first bottleneck, x [B,H,W,64], shortcut [B,H,W,256] required;
 *                              w[3] == NULL: an identity bottleneck, x [B,H,W,256].  t1 / t2 [B,H,W,64]; y [B,H,W,256]; H % 8 == 0, W % 8 == 0.
 *                              tap != 0 also stores conv1's, conv2's and the downsample's outputs to t1 / t2 / shortcut (else scratch).
 * fp16 storage (every fp16 store of these kernels; capf_debug_f16_round runs the same expression on the host, out[i] = fp16 bits of in[i]):
 * round to nearest even; finite values beyond +-65504 and the infinities saturate to +-65504; NaN stays NaN; results below 2^-14 are stored as
 * fp16 subnormals (down to 2^-24, then zero).  DYNAMIC RANGE: an fp16 plan relies on what the two-fp16-piece fp32 tiles above rely on --
 * activations behind a folded BatchNorm and the folded weights are O(1e-3 .. 1e2); unlike those tiles it carries NO scale: a folded weight or an
 * activation above 65504 is clamped (a wrong but finite value), one below 6e-5 keeps fewer than 11 bits, one below 3e-8 is zero.  Subnormal fp16
 * operands are multiplied as the values they are: v_mfma_f32_32x32x16_f16 does not flush them (hipcc's kernel mode keeps fp16 denormals), and the
 * fp32 accumulators never flush (tests/test_gpu_f16_ops.py holds a conv of 1e-6 inputs to the usual bound).  Accumulation is fp32 as for bf16. */
int capf_op_pack_conv_16(void* stream, const float* w_oihw, const float* gamma, const float* beta, const float* mean, const float* var, float eps,
                         void* w_packed, float* bias, int Cout, int Cin, int ks, int layout, int dtype);
int capf_op_conv_16(void* stream, const void* x_nhwc, const void* w_packed, const float* bias, const void* residual, void* y_nhwc, int B, int H,
                    int W, int Cin, int Cout, int ks, int stride, int act, int dtype);
int capf_op_conv_16_group(void* stream, int n, const capf_conv_desc* convs, const void* const* w_row_halo, int32_t* variant, int dtype);
int capf_op_conv_16_ws_group(void* stream, int n, const capf_conv_desc* convs, int dtype);
int capf_op_linear_16(void* stream, const void* x, const void* w, const float* bias, const float* residual, void* y, int M, int N, int K,
                      int gelu_out16, int dtype);
int capf_op_bneck_16(void* stream, const void* x, const void* const w[4], const float* const bias[4], void* t1, void* t2, void* shortcut, void* y,
                     int B, int H, int W, int tap, int dtype);
int capf_debug_f16_round(const float* in, uint16_t* out, int n);

/* ---- the steps on either side of the path ---------------------------------
 * capf_preprocess: data_prefetcher.preload (ContextPose/mvn/datasets/utils.py:33-82) as one launch pair:
 *   images_bgr uint8 [B,H,W,3] -> images_out fp32 RGB NHWC ((u/255 - mean) / std; std == NULL: CPN, mean only);
 *   gt_in [B,1,17,3] -> gt_out root-relative (:52-53); k2d / kcrop [B,17,2] copied or mirrored.
 *   mode 0: as is.  mode 1: train-time horizontal flip of the whole batch incl. left/right joint swap and
 *   `192 - x - 1` (:55-65).  mode 2: flip-test stacking (:67-80): images_out [2,B,H,W,3], k2d_out / kcrop_out
 *   [2,B,17,2] hold the original followed by the mirrored sample, so ONE capf_forward of batch 2B serves both.
 * capf_fliptest_fuse: train.py:177-180 — pred2 [2,B,1,17,3] -> out [B,1,17,3] = mean(pred, un-mirrored pred). */
int capf_preprocess(void* stream, const uint8_t* images_bgr, int batch, int height, int width, const float mean[3],
                    const float* std3, int mode, float* images_out, const float* gt_in, float* gt_out,
                    const float* k2d_in, float* k2d_out, const float* kcrop_in, float* kcrop_out);
int capf_fliptest_fuse(void* stream, const float* pred2, int batch, float* out);

/* ---- N1 / A2 fused into the stem conv's load: the forward from uint8 crops (additive inside revision 12) -----------------------------
 * The channel flip, the normalisation and the mirror of data_prefetcher.preload (ContextPose/mvn/datasets/utils.py:45-50, 55-56, 67-68)
 * happen where the stem conv gathers its taps: no fp32 image is written or read (0.79 MB each way per 256x256 frame; 403 MB at 512 frames,
 * twice that for a flip-test pair).  The stem runs the uint8 form of the kernel the float route would pick at the same shape, batch and
 * dtype (kernel names: the float kernel's with a ",u8" tag); every result bit equals capf_preprocess + the float entry.
 *   images_bgr_u8 [Bsrc,H,W,3] uint8, BGR in memory, any alignment; mean[3] / std3[3] HOST floats in RGB order (std3 == NULL: mean only, CPN);
 *   mode: capf_preprocess's -- 0 as is, 1 every frame mirrored, 2 flip test: engine frame f < Bsrc is source frame f, frame Bsrc + f its
 *   mirror.  `batch` counts ENGINE frames: Bsrc in modes 0 / 1, 2 * Bsrc in mode 2 (an odd batch: CAPF_ERR_INVALID).  A mode outside
 *   0 / 1 / 2: CAPF_ERR_INVALID.  Every check of the float entries applies.  k2d / kcrop_inout / out / drop_masks: as in capf_forward /
 *   capf_forward_train, [batch, ...] -- already mirrored / stacked (capf_preprocess_points).  capf_backward after capf_forward_train_u8
 *   works unchanged: nothing in the backward reads the image.
 * capf_preprocess_points: the keypoint / ground-truth half of capf_preprocess alone (one launch, the same bits).
 * capf_input_rule_host: the normalisation rule on the host -- out[i] = ((float)u[i] * (1.0f / 255.0f) - mean[channel]) (/ std3[channel]),
 *   every step one rounded fp32 operation; the expression the device kernels evaluate (csrc/pixel_rule.h).  channel: RGB index 0..2.
 * capf_op_conv_u8: the stem conv alone (ks x ks, padding ks / 2, folded BatchNorm, optional ReLU; no residual) from a uint8 image:
 *   w_packed / bias from capf_op_pack_conv (Cin = 3), y [frames,Ho,Wo,Cout] of out_dtype CAPF_F32 / CAPF_BF16 / CAPF_F16, frames = Bsrc
 *   (modes 0 / 1) or 2 * Bsrc (mode 2) -- through the dispatch of the plan's stem op.  capf_op_conv_u8_kernel_name names the kernel it
 *   launches, capf_op_conv_stem_kernel_name the one capf_op_conv / capf_op_conv_16 launch for the float image at B frames ("" where the
 *   arguments are invalid).
 * The accounting entries (capf_op_bytes, capf_forward_stats, the roofline figures) keep describing the float-image route.               */
int capf_forward_u8(capf_handle* h, void* stream, const uint8_t* images_bgr_u8, const float mean[3], const float* std3, int mode,
                    const float* k2d, float* kcrop_inout, int batch, float* out);
int capf_backbone_forward_u8(capf_handle* h, void* stream, const uint8_t* images_bgr_u8, const float mean[3], const float* std3, int mode,
                             int batch);
int capf_forward_train_u8(capf_handle* h, void* stream, const uint8_t* images_bgr_u8, const float mean[3], const float* std3, int mode,
                          const float* k2d, float* kcrop_inout, int batch, float* out, const float* drop_masks);
int capf_preprocess_points(void* stream, int batch, int mode, const float* gt_in, float* gt_out, const float* k2d_in, float* k2d_out,
                           const float* kcrop_in, float* kcrop_out);
int capf_input_rule_host(const uint8_t* u, int n, int channel, const float mean[3], const float* std3, float* out);
int capf_op_conv_u8(void* stream, const uint8_t* images_bgr_u8, const float* w_packed, const float* bias, void* y_nhwc, int Bsrc, int mode,
                    int H, int W, int Cout, int ks, int stride, int act, const float mean[3], const float* std3, int out_dtype);
const char* capf_op_conv_u8_kernel_name(int Bsrc, int mode, int H, int W, int Cout, int ks, int stride, int out_dtype);
const char* capf_op_conv_stem_kernel_name(int B, int H, int W, int Cout, int ks, int stride, int out_dtype);
/* capf_fliptest_fuse_swap: the same fusion for any skeleton -- ContextPose_mpi/run_3dhp.py:169-180 (input_augmentation: x of the mirrored
 *   prediction negated, joints_left + joints_right swapped, mean of the two) where capf_fliptest_fuse hard-codes the H36M table.
 *   pred2 [2,batch,1,joints,3] -> out [batch,1,joints,3]; swap: HOST int32[joints], swap[j] = the joint of the mirrored prediction that
 *   lands on joint j, a permutation that is its own inverse (3DHP: 2 <-> 5, 3 <-> 6, 4 <-> 7, 8 <-> 11, 9 <-> 12, 10 <-> 13).  The table
 *   travels in the kernel arguments (no device allocation); joints <= 32.  capf_fliptest_fuse is this entry with the H36M table (same
 *   bits).  Anything else -- out of range, not involutive -- returns CAPF_ERR_INVALID.                                                   */
int capf_fliptest_fuse_swap(void* stream, const float* pred2, int batch, int joints, const int32_t* swap, float* out);

/* ---- N2, second half: evaluation metrics over gathered predictions (train.py:381-436) -----------------
 * capf_pose_errors: per pose i of pred / gt [n, joints, 3] (joints <= 32), err[i] = {e_MPJPE, e_P_MPJPE, e_N_MPJPE,
 *   e_velocity}, each the mean over joints:  MPJPE loss.py:16-22;  P_MPJPE loss.py:25-68 (similarity Procrustes; the
 *   host numpy SVD of :48-60 is replaced by Horn's quaternion closed form, fp64 Jacobi per thread);  N_MPJPE
 *   loss.py:71-84;  velocity = |(pred_i - pred_prev) - (gt_i - gt_prev)| with prev = prev[i] (the previous pose of the
 *   same evaluated subset, i.e. np.diff over the masked rows, loss.py:87-101); prev == NULL means i-1; prev[i] < 0: 0.
 *   A pose that has no such figure gets NaN in that column alone, its other columns and every other pose unaffected: e_P_MPJPE where
 *   all predicted (or all ground-truth) joints are one point (normX normY = 0; the reference's numpy SVD raises there), e_N_MPJPE where
 *   the prediction is all zero.  joints > 32: CAPF_ERR_UNSUPPORTED; joints <= 0 or n <= 0: CAPF_ERR_INVALID; nothing is launched.
 * capf_segment_sums: per-action aggregation of evaluate_using_pred (datasets/human36m.py:358-417): sums[a] =
 *   {sum e_MPJPE, sum e_P_MPJPE, sum e_N_MPJPE, sum e_velocity} over poses with segment[i] == a (fp64, fixed order:
 *   deterministic), counts[a] = {poses, poses with a predecessor}.  segment == NULL with n_segments == 1: all poses.
 *   The reference's numbers are then MPJPE_a = sums[a][0]/counts[a][0], MPJVE_a = sums[a][3]/counts[a][1], ...
 * capf_keypoints_loss: KeypointsMSELoss (mode 0) / KeypointsMSESmoothLoss (1, `threshold`) / KeypointsMAELoss (2),
 *   loss.py:104-137: pred / gt [rows, dim], validity [rows] (the reference's [...,1] mask); writes the scalar loss and,
 *   if dpred != NULL, dloss/dpred.                                                                              */
int capf_pose_errors(void* stream, const float* pred, const float* gt, int n, int joints, const int32_t* prev, float* err);
int capf_segment_sums(void* stream, const float* err, const int32_t* segment, const int32_t* prev, int n, int n_segments,
                      double* sums, int32_t* counts);
int capf_keypoints_loss(void* stream, int mode, const float* pred, const float* gt, const float* validity, int rows, int dim,
                        float threshold, float* loss, float* dpred);
/* ---- the remaining pose losses of ContextPose/mvn/models/loss.py, with gradients (csrc/pose_losses.hip).  Additive inside revision 12.
 * Every entry enqueues on `stream`, allocates nothing, never synchronises, and adds in fixed orders without atomics: the same bits on
 * every call.  All sums are fp64 from the fp32 inputs; every output element is one fp32 store of its fp64 value.  grad_scale multiplies
 * the gradients only (capf_mpjpe's rule); an output gradient pointer that is NULL is not written, and the loss bits do not depend on it.
 *
 * capf_keypoints_l2_loss: KeypointsL2Loss, loss.py:140-147.  pred / gt [rows, dim] (dim >= 1), validity [rows] (the reference's [B, J, 1] mask):
 *     loss = sum_r sqrt(v_r * sum_c (gt - pred)^2) / max(1, sum_r v_r)
 *     dpred[r, c] = grad_scale * v_r (pred - gt) / (sqrt(v_r d2_r) * max(1, sum v)),  and EXACTLY 0 where that square root is 0
 *   -- capf_mpjpe's rule at zero distance.  It covers the masked row (v_r = 0) and the exact hit (pred == gt), at both of which the
 *   reference's autograd returns NaN (sqrt'(0) * 0), so a mask that holds zeros cannot be trained through there.  dloss/dgt = -dpred; the
 *   mask gets no gradient.  One block (training batches: at most 512 x 17 rows; any row count works).
 *
 * capf_limb_length_errors: LimbLengthError, loss.py:181-201, per pose.  pred / gt [n, joints, 3], joints <= 32; limbs: HOST int32
 *   [n_limbs, 2], 1 <= n_limbs <= 64, pairs (a_l, b_l) of joints.  The table travels in the kernel's arguments like
 *   capf_fliptest_fuse_swap's (no upload; the array may be reused as soon as the call returns) and is checked HERE: an index outside
 *   [0, joints) returns CAPF_ERR_INVALID and nothing is launched.  a_l == b_l and a repeated limb are legal.
 *     err[i, l] = | |pred[i, a_l] - pred[i, b_l]| - |gt[i, a_l] - gt[i, b_l]| |                        (err: [n, n_limbs])
 *     dpred[i] [joints, 3] = grad_scale * d(sum_l err[i, l]) / dpred[i]: per joint the sum, in limb order, over the limbs that touch it of
 *     +-sign(|pred limb| - |gt limb|) (pred[a_l] - pred[b_l]) / |pred limb|.  sign(0) = 0 (equal lengths), a predicted limb of length 0
 *     contributes 0 (no direction to move along), a_l == b_l contributes 0.  Every element of dpred is written (joints that no limb
 *     touches: 0).  The gradient with respect to gt is the same call with pred and gt exchanged.  One pose per thread.
 * capf_limb_length_sums: sums[s, l] fp64 = sum of err[i, l] over the poses with segment[i] == s, counts[s] int64 = those poses.
 *   segment: device int32 [n], or NULL with n_segments == 1 (all poses); ids outside [0, n_segments) are counted nowhere.  One block per
 *   (segment, limb): thread t of 256 adds its poses t, t + 256, ... in order, then a fixed tree.  The reference's figure is
 *   sum_l (sums[0, l] / n) / n_limbs.
 *
 * capf_uncertainty_loss: UNCERTAINTY, loss.py:7-13.  pred / gt [rows, dim]; sigmas: HOST array of n_sigmas (1..8) device pointers,
 *   sigma_widths: HOST int32 [n_sigmas], sigma k is [rows, sigma_widths[k]] with width dim or 1 (broadcast over the row), anything else
 *   CAPF_ERR_INVALID.  With s = sigma + 1e-6 (formed in fp64), u = (pred - gt) / s:
 *     loss = sum_k ( mean_r |u_k[r, :]|_2 + 0.01 * mean over sigma_k's own elements of log s )
 *   dpred (or NULL) [rows, dim]; dloss/dgt = -dpred.  dsigmas: NULL, or a HOST array of n_sigmas device pointers, each NULL or sigma k's
 *   own shape (the [rows, 1] form is summed over the row inside the thread).  The norm term contributes 0 to every gradient where
 *   |u_k[r, :]| is 0 (whatever torch.norm's backward does at 0 in the caller's torch version).  s <= 0 is not clamped: the loss is NaN, as the reference's log gives, and so are the row's
 *   dpred and that sigma's gradient in that row -- the guarded optimizer step (capf_adamw_step_guarded) is what catches it.  One block.
 * Refused before anything is launched (CAPF_ERR_INVALID): a NULL input or loss / err / sums / counts pointer, rows, n, dim, joints or
 * n_segments <= 0, n_limbs outside 1..64, n_sigmas outside 1..8, segment == NULL with n_segments != 1; joints > 32: CAPF_ERR_UNSUPPORTED.
 * Cost (MI355X, tools/bench_losses.py): EXPERIMENTS.md R39.1.                                                                               */
int capf_keypoints_l2_loss(void* stream, const float* pred, const float* gt, const float* validity, int rows, int dim, float* loss,
                           float* dpred, float grad_scale);
int capf_limb_length_errors(void* stream, const float* pred, const float* gt, int n, int joints, const int32_t* limbs, int n_limbs,
                            float* err, float* dpred, float grad_scale);
int capf_limb_length_sums(void* stream, const float* err, const int32_t* segment, int n, int n_limbs, int n_segments, double* sums,
                          int64_t* counts);
int capf_uncertainty_loss(void* stream, const float* pred, const float* gt, int rows, int dim, const float* const* sigmas,
                          const int32_t* sigma_widths, int n_sigmas, float* loss, float* dpred, float* const* dsigmas, float grad_scale);

/* ---- 2-D keypoint head: final_layer + heatmap decode on the highest-resolution context map --------------------------------------------
 * What an HRNet COCO checkpoint's final_layer (nn.Conv2d(C0, 17, 1), pose_hrnet.py:497-501, commented out in the reference) computes on
 * y_list[0] = feat0, followed by the decode of its heatmaps, as ONE pass over the map (csrc/kp_head.hip): the producer of the 2-D keypoints that
 * capf_forward takes and the consumer of capf_backward_points' dk2d / dref.  Stand-alone entries on device pointers (capf_tensor("feat0")
 * serves the map of a handle; any other NHWC map of the same layout does too).  Additive inside revision 12.
 *   map_nhwc [B, H, W, C] of map_dtype (capf_dtype: fp32, bf16 or fp16; a 16-bit value is widened exactly and everything after is fp32), 16-byte
 *   aligned (8 for a 16-bit map); weight [J, C] fp32 (final_layer.weight [J, C, 1, 1]); bias [J] fp32 or NULL.  1 <= J <= 32, C % 4 == 0,
 *   4 <= C <= 512, H, W >= 1, H * W <= 2^24.
 * Logits: ONE fixed fp32 expression on the vector pipe (no matrix pipe, no block scales: a frame's result is bit-identical whatever else is in
 *   the batch and on every run, handle and scratch buffer),
 *       z[b, j, y, x] = bias[j];  for c = 0 .. C - 1 ascending:  z = fma(map[b, y, x, c], weight[j, c], z).
 *   The heatmaps are never written unless `heat` [B, J, H, W] (the fp32 logits the decode used, bit for bit) is given.
 * mode 0, argmax -- the rule HRNet checkpoints are evaluated with: idx = the FIRST maximum of z[b, j] in row-major order (ties go to the smallest
 *   index), score = z[idx], px = idx % W, py = idx / W, (x, y) = (px, py); if 1 < px < W - 1 and 1 < py < H - 1:
 *   x += 0.25 sign(z[py][px + 1] - z[py][px - 1]), y += 0.25 sign(z[py + 1][px] - z[py - 1][px]), sign(0) = 0; then, if score <= 0, (x, y) = (0, 0).
 * mode 1, integral (soft-argmax): p = softmax(beta z[b, j]) over the H * W pixels with the maximum subtracted, x = sum p col, y = sum p row,
 *   score = max z.  beta > 0 and finite (checked in both modes; pass 1 in mode 0).
 * NaN: if any logit of a (frame, joint) is NaN, its keypoint (both coordinate systems) and its score are NaN, in both modes; other joints and
 *   frames are untouched.
 * Outputs: kcrop[b, j] = (sx x + ox, sy y + oy) with decode = {sx, ox, sy, oy} (HRNet's convention: sx = W_img / W, sy = H_img / H, offsets 0;
 *   product rounded, then the sum); k2d[b, j] = A_b (kcrop_x, kcrop_y, 1) = ((A00 kx + A01 ky) + A02, (A10 kx + A11 ky) + A12) for
 *   to_image [B, 2, 3] fp32, the caller's composition of the inverse crop affine and normalize_screen_coordinates (common/camera.py:14-18);
 *   to_image == NULL: k2d is not written.  score [B, J] and heat are optional (NULL).
 * Summation orders (integral): pixels are numbered row-major and cut into tiles of 256 and slabs of ceil(tiles / 64) tiles -- a function of H * W
 *   alone.  Inside a slab 8 lanes share a joint: lane l visits pixels l, l + 8, ... of each tile, tiles ascending, with an online maximum m and
 *   sums of e = exp(beta z - m), e col, e row (rescaled by exp(m_old - m_new) when m grows); lanes are merged in ascending l, slabs in ascending
 *   order by a SECOND launch (no atomics, no signalling between workgroups), each merge as s = s1 exp(m1 - M) + s2 exp(m2 - M), M = max(m1, m2).
 *   The argmax's neighbours are recomputed from the map with the expression above (the only values read twice).
 * scratch: capf_kp_head_scratch_bytes(B, H, W, C, J, backward) bytes of device memory, 4-byte aligned (0: a shape the kernels do not take).
 * capf_kp_head_backward (mode 1 and an fp32 map only; mode 0 or a 16-bit map: CAPF_ERR_UNSUPPORTED): for dkcrop / dk2d [B, J, 2] (either may
 *   be NULL, not both; dk2d needs to_image), g = (sx, sy) * (dkcrop + A_b[:, :2]^T dk2d); logits and softmax statistics are recomputed (the
 *   forward saves nothing); dz_i = beta p_i (g_x (col_i - x) + g_y (row_i - y));
 *       dweight [J, C] = sum over frames and pixels of dz X: per block (a frame's eighth of the tiles) pixels ascending inside a tile and tiles
 *           ascending, then a second launch adds the blocks' partials -- part q of 16 takes blocks q, q + 16, ... ascending, parts ascending;
 *       dbias [J] is written as EXACT ZEROS: softmax is invariant under a shift of its logits, so the true gradient is 0, and a rounding-level
 *           residue would be normalised by AdamW into steps of size lr;
 *       dmap [B, H, W, C] (optional, 16-byte aligned) = sum_j dz Wt[j, c], joints ascending, each element by one thread: accumulate = 1 adds it
 *           to what is there (capf_backward_points' dfeat_nhwc[0]), accumulate = 0 overwrites.
 * Refusals, all before anything is launched (no device needed): a NULL map / weight / decode / scratch / kcrop (forward) / dweight / dbias
 *   (backward), both gradients NULL, dk2d without to_image, B, J, C, H or W out of range, beta <= 0 or not finite, an unknown mode or dtype,
 *   accumulate not 0 / 1, a misaligned map / dmap, scratch_bytes too small: CAPF_ERR_INVALID.
 * Cost (MI355X, HRNet-32 fp32 256 x 256, feat0 64 x 64 x 32, medians of 20 around the host call, tools/bench_kp_head.py, EXPERIMENTS.md R24.1): forward
 *   0.096 (argmax) / 0.076 ms (integral) at batch 64 and 0.318 / 0.313 ms at batch 512, against capf_backbone_forward's 5.89 / 43.4 ms and a one-read
 *   floor of 0.008 / 0.067 ms (the slab kernel alone: 36 - 48 / 250 - 275 us; bound by instruction issue per 256-pixel tile, not by memory); backward
 *   0.169 ms (dweight) / 0.233 ms (with dmap) at batch 64, 1.02 / 1.53 ms at batch 512; fp16 HRNet-48 map at batch 256: 0.194 / 0.209 ms. */
size_t capf_kp_head_scratch_bytes(int B, int H, int W, int C, int J, int backward);
int capf_kp_head_forward(void* stream, const void* map_nhwc, int map_dtype, const float* weight, const float* bias, int B, int H, int W, int C,
                         int J, int mode, float beta, const float decode[4], const float* to_image, float* kcrop, float* k2d, float* score,
                         float* heat, void* scratch, size_t scratch_bytes);
int capf_kp_head_backward(void* stream, const float* dkcrop, const float* dk2d, const void* map_nhwc, int map_dtype, const float* weight,
                          const float* bias, int B, int H, int W, int C, int J, int mode, float beta, const float decode[4],
                          const float* to_image, float* dweight, float* dbias, float* dmap, int accumulate, void* scratch, size_t scratch_bytes);
/* ---- 2-D keypoint head on a flip-test pair: the heatmaps of a crop and of its flipped-back mirror averaged, then ONE decode -------------------
 * HRNet's own flip test (lib/core/function.py validate: FLIP_TEST, flip_back, SHIFT_HEATMAP) on the maps capf_backbone_forward(_u8) leaves for
 * the 2 * Bsrc engine frames of mode 2: map_nhwc [2 * Bsrc, H, W, C], frame b < Bsrc the source frame, frame Bsrc + b its mirror.  Dtypes, shape
 * limits (on Bsrc, H, W, C, J), alignment, weight, bias, mode, beta, decode: capf_kp_head_forward's.  Forward only.  Additive inside revision 12.
 * Fused logit of source frame b, joint j, pixel (y, x), z being capf_kp_head_forward's chain on the 2 * Bsrc-frame map, bit for bit:
 *       zo = z[b, j, y, x]
 *       xs = (shift && x >= 1) ? x - 1 : x        (SHIFT_HEATMAP: flipped[:, :, :, 1:] = flipped[:, :, :, :-1]; column 0 keeps its own value)
 *       zm = z[Bsrc + b, swap[j], y, W - 1 - xs]  (flip_back: mirrored in x, left / right joints exchanged)
 *       zf = 0.5f * (zo + zm)                     (the fp32 sum rounded once, then halved)
 *   swap: HOST int32[J], a permutation that is its own inverse (capf_fliptest_fuse_swap's rule and tables); it travels in the kernel arguments.
 *   shift: 0 / 1.  The fused heatmaps are never written unless `heat` [Bsrc, J, H, W] (the zf the decode used, bit for bit) is given.
 * Decode of zf: capf_kp_head_forward's, rule for rule -- argmax: first maximum in row-major order, the quarter shift (its four neighbours are
 *   recomputed from BOTH frames with the expression above), score <= 0 -> (0, 0); integral: the same tiles of 256, slabs, 8 lanes per joint,
 *   online maximum and sums, merge orders and second launch (the summation orders are unchanged).  No atomics, no signalling between workgroups.
 * NaN: the keypoint (both coordinate systems, both sets) and the score of (b, j) are NaN if any logit of (b, j) OR of (Bsrc + b, swap[j]) is NaN
 *   -- also one in the mirror's column 0, which no pixel reads under shift = 1.  Other joints and frames are untouched.
 * A source frame's result bits depend on frames b and Bsrc + b alone: not on Bsrc, the frame's position, the run or the scratch buffer.
 * Outputs: with kcrop / k2d / score [Bsrc, J(, 2)] the decode -> decode[4] -> to_image [Bsrc, 2, 3] arithmetic of capf_kp_head_forward on zf, the
 *   stacks capf_forward takes for the 2 * Bsrc frames (no further launch):
 *       kcrop2[0, b, j] = kcrop[b, j]      kcrop2[1, b, j] = ((mirror_width - kcrop[b, swap[j]].x) - 1, kcrop[b, swap[j]].y)   (two rounded fp32
 *       k2d2 [0, b, j] = k2d[b, j]         k2d2 [1, b, j] = (-k2d[b, swap[j]].x, k2d[b, swap[j]].y)                            subtractions)
 *   kcrop2 [2, Bsrc, J, 2]; k2d2 [2, Bsrc, J, 2] or NULL (needs to_image); score [Bsrc, J] or NULL.  With J = 17, the H36M table and
 *   mirror_width = 192 (the reference's constant, datasets/utils.py:76) the stacks are capf_preprocess_points(mode = 2) of (k2d, kcrop) bit for bit.
 * scratch: capf_kp_head_pair_scratch_bytes(Bsrc, H, W, C, J) bytes, 4-byte aligned (0: a shape the kernels do not take).
 * Refusals, all before anything is launched (no device needed), CAPF_ERR_INVALID: a NULL map / weight / decode / swap / kcrop2 / scratch, k2d2
 *   without to_image, Bsrc, J, C, H or W out of range, beta <= 0 or not finite, mirror_width not finite, shift outside 0 / 1, an unknown mode or
 *   dtype, a misaligned map, scratch_bytes too small, a swap entry outside [0, J) or a table that is not its own inverse.  (H * W > 2^24, or a
 *   grid beyond 2^31 blocks: CAPF_ERR_UNSUPPORTED, as capf_kp_head_forward.)
 * Cost (MI355X, medians of 20 around the host call, tools/bench_kp_head.py --pair, EXPERIMENTS.md R28.1), against capf_kp_head_forward on the
 *   SAME 2 * Bsrc-frame map (the same bytes read, the same FMAs, half the (frame, joint) items):
 *   HRNet-32 fp32, feat0 64 x 64 x 32: Bsrc 32 -- 0.074 (argmax) / 0.071 ms (integral) against 0.073 / 0.071 ms (ratio 1.02 / 1.00); Bsrc 256 -- 0.276 /
 *   0.284 ms against 0.301 / 0.300 ms (0.92 / 0.95); fp16 HRNet-48 map, Bsrc 128 -- 0.197 / 0.191 ms against 0.186 / 0.206 ms (1.05 / 0.93): the same cost
 *   within 5 % either way, slower in two of the six.  CA_PF.forward_detect_flip_test against detect + preprocess_points + forward_flip_test: 6.86
 *   against 10.75 ms (Bsrc 32), 46.1 against 68.2 ms (Bsrc 256), 19.2 against 27.5 ms (fp16 HRNet-48, Bsrc 128). */
size_t capf_kp_head_pair_scratch_bytes(int Bsrc, int H, int W, int C, int J);
int capf_kp_head_forward_pair(void* stream, const void* map_nhwc, int map_dtype, const float* weight, const float* bias, int Bsrc, int H, int W,
                              int C, int J, int mode, float beta, const int32_t* swap, int shift, const float decode[4], const float* to_image,
                              float mirror_width, float* kcrop2, float* k2d2, float* score, float* heat, void* scratch, size_t scratch_bytes);
/* ---- heatmap supervision of the 2-D keypoint head: MSE against Gaussian targets, loss and parameter gradients in one entry -------------------
 * The loss heatmap heads are trained with -- upstream HRNet's JointsMSELoss / JointsOHKMMSELoss on generate_target's Gaussians; the reduction
 * of cpn/train.py:85-93, 124-127 (ohkm(refine_loss, 8)) -- fused with final_layer's 1x1 conv: neither the logits nor the targets reach memory
 * (csrc/kp_head.hip).  It is what trains an "argmax" head, and the only path on which final_layer.bias receives a gradient.  Stand-alone entry
 * on device pointers; additive inside revision 12.  map, weight, bias, shape limits, alignment, dtypes: capf_kp_head_forward's.
 * Logits: z[b, j, y, x] is capf_kp_head_forward's chain, bit for bit (its `heat` output).
 * Target of (b, j), (kx, ky) = kcrop_gt[b, j] in crop pixels, decode = {sx, ox, sy, oy} as in the forward (heatmap -> crop pixels):
 *       cx = (kx - ox) / sx, cy = (ky - oy) / sy      (fp32, the difference rounded, then the quotient)
 *       mu = (int)(c + 0.5f)                          (the fp32 sum truncated toward zero, Python's int(): c = -0.7 gives 0, not -1)
 *       R  = (int)ceilf(3.f * sigma)
 *       t(y, x) = exp(-((x - mu_x)^2 + (y - mu_y)^2) / (2 sigma^2)) where |x - mu_x| <= R and |y - mu_y| <= R, 0 elsewhere
 *           (in DOUBLE, as e[|x - mu_x|] e[|y - mu_y|] with e[k] = exp(-k^2 / (2 sigma^2)) and sigma the fp32 value widened; z - t is formed
 *           in double and rounded ONCE to fp32, so its error is half an ulp of z - t even where z and t nearly cancel -- an fp32 expf would
 *           leave an error relative to t, which no bound relative to the terms (z - t)^2 covers)
 *   w_bj = target_weight[b, j] (NULL: 1), forced to 0 when the window lies wholly outside the map (mu_x - R >= W, mu_y - R >= H, mu_x + R < 0 or
 *   mu_y + R < 0), when a coordinate of c is not finite, or when |c| > 2^20.
 * Per item: l_bj = scale w_bj^2 (1 / (H W)) sum_pix (z - t)^2.  HRNet's criterion multiplies prediction and target by w (hence w^2) and has
 *   scale = 0.5; scale = 1 with w in {0, 1} is cpn/train.py:124-126.
 * reduction 0, mean: loss = (1 / (B J)) sum_bj l_bj.
 * reduction 1, OHKM: loss = (1 / B) sum_b (1 / topk) sum_{j in top_b} l_bj; top_b holds the min(topk, J) largest l_bj of frame b, a NaN ranking
 *   first and ties going to the smaller joint index; the divisor stays topk (cpn/train.py:85-93); only selected items receive gradient.
 * Outputs: loss [1]; joint_loss [B, J] (l_bj, optional).  Gradients of `loss`, each optional (all NULL: the loss alone):
 *       g_bj = 2 scale w_bj^2 sel_bj / (H W norm)  (norm = B J or B topk; sel = 1 under reduction 0),  dz = g_bj (z - t)
 *       dweight [J, C] = sum_{b, pix} dz X      dbias [J] = sum_{b, pix} dz  (a real gradient here, unlike capf_kp_head_backward's zeros)
 *       dmap [B, H, W, C] fp32, 16-byte aligned = sum_j dz weight[j, c], joints ascending, each element by one thread; accumulate = 1 adds it to
 *           what is there (capf_backward_points' dfeat_nhwc[0]), 0 overwrites.  It needs an fp32 map: a 16-bit one is CAPF_ERR_UNSUPPORTED.
 * Summation orders (no atomics, no signalling between workgroups): pixels are numbered row-major and cut into capf_kp_head_forward's tiles of
 *   256; a block owns a frame's eighth of the tiles, ceil(tiles / 8) consecutive ones (capf_kp_head_backward's cut; a function of H * W alone).
 *   sum (z - t)^2 of (b, j): 8 lanes share the joint, lane l adds (by fma) pixels l, l + 8, ... of each tile, tiles ascending; the lanes are added
 *   in ascending l; a SECOND launch adds the blocks ascending, forms l_bj, ranks the joints of a frame and adds the selected l_bj of a frame in
 *   ascending j; the last launch adds the frames -- part q of 16 takes frames q, q + 16, ... ascending, the parts ascending -- and divides by
 *   norm.  dweight, dbias: per block and tile sum_pix (z - t) X (pixels ascending, by fma; X = 1 for dbias), times g_bj, added over the
 *   block's tiles ascending; the last launch adds the blocks' partials -- part q of 16 takes blocks q, q + 16, ... ascending, parts ascending.
 *   joint_loss[b, j] bits depend on frame b alone: not on B, the frame's position, the run or the scratch buffer.
 * Passes: reduction 0 knows g up front -- loss and gradients come from ONE pass over the map (3 launches); OHKM needs every l_b. before any dz:
 *   a loss pass, the selection, a gradient pass that recomputes the logits (4 launches).
 * NaN: a NaN logit makes that l_bj and the loss NaN (under OHKM it ranks first); other items' joint_loss are untouched.  An item with
 *   w_bj = 0, and under OHKM an item that is not selected, contributes EXACT zeros to every output, whatever its logits (0 is not multiplied
 *   with them).
 * scratch: capf_kp_heatmap_loss_scratch_bytes(B, H, W, C, J, reduction) bytes of device memory, 4-byte aligned (0: a shape the kernels do not
 *   take, or an unknown reduction).
 * Refusals, all before anything is launched (no device needed), CAPF_ERR_INVALID: a NULL map / weight / kcrop_gt / decode / loss / scratch,
 *   B, J, C, H or W out of range, sx or sy zero or not finite, sigma <= 0 or not finite or R > 64, an unknown reduction or dtype, topk < 1,
 *   scale not finite, accumulate not 0 / 1, a misaligned map / dmap, scratch_bytes too small.
 * Cost (MI355X, feat0 64 x 64 x 32 of HRNet-32 fp32, sigma 2, medians of 20 around the host call, tools/bench_kp_head.py --loss, EXPERIMENTS.md
 *   R33.1), mean / OHKM, against capf_kp_head_backward re-timed on the same map in the same session and a one-read floor of bytes / 8 TB/s:
 *   batch 64 (floor 0.004 ms) -- the loss alone 0.053 / 0.054 ms, with dweight and dbias 0.120 / 0.150 ms against the backward's 0.155 ms
 *   (ratio 0.77 / 0.97), with dmap 0.179 / 0.212 ms against 0.214 ms (0.84 / 0.99); batch 512 (floor 0.034 ms) -- 0.171 / 0.171 ms alone,
 *   0.654 / 0.782 ms against 0.999 ms (0.66 / 0.78), with dmap 1.095 / 1.226 ms against 1.450 ms (0.76 / 0.85); fp16 HRNet-48 map, batch 256
 *   (floor 0.013 ms; the backward takes no 16-bit map) -- 0.119 / 0.120 ms alone, 0.405 / 0.507 ms with dweight and dbias, against
 *   capf_kp_head_forward's 0.196 ms (2.07 / 2.59).  5 - 50 x the floor: not memory-bound, like the head. */
size_t capf_kp_heatmap_loss_scratch_bytes(int B, int H, int W, int C, int J, int reduction);
int capf_kp_heatmap_loss(void* stream, const void* map_nhwc, int map_dtype, const float* weight, const float* bias, int B, int H, int W, int C,
                         int J, const float* kcrop_gt, const float* target_weight, const float decode[4], float sigma, int reduction, int topk,
                         float scale, float* loss, float* joint_loss, float* dweight, float* dbias, float* dmap, int accumulate, void* scratch,
                         size_t scratch_bytes);
/* ---- CPN's own heatmap decode: two peaks of the blurred map, a quarter pixel from the first towards the second ------------------------------
 * What cpn/test.py:79-108 does with the heatmaps of refine_net.final_predict (the named tensor "heat" of a CAPF_PLAN_CPN_PREDICT handle; any
 * other NHWC map of that layout does too), as ONE launch: one workgroup per (frame, joint), the planes in LDS, no scratch, no atomics
 * (csrc/cpn_decode.hip).  Stand-alone entry on device pointers.  Additive inside revision 12.
 *   heat_nhwc [B, H, W, C] of heat_dtype (capf_dtype: fp32, bf16 or fp16; a 16-bit value is widened exactly), 16-byte aligned (8 for a 16-bit map);
 *   joint j is channel j.  1 <= J <= C <= 32, H, W >= 1, and capf_cpn_decode_lds_bytes(H, W) = 256 + 8 (H + 20)(W + 20) + 4 H W <= 160 KiB, the
 *   LDS of a compute unit: 64 x 48 (this plan) and 96 x 72 (upstream CPN at 384 x 288) fit; what does not: CAPF_ERR_UNSUPPORTED.
 * Per (b, j), z = the H x W heatmap as fp32:
 *   M  = max z;  r0 = z / 255 + 0.5 (fp32, both operations rounded);  n = z / M (fp32, IEEE division)
 *   P  = (H + 20) x (W + 20) float64, zero but for P[10 + y][10 + x] = n[y][x]
 *   g  = the 21 taps of capf_cpn_decode_taps: g_i = e_i / sum(e), e_i = exp(-(i - 10)^2 / (2 * 3.5^2)) in double on the host (3.5 is OpenCV's
 *        sigma for ksize 21, sigma 0: 0.3 ((21 - 1) / 2 - 1) + 0.8); bit-symmetric (g_i == g_{20 - i}) and summing to 1 within 2^-52
 *   D  = the separable blur of P, rows pass first, reflect-101 borders ON P (r(t) = -t for t < 0, 2 (n - 1) - t for t >= n), float64, in ONE
 *        summation order, every step an fma rounded once:
 *            R[y][x] = acc after  acc = +0;  for i = 0 .. 20 ascending:  acc = fma(g_i, P[y][r(x + i - 10)], acc)        (all rows of P)
 *            D[y][x] = acc after  acc = +0;  for i = 0 .. 20 ascending:  acc = fma(g_i, R[r(y + i - 10)][x], acc)
 *   (y1, x1) = the FIRST maximum of D in row-major order;  D[y1][x1] = 0;  (y2, x2) = the first maximum again (the zeroed cell competes)
 *   x = x1 - 10, y = y1 - 10, px = x2 - x1, py = y2 - y1, ln = sqrt(px^2 + py^2) in double;  if ln > 1e-3: x += (0.25 px) / ln, y += (0.25 py) / ln
 *   x clamped to [0, W - 1], y to [0, H - 1];  score = r0[round(y)][round(x)] (the fraction is 0 or at most 0.25 either way: never a half)
 * Outputs: x and y are converted to fp32 first; kcrop[b, j] = (sx x + ox, sy y + oy) with decode = {sx, ox, sy, oy}, product rounded, then the sum
 *   (CPN's convention: sx = W_img / W, ox = sx / 2, the same in y -- (4 x + 2) / data_shape of cpn/test.py:106-107 for any crop whose heatmap is
 *   a quarter of it per axis, and for the 384 x 288 crops whose heatmap is still 64 x 48); k2d[b, j] = ((A00 kx + A01 ky) + A02, (A10 kx + A11 ky)
 *   + A12) for to_image [B, 2, 3] fp32, every operation rounded on its own, as capf_kp_head_forward states it; to_image == NULL: k2d is not
 *   written.  score [B, J] and blurred [B, J, H + 20, W + 20] float64 (D before the zeroing; 8-byte aligned) are optional (NULL).
 * Degenerate maps: M == 0, or any NaN / +-Inf among the H W values of (b, j): its keypoint (both coordinate systems), its score and its plane of
 *   `blurred` are NaN; every other joint and frame is untouched.  M < 0 follows the arithmetic literally, as the reference would (n = z / M is then
 *   >= 1 wherever z <= M: the "peaks" are the map's minima).  A quotient z / M that overflows (|M| subnormal) is outside the contract: a NaN or
 *   Inf of D never wins a comparison here, where numpy's argmax would take a NaN.
 * A (frame, joint)'s result bits depend on its H W values alone: not on B, J, C, its position, the run or the device buffer.
 * PARITY UNPINNED in the last bits of D: OpenCV is absent from the build machine, so nothing pins cv2.GaussianBlur's own summation order, its tap
 *   rounding or its vector width; D is bit-exact against the restatement above (tests/cpn_decode_oracle.py holds it within 44 x 2^-53 x blur(|P|),
 *   two passes of 21 fma), and the integer peaks and the direction of the shift do not depend on those bits whenever the peaks are separated by more than
 *   that -- which is what the tests establish (they count the cases that are not, and bound their share).
 * Refusals, all before anything is launched (no device needed): a NULL map / decode / kcrop, k2d without to_image, B, H, W, J or C out of range
 *   (J > C, C > 32), an unknown dtype, a misaligned map / kcrop / blurred: CAPF_ERR_INVALID; planes beyond the LDS: CAPF_ERR_UNSUPPORTED.
 * Cost (MI355X, medians of 20 around the host call, tools/bench_cpn_detect.py, EXPERIMENTS.md R29.1): 0.25 ms for 128 frames x 17 joints of a
 *   bf16 64 x 48 map, 0.19 ms for 64 frames of an fp32 one, against 7.2 / 5.8 ms of capf_backbone_forward under CAPF_PLAN_CPN_PREDICT (which the
 *   head itself makes 1.3 / 1.5 ms longer than the unflagged plan's 6.0 / 4.4 ms: the concat 0.31, the five convs 0.96 / 1.15 ms). */
void capf_cpn_decode_taps(double taps[21]);
size_t capf_cpn_decode_lds_bytes(int H, int W);       /* 0: H or W out of range */
int capf_cpn_decode(void* stream, const void* heat_nhwc, int heat_dtype, int B, int H, int W, int C, int J, const float decode[4],
                    const float* to_image, float* kcrop, float* k2d, float* score, double* blurred);
/* ---- CPN's decode on a flip-test pair: the heatmaps of a crop and of its mirror averaged, then ONE two-peak decode ----------------------------
 * CPN's own test-time flip (cpn/test.py:44-70, --flip defaults to True: the procedure that made the keypoints_2d_cpn the lifter was trained on)
 * on the heatmaps one backbone pass leaves for the 2 * Bsrc engine frames of capf_preprocess mode 2: heat_nhwc [2 * Bsrc, H, W, C], frame
 * b < Bsrc the source frame, frame Bsrc + b its mirror.  Dtypes, shape limits (on Bsrc, H, W, C, J), alignment, the LDS limit, decode, the taps:
 * capf_cpn_decode's.  ONE launch of the PAIR instantiation of the same kernel: one workgroup per (source frame, joint), the same LDS planes, no
 * scratch, no atomics, no second launch (csrc/cpn_decode.hip).  Forward only.  Additive inside revision 12.
 * Fused heatmap of source frame b, joint j, pixel (y, x), z being the 2 * Bsrc-frame map widened to fp32 (test.py:62-70 restated):
 *       zo = z[b,        y, x,         j]
 *       zm = z[Bsrc + b, y, W - 1 - x, swap[j]]   (cv2.flip(.., 1), then the symmetric joints exchanged; NO column shift -- HRNet's SHIFT_HEATMAP
 *                                                  is not CPN's)
 *       zf = 0.5f * (zo + zm)                     (the fp32 sum rounded once, then halved: numpy's `+=` then `/= 2` on float32)
 *   swap: HOST int32[J], a permutation that is its own inverse (capf_fliptest_fuse_swap's rule); it travels in the kernel arguments.  The H36M
 *   table serves a head whose channels feed the H36M lifter; upstream's cfg.symmetry for COCO-ordered channels is capf.lib.COCO_SWAP.
 * Decode of zf: capf_cpn_decode's, rule for rule and in the same summation order -- M = max zf, n = zf / M, the padded plane, the row pass, then
 *   the column pass, first and second maximum, quarter shift, clamp.  r0 = zf / 255 + 0.5 is taken from the FUSED map, as the reference takes it
 *   (r0 = single_map.copy() after the fold): the score at (round(y), round(x)) recomputes zf from both frames.  The result equals
 *   capf_cpn_decode on a map that holds zf, bit for bit, decided or not.
 * Degenerate maps: capf_cpn_decode's rule on zf -- any zf of (b, j) not finite (a NaN or +-Inf in either frame, a sum that overflows), or a fused
 *   maximum of 0 (zo = -zm everywhere): the keypoint of (b, j) in both coordinate systems and BOTH sets (slot swap[j] of set 1), its score and its
 *   plane of `blurred` are NaN; every other joint and frame is untouched.  A negative fused maximum follows the arithmetic.
 * A source frame's result bits depend on frames b and Bsrc + b alone: not on Bsrc, J, C, the frame's position, the run or the device buffer.
 * Outputs: with kcrop / k2d / score [Bsrc, J(, 2)] the decode[4] -> to_image [Bsrc, 2, 3] arithmetic of capf_cpn_decode on zf, the stacks
 *   capf_forward takes for the 2 * Bsrc frames (no further launch; swap is its own inverse, so workgroup (b, j) writes its own two slots):
 *       kcrop2[0, b, j] = kcrop[b, j]      kcrop2[1, b, swap[j]] = ((mirror_width - kcrop[b, j].x) - 1, kcrop[b, j].y)   (two rounded fp32 subtractions)
 *       k2d2 [0, b, j] = k2d[b, j]         k2d2 [1, b, swap[j]] = (-k2d[b, j].x, k2d[b, j].y)
 *   kcrop2 [2, Bsrc, J, 2]; k2d2 [2, Bsrc, J, 2] or NULL (needs to_image); score [Bsrc, J] or NULL.  With J = 17, the H36M table and
 *   mirror_width = 192 (the reference's constant, datasets/utils.py:76) the stacks are capf_preprocess_points(mode = 2) of (k2d, kcrop) bit for
 *   bit, and capf_kp_head_forward_pair's layout.  Optional (NULL): blurred [Bsrc, J, H + 20, W + 20] float64 (D of zf before the zeroing, 8-byte
 *   aligned) and fused [Bsrc, J, H, W] fp32 -- the zf the decode used, bit for bit (written for degenerate maps too).
 * PARITY UNPINNED in the last bits of D exactly as for capf_cpn_decode: nothing pins cv2.GaussianBlur's own summation order; the fold
 *   itself is exact arithmetic on two fp32 values and is pinned bit for bit (tests/cpn_flip_oracle.py, two restatements).
 * Refusals, all before anything is launched (no device needed), CAPF_ERR_INVALID: a NULL map / decode / swap / kcrop2, k2d2 without to_image,
 *   Bsrc, H, W, J or C out of range (J > C, C > 32), an unknown dtype, a misaligned map / kcrop2 / blurred / fused, mirror_width not finite, a swap
 *   entry outside [0, J) or a table that is not its own inverse; CAPF_ERR_UNSUPPORTED: planes beyond the LDS limit, a grid of 2^31 blocks or more.
 * Cost (MI355X, medians of 20 around the host call, two runs, tools/bench_cpn_detect.py --pair, EXPERIMENTS.md R30.1; 64 x 48 x 20 maps, 17 joints):
 *   fp32, Bsrc 32 -- 0.126 / 0.136 ms against capf_cpn_decode's 0.159 ms on the same 2 * Bsrc-frame map (twice the items) and 0.103 ms on Bsrc
 *   frames (the same items, half the map bytes); bf16, Bsrc 64 -- 0.180 / 0.165 ms against 0.239 and 0.145 ms.  SLOWER than the single decode at
 *   Bsrc by 14 - 31 % (the second strided gather of the load and the score), 14 - 30 % faster than decoding all 2 * Bsrc frames.
 *   CA_PF.forward_detect_cpn_flip against a backbone pass over the pair + the fold in torch + capf_cpn_decode + capf_preprocess_points +
 *   forward_flip_test: 7.2 against 13.0 ms (fp32, Bsrc 32), 5.7 against 9.8 ms (bf16, Bsrc 64) -- one backbone pass over the pair saved. */
int capf_cpn_decode_pair(void* stream, const void* heat_nhwc, int heat_dtype, int Bsrc, int H, int W, int C, int J, const int32_t* swap,
                         const float decode[4], const float* to_image, float mirror_width, float* kcrop2, float* k2d2, float* score,
                         double* blurred, float* fused);
/* capf_pck_counts: the MPI-INF-3DHP evaluation (ContextPose_mpi/3dhp_test/test_util, MATLAB: mpii_test_predictions_py.m,
 *   mpii_evaluate_errors.m, mpii_compute_3d_pck.m), which callers otherwise export to .mat files and run off the GPU; capf_pose_errors /
 *   capf_segment_sums serve H36M only.  Per pose i of pred / gt [n, joints, 3] (same unit; to_mm converts it to mm): gt made relative to
 *   joint `root` (mpii_test_predictions_py.m:46), pred's root joint taken as 0 (run_3dhp.py:118), per-joint error e = |pred - gt| x to_mm
 *   in fp64 (:50-51).  Outputs per segment s (segment[i], int32 [n]; NULL with n_segments == 1: all poses; ids outside [0, n_segments)
 *   are skipped): counts[s][j][31] int32 = poses with e < 5 t mm, t = 0..30 (strict <, mpii_compute_3d_pck.m:20, 30), mpjpe_sums[s][j]
 *   fp64 = sum of e in a fixed order (the same bits on every call), frames[s] int32 = poses.  n may be 0 (zeros out; segment may then
 *   be NULL).  PCK@150 / AUC per joint group and the MPJPE tables follow on the host from these integers
 *   (mvn/datasets/mpi_inf_3dhp.py::evaluate).                                                                                          */
int capf_pck_counts(void* stream, const float* pred, const float* gt, int n, int joints, int root, double to_mm, const int32_t* segment,
                    int n_segments, int32_t* counts, double* mpjpe_sums, int32_t* frames);
/* capf_pck2d_counts: the 2-D PCKh counts of evaluate2d / evaluate_2d_joint (ContextPose/mvn/datasets/human36m.py:438-479) and of the
 *   accuracy figure of CA_PF.keypoint_loss(return_accuracy=True).  pred / gt: device fp32 [n, joints, 2].
 *   Arithmetic, all fp64, every operation rounded on its own (no contraction; division and sqrt correctly rounded), so that a float64
 *   restatement gets the same numbers (tests/pck2d_oracle.py):  u = ((double)px - (double)gx) / (double)nx,  v likewise with ny,
 *   e = sqrt(u u + v v).  strict == 0: sample (i, j) is detected at threshold k iff e <= thresholds[k] -- the reference's rule
 *   `distance <= headsize * threshold`: the caller passes norm = NULL and thresholds already multiplied by headsize in double, the
 *   product the reference forms; strict == 1: iff e < thresholds[k].
 *   norm: device fp32 [n, 2] = per-pose (nx, ny), or NULL = (1, 1).  weight: device fp32 [n, joints], or NULL = every sample valid.
 *   thresholds: HOST doubles, n_thresholds of them (1..32); they travel in the kernel's arguments (no upload, no synchronisation; the
 *   array may be reused as soon as the call returns).  segment: device int32 [n], or NULL (with poses, n_segments must then be 1: all poses).
 *   Validity: sample (i, j) is valid iff (weight is NULL or weight[i, j] > 0) and (norm is NULL or both of pose i's entries are finite
 *   and > 0) and (segment is NULL or segment[i] lies in [0, n_segments)).  Only valid samples enter the outputs, for segment s =
 *   segment[i] (0 without segments):  counts[s][k][j] int32 = detected samples,  valid[s][j] int32 = valid samples,  err_sums[s][j] fp64 =
 *   the sum of e.  One block per (segment, joint): thread t of 256 adds its poses t, t + 256, ... in that order, then the 256 partials are
 *   added in a fixed tree (partial t += partial t + o for o = 128, 64, .., 1): the same bits on every call.
 *   Non-finite distances: a NaN e (a NaN coordinate) fails every threshold, counts as valid and makes that (segment, joint)'s err_sums NaN;
 *   e = +inf likewise with an inf sum (IEEE: it passes `<=` only against a threshold that is itself +inf).  No other joint or segment is
 *   affected.  n may be 0: all outputs are zero, and pred, gt and segment may be NULL at any n_segments (no pose, nothing to read).  Every element of the three
 *   outputs is written by every successful call.
 *   Refused before anything is launched, no device needed -- CAPF_ERR_INVALID: NULL counts / valid / err_sums / thresholds, n_thresholds
 *   outside 1..32, a NaN threshold, joints <= 0, n < 0, n_segments <= 0, strict not 0 or 1, and with n > 0: NULL pred or gt,
 *   segment == NULL with n_segments != 1; CAPF_ERR_UNSUPPORTED: joints > 32 (capf_pose_errors' rule), n_segments * joints >= 2^31.
 *   Rates (counts / valid; NaN where valid == 0) and the tables follow on the host: mvn/datasets/human36m.py::evaluate2d, Pck2dAccumulator.
 *   Cost (MI355X, medians of 20 around the host call, two runs, tools/bench_pck2d.py, EXPERIMENTS.md R36.1; 17 joints, 10 thresholds):
 *   0.024 ms at n = 512, 0.82 ms at n = 100 000 (0.89 ms with 2 segments); CA_PF.keypoint_loss + backward at batch 64 (HRNet-32 fp32):
 *   5.90 - 5.96 ms with return_accuracy against 5.81 - 5.87 ms without, + 0.09 ms.  Not a hot path: one block per (segment, joint). */
int capf_pck2d_counts(void* stream, const float* pred, const float* gt, int n, int joints, const float* norm, const float* weight,
                      const double* thresholds, int n_thresholds, int strict, const int32_t* segment, int n_segments, int32_t* counts,
                      int32_t* valid, double* err_sums);

/* ---- N3: the per-frame affine crop in front of the prefetcher ------------------------
 * capf_affine_from_center_scale: get_affine_transform(center, scale, 0, (out_w, out_h)) of
 *   mvn/utils/img.py:16-48 (rot 0, shift 0): the 2x3 row-major double matrix cv2.getAffineTransform returns
 *   for the three float32 point pairs.  Host code, no GPU needed.
 * capf_warp_affine: crop_image (img.py:51-69, called from Human36M.__getitem__ human36m.py:298-300) for a whole
 *   batch: out[b] = cv2.warpAffine(frame_b, m_b, (out_w, out_h), flags=INTER_LINEAR), constant border 0, 8-bit
 *   3-channel.  frames: DEVICE array of `batch` device pointers; dims: device int32 [batch][3] = rows, cols,
 *   row pitch in bytes; m: device double [batch][6] FORWARD matrices; out: uint8 [batch, out_h, out_w, 3].
 *   OpenCV's fixed-point arithmetic (10-bit coordinates, 5-bit fractions, 15-bit weights) is restated from its
 *   published algorithm -- OpenCV is absent from the build container, so this row's parity is unpinned. */
/* capf_jpeg_info / capf_jpeg_decode: the image decode in FRONT of that crop -- cv2.imread(path, IMREAD_COLOR | IMREAD_IGNORE_ORIENTATION) of
 *   Human36M.__getitem__ (human36m.py:292-295) for a baseline JPEG held in host memory: uint8 BGR [height][width][3] on the device, ready
 *   for capf_warp_affine.  The host walks the entropy-coded segment (Huffman decode, DC prediction, restart markers); dequantisation +
 *   inverse DCT, chroma upsampling and YCbCr -> BGR run on the GPU.  The arithmetic is libjpeg's default decode path restated -- "islow"
 *   integer IDCT (jidctint.c), "fancy" triangle upsampling (jdsample.c), 16-bit fixed point colour conversion (jdcolor.c) -- which is what
 *   cv2.imread and Pillow run: the result is bit-exact against Pillow's libjpeg-turbo decode (tests/test_jpeg.py; OpenCV itself is not
 *   in the image).  Baseline / extended sequential Huffman, 8 bit, grey or YCbCr in one interleaved scan, 4:4:4 / 4:2:2 / 4:2:0, restart
 *   intervals; anything else (progressive, arithmetic, CMYK, other sampling, and three-component files libjpeg takes for RGB: no JFIF
 *   APP0 and an Adobe APP14 with transform 0, or neither marker and component ids 'R','G','B') returns CAPF_ERR_UNSUPPORTED and the
 *   caller keeps its host decoder.  capf_jpeg_info: geometry + the scratch bytes capf_jpeg_decode needs (device memory, 16-byte aligned).  capf_jpeg_decode
 *   enqueues on `stream` and waits for the coefficient upload (it reuses a per-thread host staging buffer): a loader-side call, never
 *   part of capf_forward.  capf_jpeg_coefficients: the host half alone -- quantised coefficients in natural order, component after
 *   component, blocks [rows][cols][64] over the MCU-padded image (no GPU needed).                                                      */
int capf_jpeg_info(const uint8_t* data, size_t n_bytes, int32_t* width, int32_t* height, int32_t* components, int32_t* h_samp,
                   int32_t* v_samp, size_t* scratch_bytes);
int capf_jpeg_coefficients(const uint8_t* data, size_t n_bytes, int16_t* coef, size_t coef_elems);
int capf_jpeg_decode(void* stream, const uint8_t* data, size_t n_bytes, uint8_t* out_bgr, size_t out_pitch_bytes, void* scratch,
                     size_t scratch_bytes);
/* capf_jpeg_batch_info / capf_jpeg_decode_batch: the same decode for a BATCH of files in one call, the entropy decode included, with the
 *   output bits of capf_jpeg_decode.  The host parses each file's markers up to SOS and copies the entropy-coded bytes of the whole batch
 *   to the device in ONE upload; the GPU removes FF 00 stuffing, finds the restart markers and decodes the Huffman stream by
 *   self-synchronising subsequences (csrc/jpeg_sync.h): each segment (restart interval, or the whole scan) is cut into subsequence_bytes
 *   pieces, one lane each, whose guessed start states are reconciled in a fixed number of sync rounds, and any segment not yet proven
 *   after them is finished by one lane decoding serially -- results never depend on convergence.  IDCT, upsampling and colour then run
 *   as one grid over all blocks / pixels of the batch.
 *   capf_jpeg_batch_info (host only): info[n][5] = width, height, components, coefficient count (capf_jpeg_coefficients' layout),
 *   status (CAPF_OK or the file's capf_jpeg_info error); *scratch_bytes = device scratch capf_jpeg_decode_batch needs for this batch at
 *   this subsequence length.  Returns the first file's error if any file is outside the supported subset.
 *   capf_jpeg_decode_batch: out_bgr = HOST array of n device pointers (uint8 BGR [height][width][3], row pitch out_pitch_bytes[i]);
 *   coef_out = optional device int16 buffer receiving every file's coefficients back to back (capf_jpeg_coefficients' layout, files in
 *   order); scratch = device memory of at least the batch_info size; status = device int32[n], 0 or a bitwise OR of
 *   1 (a DC category > 11 or an AC size > 10), 2 (a segment's entropy data does not decode to its MCU count), 4 (restart-marker count
 *   differs from ceil(MCUs / interval) - 1).  A flagged file's pixels are undefined; the other files are unaffected.  The whole batch
 *   is refused before anything is enqueued if any file is outside the supported subset (its capf_jpeg_info error).  Enqueues on
 *   `stream` and waits only for its own staging upload, never for the kernels.  subseq_bytes: 0 = the default (256), else 1 .. 2^20.
 * capf_jpeg_coefficients_subseq: the device algorithm's steps run serially on the CPU (same code, lane by lane, same sync rounds and
 *   fallback) -> capf_jpeg_coefficients' output, or CAPF_ERR_INVALID where the device would set a status bit (tests; no GPU). */
int capf_jpeg_batch_info(int n, const uint8_t* const* data, const size_t* n_bytes, int subseq_bytes, int32_t* info, size_t* scratch_bytes);
int capf_jpeg_decode_batch(void* stream, int n, const uint8_t* const* data, const size_t* n_bytes, uint8_t* const* out_bgr,
                           const size_t* out_pitch_bytes, int16_t* coef_out, void* scratch, size_t scratch_bytes, int32_t* status,
                           int subseq_bytes);
int capf_jpeg_coefficients_subseq(const uint8_t* data, size_t n_bytes, int16_t* coef, size_t coef_elems, int subseq_bytes);
/* capf_jpeg_crop_rect / capf_jpeg_crop_batch_info / capf_jpeg_decode_crop_batch: the crop-aware route -- files in, affine crops out, for a
 *   caller whose only use of the frames is capf_warp_affine.  For every file whose status word is 0, out[i] equals
 *   capf_warp_affine(capf_jpeg_decode_batch(file i), m_i) bit for bit, at every subseq_bytes and for any forward matrix (rotation and shear
 *   included).  The entropy decode is capf_jpeg_decode_batch's (it is serial per segment and has to walk every block); from the write pass
 *   on only the MCUs the warp can read are kept: AC coefficients of those MCUs in a compact buffer, one DC difference per block of the
 *   whole image (a DC value is the sum of the differences before it in its segment), then dequantisation, IDCT, upsampling and colour
 *   over that rectangle into a BGR patch which the warp samples with the rectangle's origin subtracted and the IMAGE's border (constant
 *   0).  No full-frame buffer is allocated anywhere.
 *   capf_jpeg_crop_rect (host only): the rule.  pixel_rect = [x0, y0, x1, y1) is the smallest rectangle of a width x height image that
 *   holds every tap of the out_w x out_h crop with forward matrix m: the warp's own fixed-point coordinates (inverse map in double, rounded
 *   to 1/1024, taps at the integer part and the integer part + 1) evaluated at the four output corners -- each axis is a sum of one
 *   monotonic term per output coordinate, so the corners give the exact extremes --, clamped to the image.  All four are 0 when the crop
 *   lies wholly outside the image (the output is then all border).  mcu_rect = [mx0, my0, mx1, my1) in MCUs of 8 h_samp x 8 v_samp
 *   pixels: pixel_rect grown by one pixel on the sides along which chroma is subsampled (h_samp / v_samp = 2: "fancy" upsampling
 *   reads the neighbouring chroma sample and replicates only at true image edges), clamped, then widened to whole MCUs.  h_samp, v_samp:
 *   capf_jpeg_info's (1,1 / 2,1 / 2,2; grey files report 1,1).
 *   capf_jpeg_crop_batch_info (host only): m = host double [n][6]; info[n][13] = width, height, components, coefficients kept (64 per
 *   block of the MCU rectangle), status (CAPF_OK or the file's capf_jpeg_info error), pixel_rect[4], mcu_rect[4]; *scratch_bytes = device
 *   scratch capf_jpeg_decode_crop_batch needs for these files, matrices, output size and subsequence length.  n >= 1.
 *   capf_jpeg_decode_crop_batch: m = HOST double [n][6] forward matrices; out = device uint8 [n, out_h, out_w, 3]; scratch, status,
 *   subseq_bytes, the refusal of a batch holding an unsupported file and the stream behaviour (enqueue, wait only for the staging
 *   upload) as capf_jpeg_decode_batch.  A flagged file's crop is undefined; the other files are unaffected.                              */
int capf_jpeg_crop_rect(int width, int height, int h_samp, int v_samp, const double m[6], int out_w, int out_h, int32_t pixel_rect[4],
                        int32_t mcu_rect[4]);
int capf_jpeg_crop_batch_info(int n, const uint8_t* const* data, const size_t* n_bytes, const double* m, int out_w, int out_h,
                              int subseq_bytes, int32_t* info, size_t* scratch_bytes);
int capf_jpeg_decode_crop_batch(void* stream, int n, const uint8_t* const* data, const size_t* n_bytes, const double* m, int out_h,
                                int out_w, uint8_t* out, void* scratch, size_t scratch_bytes, int32_t* status, int subseq_bytes);
int capf_affine_from_center_scale(const double center[2], const double scale[2], int out_w, int out_h, double m[6]);
int capf_warp_affine(void* stream, const uint8_t* const* frames, const int32_t* dims, const double* m, int batch,
                     int out_h, int out_w, uint8_t* out);
/* capf_erase_scratch_bytes / capf_erase_patches: erase_image (ContextPose/mvn/utils/img.py:179-198), the joint-centred cut-out behind the
 *   configuration's train.erase / val.erase, for a batch of uint8 crops on the device -- between capf_jpeg_decode_crop_batch / capf_warp_affine
 *   and capf_preprocess / capf_forward_u8.  images / out: uint8 [batch, height, width, 3]; centers: fp32 [batch, patches, 2] = (x, y) in crop
 *   pixels; mask: uint8 [batch, patches] or NULL (every patch).  Frame b becomes
 *       erase_image(images[b], [centers[b, p] for p ascending if mask == NULL or mask[b, p] != 0], size, use_mean)
 *   bit for bit (tests/golden/erase_reference.npz holds the reference's own outputs; tests/erase_oracle.py is the integer restatement):
 *   Truncation.  A centre counts iff x > -1 && x < width && y > -1 && y < height, evaluated on the floats: the reference's int() (toward
 *     zero) followed by its range test, so -0.5 truncates to 0 and counts, -1.0 does not, width - 0.25 does, width does not.
 *   Patch.  xc = (int)x, yc = (int)y; columns [max(0, xc - size / 2), min(width, xc + size / 2 + 1)), rows likewise with height (integer
 *     division: size 0 and 1 paint one pixel).  use_mean == 0: the patch becomes 0.  Otherwise each channel becomes the mean of that channel
 *     over the patch in the ORIGINAL image, truncated as numpy stores a float64 into a uint8 array: the integer sum / count, from 64-bit sums.
 *   Overlap order.  Patches apply in ascending p: a pixel under several counting patches takes the value of the highest p, a mean never
 *     sees an earlier patch's paint, a pixel under none is copied.
 *   The one divergence.  A NaN or infinite centre fails the test above and is skipped (1e30 too, without a float-to-int conversion); the
 *     reference's int() raises on a non-finite one.
 *   out == images (in place) gives the bits of the out-of-place call.  Two launches on `stream`, no atomics, no allocation, no
 *   synchronisation; results do not depend on the launch geometry.  scratch: device memory, 16-byte aligned, at least
 *   capf_erase_scratch_bytes(batch, patches) bytes (32 per patch; 0 for batch < 1, patches < 1 or patches > 32), sharing no byte with images / out.
 *   Refused before anything is launched, no device needed -- CAPF_ERR_INVALID: NULL images / centers / out / scratch, batch / height / width /
 *   patches < 1, size < 0, scratch_bytes too small or scratch misaligned, out overlapping images other than out == images, scratch
 *   overlapping either; CAPF_ERR_UNSUPPORTED: patches > 32 (the joint cap), a frame of more than 2^31 - 1 bytes, batch * ceil(height *
 *   width / 256) >= 2^31.                                                                                                                  */
size_t capf_erase_scratch_bytes(int batch, int patches);
int capf_erase_patches(void* stream, const uint8_t* images, int batch, int height, int width, const float* centers, const uint8_t* mask,
                       int patches, int size, int use_mean, uint8_t* out, void* scratch, size_t scratch_bytes);

/* ---- measurement aids (bench.py roofline line; no reference counterpart) -------------------------
 * capf_op_info: op `index` in launch order: its plan name, the kernel (template instantiation) it
 *   launches at `batch`, and its algorithmic FLOPs at `batch`.
 * capf_forward_profile: capf_forward with a hipEvent pair recorded on `stream` around every launch;
 *   synchronises the stream and writes the elapsed milliseconds per op into op_ms[0..n_ops).  Every op is
 *   launched on its own, in program order (capf_set_lanes is ignored).
 * capf_forward_profile_launches: the same for the PRODUCT schedule (capf_set_lanes 0 or 2 / 3; side streams are
 *   not used: mode 3 is timed as its one-chain form): one event pair per launch.  op_leader[i] = first op of the launch op i rode in (-1: not
 *   launched); op_ms[i] = elapsed ms of that launch if i is a leader, else 0.  A grouped launch therefore
 *   shows up as one time for several ops.                                                              */
int capf_num_ops(const capf_handle* h);
int capf_op_info(const capf_handle* h, int index, int batch, const char** name, const char** kernel,
                 double* flops);
/* FLOPs the matrix pipe is asked to EXECUTE for op `index` at `batch` (2 x issued MACs; K padding included, tile-edge padding
 * not).  Differs from capf_op_info's ALGORITHMIC count for the Winograd kernels (F(4,3): 1/2, F(2,3): 2/3 of the direct
 * convolution's multiplies): bench.py reports both, so that `roofline.frac` (algorithmic / peak) is never read
 * as matrix-pipe utilisation. */
int capf_op_executed_flops(const capf_handle* h, int index, int batch, double* flops);
/* Algorithmic (compulsory) HBM bytes of op `index` at `batch`: each operand read once, the result written once
 * (bf16 tensors 2 B/element).  bench.py's HBM-side roofline divides these by the measured launch durations. */
int capf_op_bytes(const capf_handle* h, int index, int batch, double* bytes);
/* capf_op_schedule: where op `index` sits in the launch schedule: its fork/join region (-1 outside / control op),
 *   its dependency level inside the region (capf_set_lanes mode 2 issues a region level by level), its lane
 *   (mode 1: side stream), and the workspace buffer ids it reads (5 slots) and writes (6 slots; a conv's / fuse sum's bf16 shadow under
 *   CAPF_PLAN_BF16_F32_STREAM in the third), -1 = unused,
 *   -2 = the external image.  Lets host-side tests check that the schedule is a valid topological order. */
int capf_op_schedule(const capf_handle* h, int index, int32_t* region, int32_t* level, int32_t* lane,
                     int32_t reads[5], int32_t writes[6]);
/* The stream class op `index` is issued on at `batch` under the current capf_set_lanes mode: 0 = the caller's stream, 1 = a library-owned
 *   stream that runs a lane (mode 1) or the side chain (mode 3 at batch 16..128: lanes 1 + 2 of a region with two or more lanes).  The
 *   event-bracketed profiling runs (capf_forward_profile*) stay on the caller's stream.  Lets host-side tests and tools
 *   see which schedule a handle runs.  (Additive to revision 12: struct layouts and every existing entry point unchanged.) */
int capf_op_stream_class(const capf_handle* h, int index, int batch);
/* ---- layer-wise ("teacher-forced") parity aids ---------------------------------------------------------------
 * A deep bf16 network is chaotic at the rounding level: two correct implementations that differ only in fp32 summation
 * order drift apart to the full bf16 noise floor after ~50 layers, so an end-to-end comparison cannot be tighter than that
 * floor.  What CAN be tight is one op at a time on the engine's OWN inputs:
 *   capf_forward_prefix : the product schedule (grouped launches and all) for the first n_ops ops only; k2d / kcrop_inout /
 *                         out may be NULL while n_ops stays inside the backbone.
 *   capf_op_describe    : geometry, operand types and parameter indices of op `index`, and `checkpoint` = the prefix
 *                         length after which every tensor the op touched is still intact in the workspace (buffers are
 *                         reused along the plan; a fork/join region keeps all of its buffers until its join).
 *   capf_op_tensor      : device pointer of one operand of op `index` after such a prefix (slot 0..3 inputs, 4 residual,
 *                         5 output, 6 the bf16 shadow of an fp32 output under CAPF_PLAN_BF16_F32_STREAM -- CAPF_ERR_INVALID where the op
 *                         writes none; the external image for the stem's input).  Under that flag in_dtype / out_dtype are what is
 *                         stored (a conv reading a shadow: in_dtype 2), and every residual a conv reads is fp32.
 * tests/test_gpu_layerwise.py recomputes every backbone op on the CPU from the engine's inputs and compares outputs.   */
typedef struct capf_op_desc {
    int32_t kind;              /* 0 conv / linear on the MFMA kernels, 1 fuse-sum, 2 max-pool 3x3 s2, 3 bilinear resize, 4 LayerNorm over rows,
                                * 5 multi-head self-attention over the tokens of a group, -1 other */
    int32_t backbone;          /* 1: the op belongs to the backbone plan */
    int32_t conv;              /* kind 0: 1 = convolution (NHWC), 0 = rows-mode linear */
    int32_t Cin, H, W, Cout, Ho, Wo, ks, stride, pad, act;   /* act: 0 none, 1 ReLU, 2 GELU */
    int32_t in_dtype, out_dtype;                             /* capf_tensor convention: 0 fp32, 2 bf16, 3 fp16 */
    int32_t mfma_bf16;         /* operands are rounded to the handle's 16-bit compute dtype for the matrix pipe (bf16, or fp16 on a CAPF_F16 handle) */
    int32_t n_in, shift[4], relu;                            /* fuse-sum: inputs, log2 nearest-upsample factors, ReLU */
    int32_t p_weight, p_bn_weight;                           /* capf_param_info indices of <conv>.weight and <bn>.weight; -1 */
    int32_t has_residual;
    int32_t checkpoint;
    /* rows-mode ops of the lifter (kind 0 with conv == 0, kinds 4 and 5; pose_dformer.py:15-79): row m of an operand lives at element
     * (m / G) * S1 + (m % G) * S2 + off of its buffer, maps[k] = {G, S1, S2, off} for k = 0 input rows, 1 output rows, 2 residual rows
     * (kind 4: the rows ADDED to the input before normalising).  kind 0: Cin = K, Cout = N, p_weight / p_bias [N,K] / [N]; an
     * in-place update (proj, fc2: output rows == residual rows) reads its residual from the state BEFORE the op, i.e. after
     * capf_forward_prefix(index), its result after capf_forward_prefix(index + 1).  kind 4: Cin = width, p_ln_weight / p_ln_bias, eps.
     * kind 5: input rows [groups * tokens, 3 * heads * head_dim] ordered (q | k | v) x heads x head_dim (pose_dformer.py:49), output
     * rows [groups * tokens, heads * head_dim]; groups per frame / tokens / heads / head_dim in attn[4].                            */
    int32_t rows_per_frame;
    int32_t p_bias, p_ln_weight, p_ln_bias;
    float eps;
    int32_t attn[4];
    int64_t maps[3][4];
    /* kind 0, conv: up_H > 0 = the tensor in slot 1, [B, up_H, up_W, Cout] in the output's dtype, is resized to Ho x Wo (bilinear, align_corners =
     * True) and ADDED BEHIND the activation, in fp32, before the one storage rounding: CPN's `lateral + upsampled path` (globalNet.py:66) inside the
     * lateral conv's launch (compute_dtype = bf16; CAPF_PLAN_NO_UPADD: a kind-3 op behind the conv instead).  0 otherwise.                          */
    int32_t up_H, up_W;
} capf_op_desc;
int capf_forward_prefix(capf_handle* h, void* stream, const float* images_nhwc, const float* k2d, float* kcrop_inout,
                        int batch, float* out, int n_ops);
int capf_op_describe(const capf_handle* h, int index, capf_op_desc* desc);          /* writes sizeof(capf_op_desc) of THIS header's revision */
/* ... for callers that cannot rule out a header / library mismatch: never writes more than desc_bytes (what the caller's struct holds);
 * fields beyond that are dropped, a shorter library struct leaves the caller's tail zeroed.                                            */
int capf_op_describe_sized(const capf_handle* h, int index, void* desc, size_t desc_bytes);
int capf_op_tensor(const capf_handle* h, int index, int slot, const void** dev_ptr);
/* Does op `index` exchange a PLANES tensor (capf_op_conv_f32h2_planes) with its BasicBlock partner at this batch?  Returns 0: no (plain fp32 on both
 * sides), 1: its OUTPUT (slot 5) holds planes, 2: its INPUT (slot 0) does; *exps: the device pointer of the int32 [tiles][channels / 16] exponent table
 * (valid after a forward of that batch), *tile_pixels: output pixels per tile.  The layer-wise tests decode the planes with these.                 */
int capf_op_h2_planes(const capf_handle* h, int index, int batch, const void** exps, int32_t* tile_pixels);

int capf_forward_profile(capf_handle* h, void* stream, const float* images_nhwc, const float* k2d,
                         float* kcrop_inout, int batch, float* out, float* op_ms, int n_ops);
int capf_forward_profile_launches(capf_handle* h, void* stream, const float* images_nhwc, const float* k2d,
                                  float* kcrop_inout, int batch, float* out, float* op_ms, int32_t* op_leader,
                                  int n_ops);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif /* CAPF_H */
