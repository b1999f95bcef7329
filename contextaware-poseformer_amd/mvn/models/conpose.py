"""CA_PF — drop-in for ContextPose/mvn/models/conpose.py:10-42 running on libcapf.so.

Same constructor (`CA_PF(config, device)`), same attributes (`.backbone`, `.volume_net`), same
state_dict names/shapes, same call

    model(images[B,H,W,3] fp32 NHWC, keypoints_2d_cpn[B,17,2], keypoints_2d_cpn_crop[B,17,2]) -> [B,1,17,3]

including the reference's in-place normalisation of the third argument (conpose.py:34-35).  The
compute is one capf_forward call: hand-written gfx950 kernels, enqueued on torch's current stream.
There is no eager / CPU fallback: CPU tensors or a missing libcapf.so raise.
"""
import collections

import torch
from torch import nn

from capf.lib import (KP_INTEGRAL, KP_LOSS_REDUCTIONS, KP_MODES, PLAN_BN_BATCH_STATS, PLAN_CPN_PREDICT, CapfError, Engine, cpn_decode,
                      cpn_decode_pair, fliptest_fuse, input_constants, kp_head_backward, kp_head_forward, kp_head_forward_pair, kp_heatmap_loss,
                      pck2d_counts)

from . import _native


MIRROR_MODES = {"none": 0, "all": 1, "pair": 2}       # CA_PF.forward_u8's `mirror` -> capf_preprocess's mode
CROP_HALF = (192 // 2, 256 // 2)                      # conpose.py:34: ref = kcrop / (96, 128) - 1, so d(ref)/d(kcrop) = 1 / (96, 128)

# Where the context maps of one call come from.  An entry point builds this record and nothing downstream looks at the entry any more.
#   kind "images"     data = the fp32 NHWC images: the backbone runs on them
#        "u8"         data = (uint8 BGR crops, mean, std, capf_preprocess's mode): the same, the stem reads the crops
#        "workspace"  data = None: the maps of this batch are in the workspace already (forward_detect ran the backbone and the head)
#        "maps"       data = four contiguous NHWC maps of the caller's
# batch counts ENGINE frames (2 * Bsrc for a flip-test pair); word is what the messages call the source.
_Source = collections.namedtuple("_Source", "kind device batch word data")


def _require_cuda(dev):
    if dev.type != "cuda":
        raise CapfError("CA_PF runs on an MI355X only: inputs are on {} (no CPU fallback)".format(dev))


def _run_backbone(owner, eng, src, stream):
    """The backbone alone on an image source: its maps stay in the workspace (no gradient reaches it)."""
    if src.kind == "u8":
        eng.backbone_forward_u8(*src.data, stream)
    elif owner._bn_batch_active():
        owner._backbone_forward_bn(eng, src.data, stream)
    else:
        eng.backbone_forward(src.data, stream)


def _run_source(owner, eng, src, k2d, kcrop, out, stream, train, masks=None):
    """(source, training step?, batch statistics active?) -> engine calls: the one place that states this table, and with _run_backbone
    the only caller of the engine's forward entries.  `train`: the native training step (activations kept for ONE backward)."""
    if src.kind == "u8":            # the stem reads the crops (nothing in the backward reads the image)
        if train:
            eng.forward_train_u8(*src.data, k2d, kcrop, out, stream, masks)
        else:
            eng.forward_u8(*src.data, k2d, kcrop, out, stream)
    elif src.kind == "images" and not owner._bn_batch_active():
        if train:
            eng.forward_train(src.data, k2d, kcrop, out, stream, masks)
        else:
            eng.forward(src.data, k2d, kcrop, out, stream)
    else:                           # the lifter alone, on maps that ...
        if src.kind == "images":    # ... the backbone makes with batch statistics (backbone_bn="batch", backbone in train mode)
            owner._backbone_forward_bn(eng, src.data, stream)
        elif src.kind == "maps":    # ... the caller supplies ("workspace": they are there)
            eng.set_features(src.data, stream)
        if train:
            eng.lifter_forward_train(k2d, kcrop, out, stream, masks)
        else:
            eng.lifter_forward(k2d, kcrop, out, stream)


def _private_ref(ctx, index, kcrop):
    """The buffer a step hands to the engine as kcrop_inout: the caller's tensor (normalised in place, conpose.py:34-35), unless it takes
    part in the graph -- then a private contiguous copy, because the in-place write would raise on a leaf and corrupt a non-leaf."""
    return kcrop.detach().clone(memory_format=torch.contiguous_format) if ctx.needs_input_grad[index] else kcrop


def _crop_grad(owner, dref):
    """dL/d(crop keypoints in pixels) from dL/d(ref): one division by (96, 128)."""
    scale = owner.__dict__.setdefault("_crop_half", {})
    if dref.device not in scale:
        scale[dref.device] = torch.tensor(CROP_HALF, dtype=torch.float32, device=dref.device)
    return dref / scale[dref.device]


class _LifterStep(torch.autograd.Function):
    """Autograd boundary of the native training step on any source: forward = _run_source(..., train), backward = capf_backward into one flat
    gradient buffer whose slices are returned as the parameter gradients (so torch optimizers, DDP hooks and `capf.dist.allreduce_mean_`
    all see ordinary .grad tensors).  Caller-supplied maps travel as n_maps (0 or 4) leading tensor arguments, contiguous NHWC (the permute
    from the backbone's NCHW, and its transpose on the way back, are torch's): backward = capf_backward_maps, which returns their gradient
    too.  When k2d or kcrop takes part in the graph, backward = capf_backward_points and their gradients are returned as well (kcrop's
    w.r.t. the pixel values the caller passed)."""

    @staticmethod
    def forward(ctx, owner, eng, src, k2d, kcrop, masks, names, n_maps, *maps_and_params):
        feats, params = maps_and_params[:n_maps], maps_and_params[n_maps:]
        out = torch.empty(src.batch, 1, owner.num_joints, 3, dtype=torch.float32, device=src.device)
        kcrop = _private_ref(ctx, 4, kcrop)
        _run_source(owner, eng, src, k2d, kcrop, out, torch.cuda.current_stream(src.device).cuda_stream, True, masks)
        ctx.token = eng.train_generation()
        ctx.eng, ctx.masks, ctx.names, ctx.owner, ctx.n_maps = eng, masks, names, owner, n_maps
        if n_maps:
            ctx.map_grad_mode = resolve_map_grad_mode(owner.map_grad_mode)      # (the step's mode is the one in force at its forward)
        ctx.keep = (k2d, kcrop)     # the backward re-reads the keypoints / normalised ref: keep them alive
        ctx.map_shapes = [f.shape for f in feats]
        ctx.shapes = [p.shape for p in params]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        eng = ctx.eng
        if eng.train_generation() != ctx.token:
            raise CapfError("backward of a CA_PF forward whose saved activations were overwritten by a later forward on the "
                            "same engine (the native step keeps ONE set of activations in its workspace): call backward "
                            "before the next forward of this model")
        layout, total = eng.grad_layout_cached()
        flat = torch.empty(total, dtype=torch.float32, device=grad_out.device)
        dfeat = [torch.empty(shp, dtype=torch.float32, device=grad_out.device) for shp in ctx.map_shapes] if ctx.n_maps else None
        stream = torch.cuda.current_stream(grad_out.device).cuda_stream
        if dfeat is not None and eng.map_grad_mode() != ctx.map_grad_mode:      # a state change of the handle: once per change, not per step
            eng.set_map_grad_mode(ctx.map_grad_mode)
        need_k2d, need_ref = ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        dk2d = dkcrop = None
        if need_k2d or need_ref:
            dk2d = torch.empty_like(ctx.keep[0]) if need_k2d else None
            dref = torch.empty_like(ctx.keep[1]) if need_ref else None
            eng.backward_points(grad_out.contiguous(), flat, stream, ctx.masks, dfeat, dk2d, dref)
            dkcrop = _crop_grad(ctx.owner, dref) if need_ref else None
        elif dfeat is not None:
            eng.backward_maps(grad_out.contiguous(), flat, dfeat, stream, ctx.masks)
        else:
            eng.backward(grad_out.contiguous(), flat, stream, ctx.masks)
        ctx.owner.last_flat_grad = flat
        head = (None, None, None, dk2d, dkcrop, None, None, None)
        if dfeat is not None:           # (map gradients only for maps that require grad)
            head += tuple(g if need else None for g, need in zip(dfeat, ctx.needs_input_grad[8:8 + ctx.n_maps]))
        if ctx.owner.flat_grad_only:      # the caller consumes last_flat_grad itself (capf.optim.FusedAdamW + capf.dist)
            return head + (None,) * len(ctx.names)
        grads = tuple(flat[layout[n][0]: layout[n][0] + layout[n][1]].view(shp) for n, shp in zip(ctx.names, ctx.shapes))
        return head + grads


class KeypointHead(nn.Module):
    """HRNet's final_layer (nn.Conv2d(C0, num_joints, 1), pose_hrnet.py:497-501) as a parameter holder: a COCO checkpoint's
    final_layer.weight / final_layer.bias load into it by name.  The module is never called -- the 1x1 conv and the heatmap decode are one
    native pass over feat0 (capf_kp_head_forward); torch's default Conv2d initialisation serves a head trained from scratch (CPN)."""

    def __init__(self, channels, num_joints):
        super().__init__()
        self.final_layer = nn.Conv2d(channels, num_joints, kernel_size=1, stride=1, padding=0)

    def forward(self, *args):
        raise CapfError("KeypointHead only holds final_layer's parameters: use CA_PF.detect / forward_detect or "
                        "mvn.models.conpose.keypoint_head (there is no eager path)")


class _KeypointHeadFn(torch.autograd.Function):
    """Autograd boundary of the native keypoint head: forward = capf_kp_head_forward on an NHWC map, backward (integral decode, fp32 map) =
    capf_kp_head_backward: gradients of final_layer's weight, an exactly zero bias gradient, and dL/d(map) when the map requires grad.
    `guard`: None for a map tensor of the caller's, or {"eng", "token"} when the map is a view of an engine's workspace -- the backward
    re-reads it there and refuses, like the lifter's, once a later run has overwritten it."""

    @staticmethod
    def forward(ctx, x, weight, bias, to_image, mode, beta, decode, guard):
        kcrop, score, k2d, _ = kp_head_forward(x, weight, bias, mode, beta, decode, to_image)
        ctx.x, ctx.weight, ctx.bias, ctx.to_image = x, weight.detach(), None if bias is None else bias.detach(), to_image
        ctx.mode, ctx.beta, ctx.decode, ctx.guard = mode, beta, decode, guard
        ctx.mark_non_differentiable(score)
        if k2d is None:
            k2d = kcrop.new_empty(0)
            ctx.mark_non_differentiable(k2d)
        return kcrop, score, k2d

    @staticmethod
    def backward(ctx, dkcrop, _dscore, dk2d):
        if ctx.mode != KP_INTEGRAL:
            raise CapfError("the argmax keypoint head has no derivative: build the model with keypoint_head='integral' to train it")
        if ctx.x.dtype != torch.float32:
            raise NotImplementedError("the keypoint head's backward needs an fp32 map (capf_kp_head_backward), got {}".format(ctx.x.dtype))
        g = ctx.guard
        if g is not None and g["eng"].train_generation() != g["token"]:
            raise CapfError("backward of a keypoint head whose map (feat0 in the engine's workspace) was overwritten by a later forward "
                            "on the same engine: call backward before the next forward of this model")
        if ctx.to_image is None:
            dk2d = None
        want_dmap = ctx.needs_input_grad[0]
        dw, db, dmap = kp_head_backward(ctx.x.detach(), ctx.weight, ctx.bias, None if dkcrop is None else dkcrop.contiguous(),
                                        None if dk2d is None else dk2d.contiguous(), ctx.beta, ctx.decode, ctx.to_image, want_dmap)
        return (dmap, dw.view(ctx.weight.shape) if ctx.needs_input_grad[1] else None,
                db if ctx.bias is not None and ctx.needs_input_grad[2] else None, None, None, None, None, None)


def keypoint_head(map_nhwc, weight, bias=None, to_image=None, mode="integral", beta=1.0, decode=(1.0, 0.0, 1.0, 0.0)):
    """The native keypoint head as a free function on ANY contiguous NHWC map [B, H, W, C] (fp32; bf16 / fp16 without gradients):
    returns (kcrop [B, J, 2], score [B, J], k2d [B, J, 2] | None).  With mode="integral" the result is differentiable in weight [J, C]
    or [J, C, 1, 1], in bias (gradient exactly 0) and in the map: a torch backbone in front of CA_PF.forward_features gets the head's and
    the lifter's gradients.  decode = (sx, ox, sy, oy): heatmap -> crop pixels; to_image [B, 2, 3]: crop pixels -> the lifter's k2d."""
    if not isinstance(mode, str) or mode not in KP_MODES:
        raise ValueError("mode must be 'argmax' or 'integral', got {!r}".format(mode))
    kcrop, score, k2d = _KeypointHeadFn.apply(map_nhwc, weight, bias, to_image, KP_MODES[mode], float(beta),
                                              tuple(float(v) for v in decode), None)
    return kcrop, score, (k2d if to_image is not None else None)


class _HeatmapLossFn(torch.autograd.Function):
    """Autograd boundary of the native heatmap loss: forward = capf_kp_heatmap_loss on an NHWC map, which produces the gradients of the loss in
    the same call; they are kept and backward multiplies them by grad_output.  Nothing is re-read later, so a map in an engine's workspace
    needs no guard."""

    @staticmethod
    def forward(ctx, x, weight, bias, kcrop_gt, target_weight, decode, sigma, reduction, topk, scale):
        need_map = ctx.needs_input_grad[0]
        if need_map and x.dtype != torch.float32:
            raise NotImplementedError("the heatmap loss's map gradient needs an fp32 map (capf_kp_heatmap_loss), got {}".format(x.dtype))
        need_params = ctx.needs_input_grad[1] or (bias is not None and ctx.needs_input_grad[2])
        loss, _, dw, db, dmap = kp_heatmap_loss(x.detach(), weight.detach(), None if bias is None else bias.detach(), kcrop_gt, target_weight,
                                                decode, sigma, reduction, topk, scale, want_grads=need_params, want_dmap=need_map)
        ctx.grads = (dmap, None if dw is None else dw.view(weight.shape), db if bias is not None else None)
        return loss.view(())

    @staticmethod
    def backward(ctx, grad_out):
        return tuple(g * grad_out if g is not None and need else None for g, need in zip(ctx.grads, ctx.needs_input_grad[:3])) + (None,) * 7


def keypoint_heatmap_loss(map_nhwc, weight, bias, keypoints_crop, target_weight=None, decode=(1.0, 0.0, 1.0, 0.0), sigma=2.0, reduction="mean",
                          topk=8, scale=0.5):
    """Heatmap supervision of the native keypoint head as a free function on ANY contiguous NHWC map [B, H, W, C] (fp32 / bf16 / fp16): the
    mean-squared error of final_layer's heatmaps against Gaussians of `sigma` cells around keypoints_crop [B, J, 2] (crop pixels; decode =
    (sx, ox, sy, oy): heatmap -> crop pixels), weighted per joint by target_weight [B, J] -- upstream HRNet's JointsMSELoss (reduction "mean",
    scale 0.5) / JointsOHKMMSELoss ("ohkm": the topk hardest joints of each frame).  Returns a 0-d loss, differentiable in weight [J, C] or
    [J, C, 1, 1], in bias (a real gradient) and, for an fp32 map, in the map; a 16-bit map that requires grad raises NotImplementedError.
    Neither the heatmaps nor the targets are materialised (capf_kp_heatmap_loss)."""
    if not isinstance(reduction, str) or reduction not in KP_LOSS_REDUCTIONS:
        raise ValueError("reduction must be 'mean' or 'ohkm', got {!r}".format(reduction))
    gt = keypoints_crop.detach().to(torch.float32).contiguous()
    tw = None if target_weight is None else target_weight.detach().to(torch.float32).reshape(gt.shape[0], gt.shape[1]).contiguous()
    return _HeatmapLossFn.apply(map_nhwc, weight, bias, gt, tw, tuple(float(v) for v in decode), float(sigma), KP_LOSS_REDUCTIONS[reduction],
                                int(topk), float(scale))


# What CA_PF's two detect flows (_single_flow, _pair_flow) need to know about a keypoint head -- everything that differs between the heads is
# here and nowhere else; CA_PF.__init__ picks one from keypoint_head.  `m` is the CA_PF.
#   maps                            the workspace tensor the head reads, as Engine.tensor_view names it
#   decode(H, W, h, w)              heatmap [h, w] -> pixels of the H x W crop, as (sx, ox, sy, oy)
#   trains(m)                       this call must produce gradients of the head's parameters; refuses what has no derivative
#   single(m, eng, maps, decode, to_image, trains) -> (kcrop, score, k2d | None, guard | None)
#   pair(m, maps, decode, to_image, swap, ...)     -> (kcrop2 [2,B,J,2], score [B,J], k2d2 [2,B,J,2] | None); always without grad.  What only
#                                   one head's pair takes follows `swap` as a keyword of the entry's: `shift` (_FinalLayerHead: HRNet's
#                                   SHIFT_HEATMAP; detect_flip_test / forward_detect_flip_test pass it), nothing for _CpnHead
# The record is fixed at construction.  keypoint_head_mode may still be switched between "argmax" and "integral" afterwards (both are
# _FinalLayerHead, which reads the mode at each call); switching to or from "cpn" that way is not supported (other plan, other parameters).
class _FinalLayerHead:
    """keypoint_head="argmax" / "integral": self.keypoint_head.final_layer and the heatmap decode, one native pass over feat0."""
    maps = "feat0"

    @staticmethod
    def decode(H, W, h, w):
        return (float(W) / w, 0.0, float(H) / h, 0.0)       # HRNet's convention: heatmap cell -> crop pixel

    @staticmethod
    def trains(m):
        return m._head_trains()

    @staticmethod
    def single(m, eng, feat0, decode, to_image, trains):
        weight, bias = m._head_params()
        guard = {"eng": eng, "token": None} if trains else None
        with torch.set_grad_enabled(trains):
            kcrop, score, k2d = _KeypointHeadFn.apply(feat0, weight, bias, to_image, KP_MODES[m.keypoint_head_mode], m.keypoint_beta, decode, guard)
        return kcrop, score, (k2d if to_image is not None else None), guard

    @staticmethod
    def pair(m, feat0, decode, to_image, swap, shift):
        weight, bias = m._head_params()
        return kp_head_forward_pair(feat0, weight.detach(), bias.detach(), KP_MODES[m.keypoint_head_mode], m.keypoint_beta, swap, bool(shift),
                                    decode, to_image, float(2 * CROP_HALF[0]))[:3]


class _CpnHead:
    """keypoint_head="cpn": the backbone pass ran refine_net.final_predict too; CPN's two-peak decode of its heatmaps.  No derivative."""
    maps = "heat"

    @staticmethod
    def decode(H, W, h, w):
        sx, sy = float(W) / w, float(H) / h
        return (sx, 0.5 * sx, sy, 0.5 * sy)      # CPN's convention, (4 x + 2) / data_shape of cpn/test.py:106-107 in crop pixels: a cell's centre

    @staticmethod
    def trains(m):
        m._cpn_head_frozen()
        return False

    @staticmethod
    def single(m, eng, heat, decode, to_image, trains):
        with torch.no_grad():
            return cpn_decode(heat, m.num_joints, decode, to_image)[:3] + (None,)

    @staticmethod
    def pair(m, heat, decode, to_image, swap):
        return cpn_decode_pair(heat, m.num_joints, swap, decode, to_image, float(2 * CROP_HALF[0]))[:3]


MAP_GRAD_MODES = {"atomic": 0, "ordered": 1}
BACKBONE_BN_MODES = ("running", "batch")
BN_MOMENTUM = 0.1      # nn.BatchNorm2d's default, which every BatchNorm of the reference backbones keeps (pose_hrnet.py BN_MOMENTUM = 0.1)


def resolve_map_grad_mode(value):
    """CA_PF.map_grad_mode -> capf_set_map_grad_mode's argument.  None follows torch: the library has a deterministic form of the map
    gradient, so torch.use_deterministic_algorithms(True) selects it."""
    if value is None:
        return 1 if torch.are_deterministic_algorithms_enabled() else 0
    if not isinstance(value, str) or value not in MAP_GRAD_MODES:
        raise ValueError("map_grad_mode must be None, 'atomic' or 'ordered', got {!r}".format(value))
    return MAP_GRAD_MODES[value]


class CA_PF(nn.Module):
    def __init__(self, config, device="cuda:0", compute_dtype="fp32", context_blocks=True, plan_flags=0, backbone_bn="running",
                 keypoint_head=None, keypoint_beta=1.0):
        """keypoint_head: None (default) -- the module, its state_dict and its engines are exactly the reference's: the 2-D keypoints come
        from outside.  "argmax" / "integral": the module gains self.keypoint_head.final_layer (weight [J, C0, 1, 1], bias [J]; an HRNet COCO
        checkpoint's final_layer.* load by name, CPN gets a fresh head on its 256-channel feat0) and detect / forward_detect run it on
        feat0: "argmax" is the hard decode HRNet checkpoints are evaluated with (no gradient), "integral" the soft-argmax
        softmax(keypoint_beta * heatmap) whose weights train through the lifter (forward_detect under grad, fp32 models).
        "cpn" (CPN backbones only, fp32 / bf16; anything else: ValueError): the head the CPN checkpoint itself carries,
        backbone.refine_net.final_predict.* (refineNet.py:64-70), and CPN's own two-peak decode (cpn/test.py:79-108).  NO module and NO
        parameter is added -- state_dict() is the default module's, the checkpoint's weights are the head --; the engines are created with
        PLAN_CPN_PREDICT, so the backbone pass also leaves the heatmaps ("heat"), and detect / forward_detect decode them with
        capf_cpn_decode.  The head has no derivative and belongs to the frozen backbone.  CPN's own test-time flip (the heatmaps of the crop
        and of its mirror averaged without a column shift, cpn/test.py:44-70) has entries of its own, detect_cpn_flip /
        forward_detect_cpn_flip; HRNet's detect_flip_test / forward_detect_flip_test raise for this head.
        backbone_bn: what the frozen backbone's BatchNorm layers do while `self.backbone.training` is set.  "running" (default): the
        running statistics, folded into the convs, whatever the mode -- i.e. a frozen backbone left in .train() silently gets eval-mode
        BatchNorm.  "batch" (HRNet, fp32): the module honours self.backbone.training as torch does -- in train mode every forward
        normalises with the statistics of the batch, moves running_mean / running_var with momentum 0.1 and counts num_batches_tracked
        (capf_backbone_forward_bn; what ContextPose_mpi/run_3dhp.py:31-35 computes, which never calls backbone.eval()); in eval mode
        (an explicit backbone.eval() wins) today's route, on the statistics as they then stand.  No gradient reaches the backbone.
        compute_dtype: 'fp32' (exact fp32 MFMA, the reference's precision), 'bf16' (backbone convolutions on
        bf16 MFMA with bf16 activations and fp32 accumulation; the lifter stays fp32) — an extension of the
        reference signature for BASELINE.json's bf16 configurations — or 'fp16' (the bf16 plan with IEEE fp16 as its
        16-bit element: same speed, 11 significand bits instead of 8; HRNet backbones, inference only)."""
        if not isinstance(backbone_bn, str) or backbone_bn not in BACKBONE_BN_MODES:
            raise ValueError("backbone_bn must be 'running' or 'batch', got {!r}".format(backbone_bn))
        if backbone_bn == "batch" and (compute_dtype != "fp32" or config.model.backbone.type not in ("hrnet_32", "hrnet_48")):
            raise ValueError("backbone_bn='batch' needs an HRNet backbone and compute_dtype='fp32' (got {!r}, {!r})".format(
                config.model.backbone.type, compute_dtype))
        if keypoint_head is not None and (not isinstance(keypoint_head, str) or (keypoint_head not in KP_MODES and keypoint_head != "cpn")):
            raise ValueError("keypoint_head must be None, 'argmax', 'integral' or 'cpn', got {!r}".format(keypoint_head))
        if keypoint_head == "cpn" and config.model.backbone.type != "cpn":
            raise ValueError("keypoint_head='cpn' is the CPN checkpoint's own head (refine_net.final_predict): it needs a CPN backbone, "
                             "got {!r}".format(config.model.backbone.type))
        if not (isinstance(keypoint_beta, (int, float)) and 0.0 < float(keypoint_beta) < float("inf")):
            raise ValueError("keypoint_beta must be a positive finite number, got {!r}".format(keypoint_beta))
        super().__init__()
        self.compute_dtype = compute_dtype
        self.backbone_bn = backbone_bn
        self.keypoint_head_mode = keypoint_head
        self._head = None if keypoint_head is None else _CpnHead if keypoint_head == "cpn" else _FinalLayerHead
        self.keypoint_beta = float(keypoint_beta)
        if backbone_bn == "batch":
            plan_flags |= PLAN_BN_BATCH_STATS
        if keypoint_head == "cpn":
            plan_flags |= PLAN_CPN_PREDICT
        self.plan_flags = plan_flags               # capf.lib.PLAN_* bits: parity tests compare kernel families; 0 = product plan
        self.context_blocks = context_blocks       # False: the MPI-INF-3DHP variant (model/conpose.py)
        self.num_joints = config.model.backbone.num_joints
        self._config = config
        self._backbone_type = config.model.backbone.type
        # schema from a plan-only handle (no GPU needed): names == reference state_dict
        plan = Engine(_native.make_capf_config(config, 256, 192, context_blocks=context_blocks), device=None)
        schema = plan.schema()
        feat0_channels = plan.feature_shapes()[0][2]
        plan.close()
        self.backbone = _native.build_param_tree(_native.Container(), schema, "backbone")
        self.volume_net = _native.build_param_tree(_native.Container(), schema, "volume_net")
        if self._backbone_type == "cpn":
            _native.init_cpn_convs(self.backbone)
        _native.init_deformable_blocks(self.volume_net)
        if keypoint_head in KP_MODES:             # (registered last, and only then: the default module's state_dict is the reference's;
                                                  # "cpn" registers nothing: its head is backbone.refine_net.final_predict)
            self.keypoint_head = KeypointHead(feat0_channels, self.num_joints)

        if config.model.backbone.fix_weights:
            print("model backbone weights are fixed")
            for p in self.backbone.parameters():
                p.requires_grad = False

        self.drop_path_rate = 0.2   # PoseTransformer(drop_path_rate=0.2), dpr = linspace(0, rate, levels) (pose_dformer.py:147,187)
        self.last_flat_grad = None  # flat fp32 gradient of volume_net.* written by the last backward
        # True: backward leaves the gradient in last_flat_grad ONLY and sets no .grad (autograd would clone each of the 191 slices
        # into its parameter's .grad: 191 small device copies per step that a flat optimizer never reads; they overlap the rest of
        # the step -- no measurable change of a 512-frame step, the point is not to materialise a second copy of the gradient)
        self.flat_grad_only = False
        # how forward_features' backward sums the gradient w.r.t. the context maps (capf_set_map_grad_mode): "atomic" (fp32 atomic
        # adds, not bit-reproducible), "ordered" (a fixed summation order, bit-reproducible), or None: ordered when
        # torch.are_deterministic_algorithms_enabled(), else atomic
        self.map_grad_mode = None
        self._engines = {}          # (device index, H, W) -> Engine
        # Parameter-change tracking.  `_generation` counts events that may have replaced parameter STORAGE or frozen
        # (backbone) VALUES: load_state_dict on the model or either child, .to()/._apply, params_changed().  Every engine
        # remembers the generation it last bound at (one shared flag would be cleared by the first engine that rebinds
        # and leave the engines of other input resolutions stale).  volume_net parameters are additionally fingerprinted
        # per call by (data_ptr, _version): optimizer steps bump versions, capf.optim.flatten_ / `p.data = ...` move
        # storage without bumping anything else.
        self._generation = 0
        hook = lambda module, incompatible: self._mark_dirty()
        self.register_load_state_dict_post_hook(hook)
        self.backbone.register_load_state_dict_post_hook(hook)
        self.volume_net.register_load_state_dict_post_hook(hook)

    # ---- parameter-change tracking -----------------------------------------------------------
    def _mark_dirty(self):
        self._generation += 1

    def _apply(self, fn, *args, **kwargs):
        self._generation += 1
        return super()._apply(fn, *args, **kwargs)

    def params_changed(self):
        """Tell the engine that parameter VALUES changed in place where torch cannot see it (manual .data edits
        of backbone weights, an optimizer stepping backbone parameters).  volume_net parameters, load_state_dict and
        .to() are tracked automatically."""
        self._generation += 1

    def lifter_params_changed(self):
        """Call after an in-place update of volume_net VALUES that torch cannot see (capf.optim.FusedAdamW writes
        them from its own kernel); torch optimizers bump tensor versions and are picked up automatically."""
        stream = torch.cuda.current_stream().cuda_stream
        for eng in self._engines.values():
            if eng._bound:
                eng.lifter_params_changed(stream)

    # ---- backbone_bn="batch" ---------------------------------------------------------------------
    def _bn_batch_active(self):
        """This forward normalises with batch statistics: backbone_bn="batch" and the backbone is in train mode."""
        return self.backbone_bn == "batch" and self.backbone.training

    def _backbone_forward_bn(self, eng, images, stream):
        """capf_backbone_forward_bn, and what torch's BatchNorm2d does next to it: num_batches_tracked += 1, on the device.  The running
        statistics moved under every engine's folded packs: each refolds once, before its next running-statistics forward."""
        eng.backbone_forward_bn(images, stream, BN_MOMENTUM)
        with torch.no_grad():
            gen, nbt = self.__dict__.get("_bn_counters", (None, None))
            if gen != self._generation:      # (.to() replaces the buffers: _apply bumps the generation)
                nbt = [b for n, b in self.backbone.named_buffers() if n.endswith("num_batches_tracked")]
                self.__dict__["_bn_counters"] = (self._generation, nbt)
            torch._foreach_add_(nbt, 1)
        for e in self._engines.values():
            e._bn_stale = True

    def _engine(self, images):
        dev = images.device
        _require_cuda(dev)
        B, H, W, C = images.shape
        if C != 3:
            raise ValueError("images must be [B,H,W,3] NHWC")
        return self._engine_at(dev, H, W)

    def _engine_at(self, dev, H, W):
        """The engine of a device and crop size, bound to the module's current parameters."""
        key = (dev.index, H, W)
        eng = self._engines.get(key)
        if eng is None:
            eng = Engine(_native.make_capf_config(self._config, H, W, context_blocks=self.context_blocks,
                                                  compute_dtype=self.compute_dtype, plan_flags=self.plan_flags), device=dev.index)
            eng._bound_generation = None
            eng._lifter_print = None
            eng._bn_stale = False
            self._engines[key] = eng
        lifter = list(self.volume_net.parameters())
        ptrs = tuple(p.data_ptr() for p in lifter)
        versions = tuple(p._version for p in lifter)
        moved = eng._lifter_print is None or eng._lifter_print[0] != ptrs
        if eng._bound_generation != self._generation or moved or not eng._bound:
            # storage may have moved (or frozen values changed): borrow every pointer again, fold + pack everything
            if self.backbone.training and any(p.requires_grad for p in self.backbone.parameters()):
                raise NotImplementedError("training-mode BatchNorm / backbone gradients are outside the hot "
                                          "path: freeze the backbone (fix_weights) and call backbone.eval()")
            state = self.state_dict(keep_vars=True)
            eng._bound = {}
            eng.bind_state({k: v.data for k, v in state.items()}, torch.cuda.current_stream(dev).cuda_stream)
            eng._bound_generation = self._generation
            eng._lifter_print = (ptrs, versions)
            eng._bn_stale = False
            eng.rebinds = getattr(eng, "rebinds", 0) + 1
        elif eng._lifter_print[1] != versions:
            eng.lifter_params_changed(torch.cuda.current_stream(dev).cuda_stream)      # only volume_net values moved (optimizer step)
            eng._lifter_print = (ptrs, versions)
        if eng._bn_stale and not self._bn_batch_active():
            # batch-statistics forwards moved the running statistics: fold them again, once, on leaving train mode
            eng.params_changed(torch.cuda.current_stream(dev).cuda_stream)
            eng._bn_stale = False
        return eng

    # ---- keypoints that take part in the graph ---------------------------------------------------
    def _keypoint_grads(self, keypoints_2d_cpn, keypoints_2d_cpn_crop):
        """True when this call must return gradients w.r.t. a keypoint tensor (grad mode on and one of them requires grad).  The native
        backward has them on fp32 plans only: a 16-bit model refuses here instead of dropping them."""
        need = torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in (keypoints_2d_cpn, keypoints_2d_cpn_crop))
        if need and self.compute_dtype != "fp32":
            raise NotImplementedError("gradients w.r.t. the keypoints need compute_dtype='fp32' (capf_backward_points); this model's "
                                      "compute_dtype is {!r}: detach the keypoint tensors or build the model in fp32".format(self.compute_dtype))
        return need

    @staticmethod
    def _crop_buffer(keypoints_2d_cpn_crop):
        """(the tensor handed on as the third argument, whether the caller's tensor receives the normalised values).  A tensor that does
        not require grad is normalised IN PLACE (conpose.py:34-35; a non-contiguous view through a contiguous staging copy that is
        written back).  One that requires grad is never mutated -- the reference's in-place division would raise on such a leaf: the step
        normalises a private contiguous copy (_private_ref; under no_grad the copy is made here)."""
        t = keypoints_2d_cpn_crop
        if t.requires_grad:
            if not torch.is_grad_enabled():
                return t.detach().clone(memory_format=torch.contiguous_format), False
            return t.contiguous(), False
        return (t if t.is_contiguous() else t.contiguous()), True

    def _lifter_step_params(self, input_grads):
        """[(name, parameter)] of volume_net when this call runs the native training step (None: the plain forward): grad mode on and
        either the lifter trains or an input (a keypoint tensor, a context map) needs its gradient (then with a frozen lifter: no
        parameter gradients)."""
        if not torch.is_grad_enabled():
            return None
        named = [(n, p) for n, p in self.volume_net.named_parameters()]
        if any(p.requires_grad for _, p in named):
            if not all(p.requires_grad for _, p in named):
                raise NotImplementedError("partially frozen volume_net is not supported by the native backward")
            return named
        return [] if input_grads else None

    # ---- what every entry ends in ---------------------------------------------------------------------
    def _image_source(self, images, mode=0):
        """The source record of [B,H,W,3] images: fp32, or uint8 BGR crops with the configured backbone's normalisation constants and
        capf_preprocess's mode."""
        if images.dtype != torch.uint8:
            return _Source("images", images.device, images.shape[0], "images", images)
        mean, std = input_constants("cpn" if self._backbone_type == "cpn" else "hrnet_32")
        return _Source("u8", images.device, images.shape[0] * (2 if mode == 2 else 1), "images", (images, mean, std, mode))

    def _run_lifter(self, eng, src, k2d, kcrop, named):
        """The native training step on `named` (_lifter_step_params) or, with None, the plain call; returns joints3d [B,1,J,3]."""
        if named is None:
            out = torch.empty(src.batch, 1, self.num_joints, 3, dtype=torch.float32, device=src.device)
            _run_source(self, eng, src, k2d, kcrop, out, torch.cuda.current_stream(src.device).cuda_stream, False)
            return out
        names = tuple("volume_net." + n for n, _ in named)
        maps = src.data if src.kind == "maps" else ()
        return _LifterStep.apply(self, eng, src, k2d, kcrop, self._drop_masks(src.batch, src.device), names, len(maps), *maps,
                                 *[p for _, p in named])

    def _lift(self, src, crop_size, keypoints_2d_cpn, keypoints_2d_cpn_crop, input_grads):
        """The shared end of forward / forward_u8 / forward_features: the keypoint checks, the engine of crop_size = (H, W), the lifter
        on the source's maps as a training step or a plain call, and the normalised crop keypoints written back."""
        B, dev = src.batch, src.device
        for name, t in (("keypoints_2d_cpn", keypoints_2d_cpn), ("keypoints_2d_cpn_crop", keypoints_2d_cpn_crop)):
            if t.dtype != torch.float32:
                raise TypeError("{} must be float32, got {}".format(name, t.dtype))
            if t.device != dev:
                raise ValueError("{} is on {} but {} are on {}".format(name, t.device, src.word, dev))
            if tuple(t.shape) != (B, self.num_joints, 2):
                pair = src.kind == "u8" and src.data[3] == 2
                raise ValueError("{} must have shape ({}, {}, 2){}, got {}".format(
                    name, B, self.num_joints, " for mirror='pair' (two sets of {} frames)".format(B // 2) if pair else "", tuple(t.shape)))
        with torch.cuda.device(dev):
            eng = self._engine(src.data) if crop_size is None else self._engine_at(dev, *crop_size)
            k2d = keypoints_2d_cpn.contiguous()
            # the third argument is normalised IN PLACE (conpose.py:34-35); a non-contiguous view (which the reference
            # accepts) goes through a contiguous staging copy that is written back
            kcrop, write_back = self._crop_buffer(keypoints_2d_cpn_crop)
            out = self._run_lifter(eng, src, k2d, kcrop, self._lifter_step_params(input_grads))
            if write_back and kcrop is not keypoints_2d_cpn_crop:
                with torch.no_grad():
                    keypoints_2d_cpn_crop.copy_(kcrop)
        return out

    # ---- conpose.py:30-42 --------------------------------------------------------------------
    def forward(self, images, keypoints_2d_cpn, keypoints_2d_cpn_crop):
        """conpose.py:30-42.  The third argument is normalised in place (conpose.py:34-35) unless it requires grad: then it is left
        untouched, a private contiguous copy is normalised, and its .grad is w.r.t. the pixel values passed.  With grad enabled,
        gradients reach volume_net's parameters and any keypoint tensor that requires grad (fp32 models; 16-bit: NotImplementedError)."""
        kp_grads = self._keypoint_grads(keypoints_2d_cpn, keypoints_2d_cpn_crop)
        if images.dtype != torch.float32:
            raise TypeError("images must be float32")
        _require_cuda(images.device)
        images = images.contiguous()
        # (crop size None: _engine reads it off the images, with its [B,H,W,3] refusal behind the keypoint checks)
        return self._lift(_Source("images", images.device, images.shape[0], "images", images), None,
                          keypoints_2d_cpn, keypoints_2d_cpn_crop, kp_grads)

    # ---- the same forward from uint8 crops: normalisation, BGR flip and mirror in the stem conv's load (capf_forward_u8) ----------
    def forward_u8(self, images_u8, keypoints_2d_cpn, keypoints_2d_cpn_crop, mirror="none"):
        """forward() on the uint8 BGR crops themselves: images_u8 is a contiguous uint8 CUDA tensor [B,H,W,3] as the loader / the crop
        decoder delivers it; no fp32 image is materialised.  Mean and std are the configured backbone's, as data_prefetcher picks them
        (datasets/utils.py:24-29, 45-50).  mirror: "none" -- as is; "all" -- every frame mirrored (the train-time flip, :55-56);
        "pair" -- the flip test (:67-68): 2B engine frames, the B crops followed by their mirrors; the keypoints are then [2B,17,2] in
        capf_preprocess mode 2's layout ([2,B,17,2] flattened: capf.lib.preprocess_points) and the result is [2B,1,17,3].  The keypoints
        are NOT mirrored here (preprocess_points does that); the third argument is normalised in place like forward's.  Under grad the
        native training step runs.  Every result bit equals forward() on capf.lib.preprocess()'s images."""
        if not isinstance(mirror, str) or mirror not in MIRROR_MODES:
            raise ValueError("mirror must be 'none', 'all' or 'pair', got {!r}".format(mirror))
        mode = MIRROR_MODES[mirror]
        kp_grads = self._keypoint_grads(keypoints_2d_cpn, keypoints_2d_cpn_crop)
        if self._bn_batch_active():
            raise NotImplementedError("forward_u8 has no batch-statistics route (backbone_bn='batch' with the backbone in train mode): "
                                      "call backbone.eval(), or forward() on capf.lib.preprocess()'s fp32 images")
        if not torch.is_tensor(images_u8) or images_u8.dtype != torch.uint8:
            raise TypeError("images_u8 must be uint8, got {}".format(getattr(images_u8, "dtype", type(images_u8))))
        _require_cuda(images_u8.device)
        if images_u8.dim() != 4 or images_u8.shape[3] != 3:
            raise ValueError("images_u8 must be [B,H,W,3] NHWC, got {}".format(tuple(images_u8.shape)))
        if not images_u8.is_contiguous():
            raise ValueError("images_u8 must be contiguous (a copy would be the image round trip this entry removes)")
        return self._lift(self._image_source(images_u8, mode), images_u8.shape[1:3], keypoints_2d_cpn, keypoints_2d_cpn_crop, kp_grads)

    # ---- detector-free: the 2-D keypoints from the native head on feat0 -------------------------
    def _head_record(self):
        if self._head is None:
            raise CapfError("this model has no keypoint head: build it with keypoint_head='argmax', 'integral' or 'cpn'")
        return self._head

    def _head_params(self):
        self._head_record()
        fl = self.keypoint_head.final_layer
        return fl.weight, fl.bias

    def _head_trains(self):
        """True when this call must produce gradients of the head's parameters; refuses what the native backward does not cover."""
        weight, bias = self._head_params()
        if not (torch.is_grad_enabled() and (weight.requires_grad or bias.requires_grad)):
            return False
        if self.keypoint_head_mode != "integral":
            raise NotImplementedError("the argmax keypoint head has no derivative: build the model with keypoint_head='integral', or freeze "
                                      "keypoint_head's parameters (requires_grad_(False)) / call under torch.no_grad()")
        if self.compute_dtype != "fp32":
            raise NotImplementedError("gradients of the keypoint head need compute_dtype='fp32' (capf_kp_head_backward, capf_backward_points); "
                                      "this model's compute_dtype is {!r}: freeze keypoint_head's parameters, call under torch.no_grad() or "
                                      "build the model in fp32".format(self.compute_dtype))
        return True

    def _detect_inputs(self, images, to_image):
        if not torch.is_tensor(images) or images.dtype not in (torch.float32, torch.uint8):
            raise TypeError("images must be float32 or uint8, got {}".format(getattr(images, "dtype", type(images))))
        _require_cuda(images.device)
        if images.dim() != 4 or images.shape[3] != 3:
            raise ValueError("images must be [B,H,W,3] NHWC, got {}".format(tuple(images.shape)))
        if images.dtype == torch.uint8 and self._bn_batch_active():
            raise NotImplementedError("uint8 images have no batch-statistics route (backbone_bn='batch' with the backbone in train mode): "
                                      "call backbone.eval(), or pass capf.lib.preprocess()'s fp32 images")
        B = images.shape[0]
        if to_image is not None:
            if not torch.is_tensor(to_image) or to_image.dtype != torch.float32 or tuple(to_image.shape) != (B, 2, 3):
                raise ValueError("to_image must be a float32 tensor [{}, 2, 3] (capf.lib.crop_to_image_matrix per frame), got {}".format(
                    B, tuple(getattr(to_image, "shape", ()))))
            if to_image.device != images.device:
                raise ValueError("to_image is on {} but images are on {}".format(to_image.device, images.device))
            to_image = to_image.detach().contiguous()
        return images.contiguous(), to_image

    # ---- the two detect flows: everything head-specific is in self._head (_FinalLayerHead / _CpnHead) ---------------------------
    def _lift_workspace(self, eng, dev, batch, k2d, ref, named):
        """The lifter on the maps the backbone pass of this call left in the workspace (_run_lifter's `named`)."""
        return self._run_lifter(eng, _Source("workspace", dev, batch, "the maps", None), k2d, ref, named)

    def _single_flow(self, images, to_image, lift, trains):
        """detect / forward_detect: inputs, engine, ONE backbone pass (no gradient reaches it), the head on its workspace tensor; with
        `lift` the lifter on the maps still in the workspace, as a training step when the lifter or the head (`trains`) needs gradients,
        and the token that lets the head's backward refuse a workspace a later run has overwritten."""
        head = self._head
        images, to_image = self._detect_inputs(images, to_image)
        dev, B, H, W = images.device, images.shape[0], images.shape[1], images.shape[2]
        with torch.cuda.device(dev):
            eng = self._engine_at(dev, H, W)
            named = self._lifter_step_params(trains) if lift else None
            with torch.no_grad():
                _run_backbone(self, eng, self._image_source(images), torch.cuda.current_stream(dev).cuda_stream)
                maps = eng.tensor_view(head.maps, B)
            kcrop, score, k2d, guard = head.single(self, eng, maps, head.decode(H, W, maps.shape[1], maps.shape[2]), to_image, trains)
            if not lift:
                return kcrop, score, k2d
            # (a crop-keypoint tensor outside the graph would be normalised in place by the lifter: it gets a copy, the caller the pixels)
            ref = kcrop.detach().clone() if named is None else kcrop if kcrop.requires_grad else kcrop.clone()
            out = self._lift_workspace(eng, dev, B, k2d, ref, named)
            if named is not None and guard is not None:
                guard["token"] = eng.train_generation()
        return out, kcrop, score

    def _pair_flow(self, images, to_image, flip_pairs, lift, **head_args):
        """The four flip entries, always without grad: the 2B engine frames [orig | mirrored], engine, ONE backbone pass over them, the
        paired head (head_args: what only one head's pair takes -- HRNet's shift); with `lift` the lifter on the maps still in the
        workspace with the stacked keypoints the head wrote, and capf_fliptest_fuse."""
        head, J = self._head, self.num_joints
        swap = self._swap_table(flip_pairs)
        src, B, H, W, to_image = self._flip_test_source(images, to_image)
        with torch.cuda.device(src.device), torch.no_grad():
            eng = self._engine_at(src.device, H, W)
            _run_backbone(self, eng, src, torch.cuda.current_stream(src.device).cuda_stream)
            maps = eng.tensor_view(head.maps, src.batch)
            kcrop2, score, k2d2 = head.pair(self, maps, head.decode(H, W, maps.shape[1], maps.shape[2]), to_image, swap, **head_args)
            if not lift:
                return kcrop2[0], score, (None if k2d2 is None else k2d2[0])
            ref = kcrop2.clone().view(2 * B, J, 2)               # (the lifter normalises its crop keypoints in place: the caller keeps the pixels)
            pred = self._lift_workspace(eng, src.device, 2 * B, k2d2.view(2 * B, J, 2), ref, None)
            out = fliptest_fuse(pred.view(2, B, 1, J, 3), swap)
        return out, kcrop2[0], score

    # ---- keypoint_head="cpn": the checkpoint's own final_predict (run by the backbone pass) and CPN's two-peak decode -------------
    def _cpn_head_frozen(self):
        """The head is part of the frozen backbone and has no derivative: a final_predict parameter that asks for a gradient is refused
        as forward refuses backbone gradients."""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.backbone.refine_net.final_predict.parameters()):
            raise NotImplementedError("gradients of refine_net.final_predict are outside the hot path (keypoint_head='cpn' has no derivative): "
                                      "freeze the backbone (fix_weights) or call under torch.no_grad()")

    def _no_cpn_flip_test(self):
        if self.keypoint_head_mode == "cpn":
            raise NotImplementedError("keypoint_head='cpn' is not served by HRNet's shifted flip test (CPN's own test-time flip averages the "
                                      "heatmaps without a column shift): use detect_cpn_flip / forward_detect_cpn_flip")

    def _cpn_flip_entry(self, name):
        if self.keypoint_head_mode != "cpn":
            raise ValueError("{} is CPN's test-time flip: it needs CA_PF(..., keypoint_head='cpn'), not keypoint_head={!r} (HRNet's flip "
                             "test: detect_flip_test / forward_detect_flip_test)".format(name, self.keypoint_head_mode))
        self._cpn_head_frozen()

    def detect(self, images, to_image=None):
        """The 2-D keypoints of the crops from the native head: backbone (one pass), final_layer on feat0 and the heatmap decode.
        images: [B,H,W,3] float32 (normalised, as forward takes them) or uint8 BGR crops (as forward_u8 takes them; the same bits).
        to_image: None, or float32 [B, 2, 3] -- per frame the matrix capf.lib.crop_to_image_matrix builds from the crop's center / scale
        and the camera resolution.  Returns (kcrop_px [B,J,2] in crop pixels, score [B,J], k2d [B,J,2] normalised image coordinates or
        None): what forward() takes as its third and second argument.  No gradients (see forward_detect).
        keypoint_head="cpn": the backbone pass runs final_predict too and capf_cpn_decode decodes its heatmaps; score is CPN's
        r0 = heatmap / 255 + 0.5 at the keypoint."""
        self._head_record()
        with torch.no_grad():
            return self._single_flow(images, to_image, False, False)

    def forward_detect(self, images, to_image):
        """forward() without detections from outside: ONE backbone pass, the keypoint head on feat0, the lifter on the maps still in the
        workspace.  Returns (joints3d [B,1,J,3], kcrop_px [B,J,2], score [B,J]); kcrop_px stays in crop pixels (the lifter normalises a
        private copy).  The result equals forward(images, k2d, kcrop_px) on detect()'s keypoints bit for bit.
        With grad enabled the lifter trains as in forward(), and an "integral" head whose parameters require grad trains THROUGH the
        lifter (fp32 models): the backbone runs once without grad, the head is its own autograd node, capf_backward_points hands it
        dL/d(k2d) and dL/d(crop keypoints), capf_kp_head_backward turns them into final_layer.weight.grad (bias.grad is exactly 0: softmax
        ignores a shift).  A loss on kcrop_px itself (KeypointsMSELoss against 2-D labels) trains the head too.  The backward re-reads feat0
        from the workspace (the lifter's training forward and backward only read the maps): run it before the next forward of this model.
        An "argmax" head with trainable parameters, or a 16-bit model with a trainable head, raises under grad instead of dropping the
        gradients.
        keypoint_head="cpn": final_predict and capf_cpn_decode take the head's place; the head has no derivative (a final_predict
        parameter that requires grad raises under grad), the lifter trains as in forward()."""
        trains = self._head_record().trains(self)
        if to_image is None:
            raise ValueError("forward_detect needs to_image [B, 2, 3]: the lifter takes the keypoints in normalised image coordinates too")
        return self._single_flow(images, to_image, True, trains)

    def keypoint_loss(self, images, keypoints_2d_crop, target_weight=None, sigma=2.0, reduction="mean", topk=8, return_accuracy=False):
        """Heatmap supervision of the native head against 2-D ground truth: ONE backbone pass (no gradient reaches it), then
        capf_kp_heatmap_loss on feat0 -- final_layer's 1x1 conv, Gaussian targets of `sigma` heatmap cells around keypoints_2d_crop [B,J,2]
        (crop pixels, what detect() returns as kcrop_px; the heatmap <-> crop convention is detect()'s), HRNet's JointsMSELoss
        (reduction "mean") or JointsOHKMMSELoss ("ohkm", the `topk` hardest joints of each frame) with per-joint target_weight [B,J],
        and its gradients, in one native call.  images: detect()'s forms (float32 or uint8 BGR crops).  Returns the 0-d loss; backward()
        leaves gradients in keypoint_head.final_layer.weight / .bias and nowhere else.  This is how an "argmax" head is trained (its decode
        has no derivative) and the only path that moves final_layer.bias; it serves "integral" models and every compute dtype alike.
        return_accuracy=True: returns (loss, acc) -- the same loss and the same gradients, bit for bit, and acc, a 0-d float64 device
        tensor without gradient: the PCK of this model's own decode on the feat0 the loss just read, the figure HRNet's training loop
        logs beside the loss, taken on decoded keypoints.  No second backbone pass, no host synchronisation: capf_kp_head_forward in the
        model's mode writes kcrop_px (detect()'s bits), capf_pck2d_counts compares it with keypoints_2d_crop under norm = (W / 10, H / 10)
        of the crop (as fp32) for every pose, strict `<`, the single threshold 0.5 and weight = target_weight, and acc is the mean over
        the joints with a valid sample of counts / valid (NaN if no joint has one).
        keypoint_head=None: CapfError; "cpn": NotImplementedError (that head belongs to the frozen backbone)."""
        head = self._head_record()
        if head is not _FinalLayerHead:
            raise NotImplementedError("keypoint_loss trains keypoint_head.final_layer: keypoint_head='cpn' has none (refine_net.final_predict "
                                      "belongs to the frozen backbone)")
        if not isinstance(reduction, str) or reduction not in KP_LOSS_REDUCTIONS:
            raise ValueError("reduction must be 'mean' or 'ohkm', got {!r}".format(reduction))
        images, _ = self._detect_inputs(images, None)
        dev, B, H, W = images.device, images.shape[0], images.shape[1], images.shape[2]
        if not torch.is_tensor(keypoints_2d_crop) or tuple(keypoints_2d_crop.shape) != (B, self.num_joints, 2):
            raise ValueError("keypoints_2d_crop must be a tensor [{}, {}, 2] in crop pixels, got {}".format(
                B, self.num_joints, tuple(getattr(keypoints_2d_crop, "shape", ()))))
        weight, bias = self._head_params()
        with torch.cuda.device(dev):
            eng = self._engine_at(dev, H, W)
            with torch.no_grad():
                _run_backbone(self, eng, self._image_source(images), torch.cuda.current_stream(dev).cuda_stream)
                feat0 = eng.tensor_view(head.maps, B)
            decode = head.decode(H, W, feat0.shape[1], feat0.shape[2])
            gt, tw = keypoints_2d_crop.to(dev), None if target_weight is None else target_weight.to(dev)
            loss = keypoint_heatmap_loss(feat0, weight, bias, gt, tw, decode, sigma, reduction, topk)
            if not return_accuracy:
                return loss
            with torch.no_grad():
                return loss, self._decode_accuracy(feat0, weight, bias, decode, gt, tw, H, W)

    @staticmethod
    def _accuracy_norm(B, H, W, device):
        """capf_pck2d_counts' norm for B crops of H rows x W columns: (nx, ny) = (W / 10, H / 10) per pose, x over the width; filled on the
        device (no host-to-device copy)"""
        norm = torch.empty(B, 2, dtype=torch.float32, device=device)
        norm[:, 0] = W / 10.0
        norm[:, 1] = H / 10.0
        return norm

    def _decode_accuracy(self, feat0, weight, bias, decode, gt, tw, H, W, threshold=0.5):
        """keypoint_loss's accuracy figure (its docstring has the rule); everything stays on the device"""
        B, J = gt.shape[0], gt.shape[1]
        kcrop, _, _, _ = kp_head_forward(feat0, weight.detach(), None if bias is None else bias.detach(), KP_MODES[self.keypoint_head_mode],
                                         self.keypoint_beta, decode, None, want_score=False)
        counts, valid, _ = pck2d_counts(kcrop, gt.detach().to(torch.float32).contiguous(), (threshold,), norm=self._accuracy_norm(B, H, W, gt.device),
                                        weight=None if tw is None else tw.detach().to(torch.float32).reshape(B, J).contiguous(), strict=True)
        seen = valid[0] > 0
        rate = torch.where(seen, counts[0, 0].to(torch.float64) / valid[0].clamp(min=1).to(torch.float64), torch.zeros((), dtype=torch.float64, device=gt.device))
        return rate.sum() / seen.sum()                          # (0 / 0 = NaN: no joint has a valid sample)

    # ---- detector-free flip test: the heatmaps of each crop and of its flipped-back mirror averaged, then decoded once -----------
    def _swap_table(self, flip_pairs):
        """flip_pairs -> the J-entry swap table of capf_kp_head_forward_pair / capf_fliptest_fuse_swap (capf.lib.MPI_SWAP's form: entry j names
        the joint that the mirror exchanges with joint j); None stays None: the H36M table, which both entries then apply themselves."""
        if flip_pairs is None:
            return None
        table = [int(v) for v in flip_pairs]
        if len(table) != self.num_joints or any(not 0 <= v < len(table) or table[v] != j for j, v in enumerate(table)):
            raise ValueError("flip_pairs must be a table of {} joint indices that is its own inverse (capf.lib.H36M_SWAP, MPI_SWAP), got {!r}".format(
                self.num_joints, flip_pairs))
        return tuple(table)

    def _flip_test_source(self, images, to_image):
        """(source record of the 2B engine frames [orig | mirrored], B, H, W, to_image) for detect_flip_test / forward_detect_flip_test."""
        if self._bn_batch_active():
            raise NotImplementedError("the flip test has no batch-statistics route (backbone_bn='batch' with the backbone in train mode): the "
                                      "2B-frame pair would change every frame's statistics -- call backbone.eval()")
        if torch.is_tensor(images) and images.dim() == 5:        # the [2,B,H,W,3] stack capf_preprocess(mode=2) emits
            if images.dtype != torch.float32 or images.shape[0] != 2:
                raise TypeError("a 5-D images tensor must be the float32 [2,B,H,W,3] stack of capf.lib.preprocess(mode=2), got {} {}".format(
                    tuple(images.shape), images.dtype))
            first, to_image = self._detect_inputs(images[0], to_image)
            pair = images.contiguous().view(-1, *images.shape[2:])
            src = _Source("images", pair.device, pair.shape[0], "images", pair)
        else:
            first, to_image = self._detect_inputs(images, to_image)
            if first.dtype == torch.uint8:                       # mirrored in the stem conv's load: no mirrored image is built
                src = self._image_source(first, 2)
            else:
                pair = torch.cat([first, torch.flip(first, [2])])
                src = _Source("images", pair.device, pair.shape[0], "images", pair)
        return src, first.shape[0], first.shape[1], first.shape[2], to_image

    def detect_flip_test(self, images, to_image=None, shift=True, flip_pairs=None):
        """detect() under HRNet's flip test: ONE backbone pass over the crops and their mirrors, then capf_kp_head_forward_pair -- per joint
        the heatmap of the crop and the flipped-back heatmap of the mirror (x mirrored, left / right joints exchanged, moved one column to
        the right when `shift`, HRNet's SHIFT_HEATMAP) are averaged and decoded once.  images: uint8 BGR crops [B,H,W,3] (mirrored in the
        stem's load), float32 [B,H,W,3] (the mirrored half is torch.flip(images, [2])), or the float32 [2,B,H,W,3] stack of
        capf.lib.preprocess(mode=2) -- the same bits.  to_image as in detect.  flip_pairs: None -- the H36M table -- or a swap table of J ints
        (capf.lib.MPI_SWAP).  Returns (kcrop_px [B,J,2], score [B,J], k2d [B,J,2] | None).  Always runs without
        grad and returns detached tensors: the paired decode has no backward.  keypoint_head="cpn": NotImplementedError."""
        self._no_cpn_flip_test()
        self._head_record()
        return self._pair_flow(images, to_image, flip_pairs, False, shift=shift)

    def forward_detect_flip_test(self, images, to_image, shift=True, flip_pairs=None):
        """The reference's flip-test evaluation (train.py:170-181) without detections from outside: ONE backbone pass over the 2B engine
        frames, the paired head (detect_flip_test; images / shift / flip_pairs as there), the lifter on the maps still in the workspace with
        the stacked keypoints the head wrote (set 1 mirrored as capf_preprocess_points(mode=2) does), capf_fliptest_fuse (its _swap form with
        flip_pairs).  Returns (joints3d [B,1,J,3], kcrop_px [B,J,2], score [B,J]); kcrop_px stays in crop pixels.  The result equals
        forward_flip_test on the stack with detect_flip_test's keypoints pushed through preprocess_points(mode=2), bit for bit.  Always runs
        without grad and returns detached tensors.  keypoint_head="cpn": NotImplementedError."""
        self._no_cpn_flip_test()
        self._head_record()
        if to_image is None:
            raise ValueError("forward_detect_flip_test needs to_image [B, 2, 3]: the lifter takes the keypoints in normalised image coordinates too")
        return self._pair_flow(images, to_image, flip_pairs, True, shift=shift)

    # ---- keypoint_head="cpn" under CPN's own test-time flip (cpn/test.py:44-70): fold of the two heatmaps, ONE two-peak decode ----
    def detect_cpn_flip(self, images, to_image=None, flip_pairs=None):
        """detect() under CPN's own test-time flip (cpn/test.py:44-70, upstream's default and the procedure behind keypoints_2d_cpn): ONE
        backbone pass over the crops and their mirrors, then capf_cpn_decode_pair -- per joint the heatmap of the crop and the heatmap of
        the mirror (x mirrored back, left / right joints exchanged, NO column shift) are averaged and decoded once with CPN's two-peak
        rule.  keypoint_head="cpn" only (anything else: ValueError).  images: the three forms of detect_flip_test -- uint8 BGR crops
        [B,H,W,3] (mirrored in the stem's load), float32 [B,H,W,3] (the mirrored half is torch.flip(images, [2])), or the float32
        [2,B,H,W,3] stack of capf.lib.preprocess(mode=2) -- the same bits.  to_image as in detect.  flip_pairs: None -- the H36M table -- or a
        swap table of J ints (capf.lib.COCO_SWAP for a checkpoint whose channels are in COCO order).  Returns (kcrop_px [B,J,2],
        score [B,J], k2d [B,J,2] | None).  Always runs without grad and returns detached tensors: the decode has no backward (a
        final_predict parameter that requires grad raises under grad)."""
        self._cpn_flip_entry("detect_cpn_flip")
        return self._pair_flow(images, to_image, flip_pairs, False)

    def forward_detect_cpn_flip(self, images, to_image, flip_pairs=None):
        """The reference's flip-test evaluation (train.py:170-181) on a CPN backbone without detections from outside, from crop to
        flip-tested 3-D pose in ONE backbone pass over the 2B engine frames: the paired decode (detect_cpn_flip; images / flip_pairs as
        there), the lifter on the maps still in the workspace with the stacked keypoints the kernel wrote (set 1 mirrored as
        capf_preprocess_points(mode=2) does), capf_fliptest_fuse (its _swap form with flip_pairs).  Returns (joints3d [B,1,J,3],
        kcrop_px [B,J,2], score [B,J]); kcrop_px stays in crop pixels.  The result equals forward_flip_test on the stack with
        detect_cpn_flip's keypoints pushed through preprocess_points(mode=2), bit for bit.  Always runs without grad and returns detached
        tensors."""
        self._cpn_flip_entry("forward_detect_cpn_flip")
        if to_image is None:
            raise ValueError("forward_detect_cpn_flip needs to_image [B, 2, 3]: the lifter takes the keypoints in normalised image coordinates too")
        return self._pair_flow(images, to_image, flip_pairs, True)

    # ---- conpose.py:40 on maps of the caller's own backbone ------------------------------------
    def _feature_geometry(self, H, W):
        """[(H_l, W_l, C_l)] of the four context maps at crop size H x W, from a plan-only handle (no GPU needed)."""
        cache = self.__dict__.setdefault("_feature_geometries", {})
        if (H, W) not in cache:
            plan = Engine(_native.make_capf_config(self._config, H, W, context_blocks=self.context_blocks), device=None)
            cache[(H, W)] = plan.feature_shapes()
            plan.close()
        return cache[(H, W)]

    def forward_features(self, features_list, keypoints_2d_cpn, keypoints_2d_cpn_crop):
        """self.volume_net(keypoints_2d_cpn, keypoints_2d_cpn_crop, features_list) (conpose.py:34-40) on context maps the CALLER
        computed: four fp32 CUDA tensors, NCHW as the reference backbones return them (pose_hrnet.py:501, networks/network.py:16-22),
        of the configured backbone's geometry at crop size (4 H_0, 4 W_0).  Returns [B,1,17,3]; the third argument is normalised in
        place exactly as forward does.  With grad enabled, gradients flow into volume_net's parameters AND into every map that
        requires grad (capf_backward_maps), so a torch backbone in front of the native lifter trains through it; the native backbone
        is not run.  self.map_grad_mode picks how the map gradients are summed: "atomic" -- fp32 atomic adds, equal up to fp32 summation
        order from run to run; "ordered" -- one fixed expression (include/capf.h, capf_set_map_grad_mode), bit-identical from run to
        run; None (default) -- ordered under torch.use_deterministic_algorithms(True), otherwise atomic.  Anything else: ValueError.
        The parameter gradients have the same bits in both.  A keypoint tensor that requires grad receives its gradient too
        (capf_backward_points: a keypoint head on the same backbone trains through the lifter); the third argument is then NOT
        mutated -- a private contiguous copy is normalised -- and its gradient is w.r.t. the pixel values passed."""
        resolve_map_grad_mode(self.map_grad_mode)
        kp_grads = self._keypoint_grads(keypoints_2d_cpn, keypoints_2d_cpn_crop)
        feats = list(features_list)
        if len(feats) != 4:
            raise ValueError("features_list must hold 4 context maps, got {}".format(len(feats)))
        for l, f in enumerate(feats):
            if not torch.is_tensor(f) or f.dim() != 4:
                raise ValueError("features_list[{}] must be a [B,C,H,W] tensor".format(l))
        B, H, W = feats[0].shape[0], 4 * feats[0].shape[2], 4 * feats[0].shape[3]
        try:
            geometry = self._feature_geometry(H, W)
        except CapfError as e:
            raise ValueError("no {} plan at crop size {}x{} (features_list[0] is {}): {}".format(
                self._backbone_type, H, W, tuple(feats[0].shape), e))
        want = ", ".join("[B,{},{},{}]".format(c, h, w) for h, w, c in geometry)
        for l, (f, (h, w, c)) in enumerate(zip(feats, geometry)):
            if tuple(f.shape) != (B, c, h, w):
                raise ValueError("features_list[{}] has shape {}; the {} maps at crop size {}x{} are NCHW {} with one B".format(
                    l, tuple(f.shape), self._backbone_type, H, W, want))
            if f.dtype != torch.float32:
                raise ValueError("features_list[{}] must be float32, got {} (maps are NCHW {})".format(l, f.dtype, want))
            if f.device != feats[0].device:
                raise ValueError("features_list[{}] is on {} but features_list[0] is on {} (maps are NCHW {})".format(
                    l, f.device, feats[0].device, want))
        dev = feats[0].device
        _require_cuda(dev)
        map_grads = torch.is_grad_enabled() and any(f.requires_grad for f in feats)
        nhwc = [f.permute(0, 2, 3, 1).contiguous() for f in feats]
        return self._lift(_Source("maps", dev, B, "the maps", nhwc), (H, W), keypoints_2d_cpn, keypoints_2d_cpn_crop, kp_grads or map_grads)

    def _drop_masks(self, B, device):
        """DropPath multipliers for one training step (timm semantics: keep-mask / keep_prob per sample;
        a 'sample' is one batch element for context / joint blocks and one (frame, joint) row group for the
        level blocks, whose batch axis is (b p) — pose_dformer.py:231-234).  None when nothing is dropped.
        Layout (include/capf.h, capf_forward_train): ctx | res | joint, `levels` blocks each, rates linspace(0, rate, levels)
        (pose_dformer.py:187); without context blocks res | joint only, `depth` blocks each, res block i and joint block i sharing
        rate i of linspace(0, rate, depth) (ContextPose_mpi/model/pose_dformer.py:215)."""
        pf = self._config.model.poseformer
        if not self.training or self.drop_path_rate <= 0.0:
            return None
        if self.context_blocks:
            rates, pers = torch.linspace(0, self.drop_path_rate, pf.levels).tolist(), (B, B * self.num_joints, B)
        else:
            rates, pers = torch.linspace(0, self.drop_path_rate, int(getattr(pf, "depth", pf.levels))).tolist(), (B * self.num_joints, B)
        parts = []
        for per in pers:
            for r in rates:
                for _ in range(2):
                    if r == 0.0:
                        parts.append(torch.ones(per, device=device))
                    else:
                        keep = 1.0 - r
                        parts.append(torch.empty(per, device=device).bernoulli_(keep).div_(keep))
        return torch.cat(parts).contiguous()

    def forward_flip_test(self, images2, keypoints_2d_cpn2, keypoints_2d_cpn_crop2):
        """Flip-test evaluation (train.py:170-181) as ONE forward: inputs are the [2,B,...] stacks that
        capf_preprocess(mode=2) emits (original, mirrored); the two predictions are un-mirrored and averaged
        by capf_fliptest_fuse.  Returns [B,1,17,3].  The crop keypoints are normalised in place."""
        two, B = images2.shape[0], images2.shape[1]
        assert two == 2 and images2.is_contiguous() and keypoints_2d_cpn_crop2.is_contiguous()
        pred = self.forward(images2.view(2 * B, *images2.shape[2:]), keypoints_2d_cpn2.reshape(2 * B, 17, 2),
                            keypoints_2d_cpn_crop2.view(2 * B, 17, 2))
        return fliptest_fuse(pred.view(2, B, 1, 17, 3))

    def engine_for(self, images):
        """The native engine serving inputs of this shape/device (tests, bench)."""
        return self._engine(images.contiguous())
