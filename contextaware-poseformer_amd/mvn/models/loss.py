"""Losses and metrics the path's callers import (`from mvn.models.loss import MPJPE, KeypointsMSELoss,
KeypointsMSESmoothLoss, KeypointsMAELoss`, ContextPose/train.py:21; P_MPJPE / N_MPJPE / MPJVE,
ContextPose/mvn/datasets/human36m.py:365-368).  Same class names, argument meaning and return kinds as
ContextPose/mvn/models/loss.py; the arithmetic runs in libcapf.so (capf_mpjpe, capf_pose_errors, capf_segment_sums,
capf_keypoints_loss, capf_keypoints_l2_loss, capf_limb_length_errors, capf_limb_length_sums, capf_uncertainty_loss).  No torch /
numpy compute and no CPU fallback: numpy arguments (the reference hands `.cpu().numpy()` arrays to P_MPJPE and MPJVE) are uploaded,
reduced on the GPU and returned as numpy scalars.

Every pose loss of the reference module is here: KeypointsL2Loss (loss.py:140-147), LimbLengthError (:181-201) and the function
UNCERTAINTY (:7-13) beside the ones above.  (VolumetricCELoss, :150-178, belongs to the volumetric model this reference no longer has.)
Their gradients are defined everywhere: 0 where a norm or square root they divide by is 0 (a masked row, pred == gt, coincident joints),
where the reference's torch.sqrt gives NaN.  limb_length_loss is LimbLengthError as a differentiable 0-d tensor: the reference class returns a
Python float and cannot serve as a loss."""
import ctypes

import numpy as np
import torch
from torch import nn


def _cuda(x):
    """numpy array or tensor -> contiguous fp32 CUDA tensor (device of the tensor, else the current device)."""
    if isinstance(x, np.ndarray):
        return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).cuda()
    if not x.is_cuda:
        from capf.lib import CapfError
        raise CapfError("metrics run on the MI355X only: got a CPU tensor (pass a CUDA tensor or a numpy array)")
    return x.detach().to(torch.float32).contiguous()


def _poses(x):
    t = _cuda(x)
    return t.reshape(-1, t.shape[-2], 3)


class _MPJPEFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt):
        from capf.lib import load_library
        lib = load_library()
        pred_c, gt_c = pred.contiguous(), gt.contiguous()
        dim = pred_c.shape[-1]
        rows = pred_c.numel() // dim
        loss = torch.empty(1, dtype=torch.float32, device=pred.device)
        # the loss depends on pred - gt alone: one buffer serves both gradients (dloss/dgt = -dloss/dpred, as autograd gives the reference's
        # torch.norm(keypoints_pred - keypoints_gt, dim=-1), loss.py:22)
        dpred = torch.empty(pred_c.shape, dtype=torch.float32, device=pred.device) if any(ctx.needs_input_grad[:2]) else None
        stream = ctypes.c_void_p(torch.cuda.current_stream(pred.device).cuda_stream)
        P = lambda t: ctypes.c_void_p(t.data_ptr() if t is not None else 0)
        if dim == 3:
            rc = lib.capf_mpjpe(stream, P(pred_c), P(gt_c), rows, P(loss), P(dpred), 1.0)
        else:
            rc = lib.capf_mpjpe_nd(stream, P(pred_c), P(gt_c), rows, dim, P(loss), P(dpred), 1.0)
        if rc:
            raise RuntimeError(f"capf_mpjpe failed ({rc})")
        ctx.dpred = dpred
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        d = ctx.dpred * g
        return (d if ctx.needs_input_grad[0] else None), (-d if ctx.needs_input_grad[1] else None)


class MPJPE(nn.Module):
    """loss.py:16-22: mean over every leading axis of ||pred - gt||_2 along the last one (any width: 3-D joints, 2-D keypoints).
    CUDA tensors only — there is no CPU fallback; other float dtypes are computed in fp32 and the loss is cast back to the inputs' dtype.
    Differentiable in both arguments, like the reference's expression: a target that requires grad receives the prediction's gradient negated."""

    def forward(self, keypoints_pred, keypoints_gt):
        assert keypoints_pred.shape == keypoints_gt.shape
        if not (keypoints_pred.is_cuda and keypoints_gt.is_cuda):
            from capf.lib import CapfError
            raise CapfError("MPJPE runs on the MI355X only: got a CPU tensor (no CPU fallback)")
        dt = torch.promote_types(keypoints_pred.dtype, keypoints_gt.dtype)
        if keypoints_pred.dtype != torch.float32 or keypoints_gt.dtype != torch.float32:
            keypoints_pred, keypoints_gt = keypoints_pred.float(), keypoints_gt.float()
        loss = _MPJPEFn.apply(keypoints_pred, keypoints_gt)
        return loss if dt == torch.float32 else loss.to(dt)        # the reference returns the inputs' dtype (torch.norm / mean)


def _set_mean(pred, gt, column, per_pair=False):
    """mean of one per-pose error column over all poses (fp64 on the device, fixed order)."""
    from capf.lib import pose_errors, segment_sums
    p, g = _poses(pred), _poses(gt)
    sums, counts = segment_sums(pose_errors(p, g))
    sums, counts = sums.cpu().numpy(), counts.cpu().numpy()
    n = counts[0, 1] if per_pair else counts[0, 0]
    return sums[0, column] / n if n > 0 else float("nan")


class P_MPJPE(nn.Module):
    """loss.py:25-68 — MPJPE after similarity alignment ("Protocol #2").  Arguments [N,17,3] (numpy, as
    human36m.py:374 passes them, or CUDA tensors); returns a numpy scalar like the reference."""

    def forward(self, keypoints_pred, keypoints_gt):
        assert keypoints_pred.shape == keypoints_gt.shape
        return np.float32(_set_mean(keypoints_pred, keypoints_gt, 1))


class N_MPJPE(nn.Module):
    """loss.py:71-84 — scale-normalised MPJPE on [B,1,17,3] tensors; returns a 0-d tensor like the reference."""

    def forward(self, keypoints_pred, keypoints_gt):
        assert keypoints_pred.shape == keypoints_gt.shape
        v = _set_mean(keypoints_pred, keypoints_gt, 2)
        dev = keypoints_pred.device if isinstance(keypoints_pred, torch.Tensor) else "cpu"
        return torch.tensor(v, dtype=torch.float32, device=dev)


class MPJVE(nn.Module):
    """loss.py:87-101 — mean per-joint velocity error over consecutive rows of [N,17,3]."""

    def forward(self, keypoints_pred, keypoints_gt):
        assert keypoints_pred.shape == keypoints_gt.shape
        return np.float32(_set_mean(keypoints_pred, keypoints_gt, 3, per_pair=True))


class _KeypointsLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, validity, mode, threshold):
        from capf.lib import keypoints_loss
        # f(gt - pred): the target's gradient is the prediction's negated (no gradient to the validity mask, which the callers build from labels)
        loss, dpred = keypoints_loss(mode, pred, gt, validity, threshold, want_grad=any(ctx.needs_input_grad[:2]))
        ctx.dpred = dpred
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        d = ctx.dpred * g
        return (d if ctx.needs_input_grad[0] else None), (-d if ctx.needs_input_grad[1] else None), None, None, None


class _KeypointsLoss(nn.Module):
    mode = 0

    def forward(self, keypoints_pred, keypoints_gt, keypoints_binary_validity):
        if not (keypoints_pred.is_cuda and keypoints_pred.dtype == torch.float32):
            from capf.lib import CapfError
            raise CapfError("keypoint losses run on the MI355X only (no CPU fallback)")
        return _KeypointsLossFn.apply(keypoints_pred, keypoints_gt, keypoints_binary_validity, self.mode,
                                      float(getattr(self, "threshold", 0.0)))


class KeypointsMSELoss(_KeypointsLoss):
    """loss.py:104-112"""
    mode = 0


class KeypointsMSESmoothLoss(_KeypointsLoss):
    """loss.py:115-126"""
    mode = 1

    def __init__(self, threshold=400):
        super().__init__()
        self.threshold = threshold


class KeypointsMAELoss(_KeypointsLoss):
    """loss.py:129-137"""
    mode = 2


def _fp32_in(what, *tensors):
    """The module's convention for a loss's tensor arguments: CUDA only (CapfError otherwise), other float dtypes computed in fp32.
    -> (the tensors as fp32, the dtype the loss is cast back to)"""
    from capf.lib import CapfError
    if not all(isinstance(t, torch.Tensor) for t in tensors):
        raise CapfError(f"{what} takes tensors, got {[type(t).__name__ for t in tensors]}")
    if not all(t.is_cuda for t in tensors):
        raise CapfError(f"{what} runs on the MI355X only: got a CPU tensor (no CPU fallback)")
    dt = tensors[0].dtype
    for t in tensors[1:]:
        dt = torch.promote_types(dt, t.dtype)
    return [t if t.dtype == torch.float32 else t.float() for t in tensors], dt


class _KeypointsL2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, validity):
        from capf.lib import keypoints_l2_loss
        # sqrt(sum((gt - pred)^2 * validity)): the target's gradient is the prediction's negated, the mask gets none
        loss, dpred = keypoints_l2_loss(pred, gt, validity, want_grad=any(ctx.needs_input_grad[:2]))
        ctx.dpred = dpred
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        d = ctx.dpred * g
        return (d if ctx.needs_input_grad[0] else None), (-d if ctx.needs_input_grad[1] else None), None


class KeypointsL2Loss(nn.Module):
    """loss.py:140-147: sum over rows of sqrt(sum((gt - pred)^2 * validity, dim=-1)) / max(1, sum(validity)); pred / gt [..., D],
    validity [..., 1].  Differentiable in pred and gt.  The gradient of a row whose square root is 0 -- validity 0, or pred == gt -- is
    exactly 0 (capf_mpjpe's rule at zero distance); the reference's autograd returns NaN there, for the whole batch's step."""

    def forward(self, keypoints_pred, keypoints_gt, keypoints_binary_validity):
        from capf.lib import CapfError
        if keypoints_pred.shape != keypoints_gt.shape:
            raise CapfError(f"KeypointsL2Loss: pred {tuple(keypoints_pred.shape)} and gt {tuple(keypoints_gt.shape)} differ in shape")
        (p, g), dt = _fp32_in("KeypointsL2Loss", keypoints_pred, keypoints_gt)
        loss = _KeypointsL2Fn.apply(p, g, keypoints_binary_validity)
        return loss if dt == torch.float32 else loss.to(dt)


# LimbLengthError.CONNECTIVITY_DICT (loss.py:185): the sixteen bones of the 17-joint Human3.6M skeleton
CONNECTIVITY_DICT = ((0, 1), (1, 2), (2, 6), (5, 4), (4, 3), (3, 6), (6, 7), (7, 8), (8, 16), (9, 16), (8, 12), (11, 12), (10, 11), (8, 13),
                     (13, 14), (14, 15))


class LimbLengthError(nn.Module):
    """loss.py:181-201: mean over the limbs of the mean over the batch of | |pred limb| - |gt limb| |.  Arguments [b, 17, 3], numpy (as the
    reference accepts) or CUDA tensors; returns a Python float like the reference.  One launch for the per-pose errors, one for the fp64
    sums per limb and ONE synchronisation (the reference: a `.cpu()` per limb, sixteen).  No gradient: see limb_length_loss."""

    def __init__(self):
        super().__init__()
        self.CONNECTIVITY_DICT = list(CONNECTIVITY_DICT)

    def forward(self, keypoints_3d_pred, keypoints_3d_gt):
        from capf.lib import CapfError, limb_length_errors, limb_length_sums, limb_table
        if tuple(keypoints_3d_pred.shape) != tuple(keypoints_3d_gt.shape) or len(keypoints_3d_pred.shape) != 3 or keypoints_3d_pred.shape[-1] != 3:
            raise CapfError(f"LimbLengthError takes pred and gt [b, joints, 3], got {tuple(keypoints_3d_pred.shape)} and {tuple(keypoints_3d_gt.shape)}")
        limb_table(self.CONNECTIVITY_DICT, keypoints_3d_pred.shape[1])          # (judged before anything is uploaded)
        p, g = _cuda(keypoints_3d_pred), _cuda(keypoints_3d_gt)
        err, _ = limb_length_errors(p, g, self.CONNECTIVITY_DICT)
        sums, _ = limb_length_sums(err)
        sums = sums.cpu().numpy()
        return float(sum(s / p.shape[0] for s in sums[0]) / len(self.CONNECTIVITY_DICT))


class _LimbLengthFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, limbs):
        from capf.lib import limb_length_errors, limb_length_sums
        n, L = pred.shape[0], len(limbs)
        scale = 1.0 / (n * L)
        err, dpred = limb_length_errors(pred, gt, limbs, want_grad=ctx.needs_input_grad[0], grad_scale=scale)
        # | |pred limb| - |gt limb| | is symmetric in its two poses: the target's gradient is the same kernel with the roles exchanged
        dgt = limb_length_errors(gt, pred, limbs, want_grad=True, grad_scale=scale)[1] if ctx.needs_input_grad[1] else None
        ctx.grads = dpred, dgt
        sums, _ = limb_length_sums(err)
        return (sums[0].sum() * scale).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        dpred, dgt = ctx.grads
        return (dpred * g if dpred is not None else None), (dgt * g if dgt is not None else None), None


def limb_length_loss(keypoints_3d_pred, keypoints_3d_gt, limbs=None):
    """LimbLengthError as a training loss: the same figure, mean over poses and limbs of | |pred limb| - |gt limb| |, as a 0-d tensor that is
    differentiable in pred and in gt.  pred / gt: CUDA [..., joints, 3]; limbs: (a, b) joint pairs, None = CONNECTIVITY_DICT.
    A predicted limb of length 0 and a limb whose two lengths agree exactly contribute a zero gradient."""
    from capf.lib import CapfError, limb_table
    if tuple(keypoints_3d_pred.shape) != tuple(keypoints_3d_gt.shape) or keypoints_3d_pred.dim() < 3 or keypoints_3d_pred.shape[-1] != 3:
        raise CapfError(f"limb_length_loss takes pred and gt [..., joints, 3], got {tuple(keypoints_3d_pred.shape)} and {tuple(keypoints_3d_gt.shape)}")
    limbs = tuple(tuple(int(v) for v in pair) for pair in (CONNECTIVITY_DICT if limbs is None else limbs))
    J = keypoints_3d_pred.shape[-2]
    limb_table(limbs, J)
    (p, g), dt = _fp32_in("limb_length_loss", keypoints_3d_pred, keypoints_3d_gt)
    loss = _LimbLengthFn.apply(p.reshape(-1, J, 3), g.reshape(-1, J, 3), limbs)
    return loss if dt == torch.float32 else loss.to(dt)


class _UncertaintyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, gt, *sigmas):
        from capf.lib import uncertainty_loss
        need = ctx.needs_input_grad
        loss, dpred, dsig = uncertainty_loss(pred, gt, sigmas, want_dpred=any(need[:2]), want_dsigma=need[2:])
        ctx.grads = dpred, dsig
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        dpred, dsig = ctx.grads
        need = ctx.needs_input_grad
        d = dpred * g if dpred is not None else None
        return ((d if need[0] else None), (-d if need[1] else None)) + tuple(s * g if s is not None else None for s in dsig)


def UNCERTAINTY(sigma_list, keypoints_pred, keypoints_gt):
    """loss.py:7-13: sum over the sigmas of mean(|| (pred - gt) / (sigma + 1e-6) ||_2) + 0.01 * mean(log(sigma + 1e-6)).  Each sigma has
    pred's shape [..., D] or [..., 1]; 1 to 8 of them.  Differentiable in pred, gt and every sigma, the norm term's gradient 0 where the
    scaled residual is 0.  sigma + 1e-6 <= 0 gives NaN (loss and gradients), unclamped, as the reference's log does."""
    from capf.lib import CapfError
    sigma_list = list(sigma_list)
    if keypoints_pred.shape != keypoints_gt.shape:
        raise CapfError(f"UNCERTAINTY: pred {tuple(keypoints_pred.shape)} and gt {tuple(keypoints_gt.shape)} differ in shape")
    if not 1 <= len(sigma_list) <= 8:
        raise CapfError(f"UNCERTAINTY takes 1..8 sigma tensors, got {len(sigma_list)}")
    lead, D = tuple(keypoints_pred.shape[:-1]), keypoints_pred.shape[-1]
    for k, s in enumerate(sigma_list):
        if not isinstance(s, torch.Tensor) or tuple(s.shape) not in (lead + (D,), lead + (1,)):
            raise CapfError(f"UNCERTAINTY: sigma {k} must be {lead + (D,)} or {lead + (1,)}, got {tuple(getattr(s, 'shape', ()))}")
    (p, g, *sig), dt = _fp32_in("UNCERTAINTY", keypoints_pred, keypoints_gt, *sigma_list)
    loss = _UncertaintyFn.apply(p, g, *sig)
    return loss if dt == torch.float32 else loss.to(dt)
