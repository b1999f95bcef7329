"""Inputs and the fp64 yardstick of the keypoint-gradient tests (test_points_grad_api.py on the CPU, test_gpu_points_grad.py on the GPU).

The yardstick is train_yardstick.lifter64's recipe -- capf_oracle.lifter_forward in float64, MPJPE, autograd, the deformable samplers in
the cells and on the clip sides the implementation under test used -- with the two keypoint tensors as leaves next to the parameters.

Margin rule of the reference points: the reference-point sampler (zeros padding, pose_dformer.py:217) takes its cell from floor() in both
the yardstick and the kernel, and no tap tells one the other's choice; so every case keeps the unnormalised coordinate of every reference
point at least MARGIN_PX from an integer on every level (fp32 roundoff of that coordinate is below 1e-5 px on a 32-pixel map), and
margin_px() measures it."""
import numpy as np
import torch

import capf_oracle as oracle
from feature_cases import GOLDEN, HRNET32_128x96, golden_inputs

MARGIN_PX = 1e-4
TAME_OFFSET_SCALE = 0.05          # the module initialises sampling_offsets near zero (mvn/models/_native.py init_deformable_blocks)


HRNET32_32x32 = [(32, 8, 8), (64, 4, 4), (128, 2, 2), (256, 1, 1)]      # (C_l, H_l, W_l): the smallest plan, top map 1 x 1
# reference values of the hand-made frame: partly outside (|g| = 1.02: the -1 / size cell, one column or row of corners missing), outside
# the larger maps but inside the small ones' border cell (1.3), outside EVERY map of a 128 x 96 crop (-2.5, 2.7) and of a 32 x 32 crop (3.5)
OFF_MAP_REF = [(-1.3, 0.23), (0.37, -1.3), (-1.02, 0.11), (0.17, -1.02), (1.02, -0.41), (-0.35, 1.02), (1.3, 0.53), (0.47, 1.3),
               (-1.3, 1.3), (-1.02, 1.02), (1.02, -1.3), (-2.5, 0.31), (0.23, 2.7), (-2.5, 2.7), (-3.5, 3.5)]
WHOLLY_OUTSIDE_128x96 = (11, 12, 13, 14)      # joints of OFF_MAP_REF with no corner inside any map of a 128 x 96 crop (one axis outside is enough)
WHOLLY_OUTSIDE_32x32 = (14,)                  # ... of a 32 x 32 crop (a 2-pixel axis reaches out to |g| = 3)


def case_inputs(B, case=GOLDEN):
    """feature_cases.golden_inputs at batch B, plus the crop keypoints in pixels that normalise to its ref:
    (maps NCHW fp32, k2d, crop keypoints, ref, gt)."""
    from capf import synth
    case = dict(case, B=B)
    maps, k2d, ref, gt = golden_inputs(case)
    _, _, kc, _ = synth.synth_inputs(B, case["H"], case["W"], seed=case["iseed"], crop_range=(192, 256), with_gt=True)
    return maps, k2d, kc, ref, gt


def normalise(kc):
    """conpose.py:34-35 in fp32, out of place."""
    ref = kc.clone()
    ref[..., 0] = ref[..., 0] / 96.0 - 1.0
    ref[..., 1] = ref[..., 1] / 128.0 - 1.0
    return ref


def off_map_(kc, frame=0):
    """Overwrite the first joints of one frame of crop keypoints (pixels) with OFF_MAP_REF's points; in place."""
    r = torch.tensor(OFF_MAP_REF, dtype=torch.float64)
    kc[frame, :len(OFF_MAP_REF)] = ((r + 1) * torch.tensor([96.0, 128.0], dtype=torch.float64)).float()
    return kc


def small_inputs(B, seed=47):
    """The 32 x 32 plan's inputs: (maps NCHW fp32 8 x 8 .. 1 x 1, k2d, crop keypoints with joint 14 of frame 0 outside every map, ref, gt)."""
    from capf import synth
    from feature_cases import synth_maps
    _, k2d, kc, gt = synth.synth_inputs(B, 32, 32, seed=seed, crop_range=(192, 256), with_gt=True)
    kc = kc.clone()
    kc[0, 14] = torch.tensor([(-3.5 + 1) * 96.0, (3.5 + 1) * 128.0])
    return synth_maps(B, HRNET32_32x32, seed), k2d, kc, normalise(kc), gt


def tame_(params):
    """Scale every sampling_offsets parameter of a {name: tensor} dict (or a module's named parameters) by TAME_OFFSET_SCALE, in place."""
    with torch.no_grad():
        for k, v in params.items():
            if ".sampling_offsets." in k:
                v.mul_(TAME_OFFSET_SCALE)
    return params


def margin_px(ref, geometry=HRNET32_128x96):
    """Smallest distance (pixels) of any unnormalised reference coordinate from an integer, over the levels of `geometry` ((C, H, W) per level;
    levels of size 1 have no cells); float64 arithmetic on the fp32 values."""
    r = ref.detach().cpu().double()
    worst = float("inf")
    for _, H, W in geometry:
        for axis, size in ((0, W), (1, H)):
            if size > 1:
                u = (r[..., axis] + 1) / 2 * (size - 1)
                worst = min(worst, (u - u.round()).abs().min().item())
    return worst


def points64(params, k2d, ref, gt, feats, cells=None, drop_masks=None, sides=None, context_blocks=True, depth=None, dtype=torch.float64):
    """lifter64 with k2d and ref as leaves.  Returns ({name: parameter gradient}, dk2d, dref, prediction, loss) in `dtype` (float64: the
    yardstick; float32: the same evaluation in the kernels' precision, whose distance from float64 is the floor of the comparison)."""
    Q = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in params.items() if k.startswith("volume_net.")}
    k = k2d.detach().cpu().to(dtype).clone().requires_grad_(True)
    r = ref.detach().cpu().to(dtype).clone().requires_grad_(True)
    fs = [f.detach().cpu().to(dtype) for f in feats]
    w = oracle.lifter_forward(Q, k, r, fs, cells=cells, unclipped=sides, context_blocks=context_blocks, depth=depth,
                              drop_masks=drop_masks.detach().cpu().to(dtype) if drop_masks is not None else None)
    loss = oracle.mpjpe(w, gt.detach().cpu().to(dtype))
    loss.backward()
    return {n: q.grad for n, q in Q.items()}, k.grad, r.grad, w.detach(), loss.item()


def oracle_cells_and_sides(params, k2d, ref, feats, drop_masks=None):
    """The cells and clip sides an fp32 evaluation of the oracle takes (the CPU stand-in for the engine's cidx / cpos taps): int64 /
    bool [B, 17, 4, 16, 2] per context block, by train_yardstick.engine_clip_sides' rule on the fp32 positions."""
    taps = {}
    with torch.no_grad():
        P = {n: v.detach().cpu().float() for n, v in params.items() if n.startswith("volume_net.")}
        oracle.lifter_forward(P, k2d.float(), ref.float(), [f.float() for f in feats], taps=taps,
                              drop_masks=drop_masks.float() if drop_masks is not None else None)
    cells, sides = [], []
    for pos in taps["ctx_pos"]:                                 # [b, l, p, hs, 2]
        pos = pos.permute(0, 2, 1, 3, 4).contiguous().numpy()   # [b, p, l, hs, 2]
        c = np.zeros(pos.shape, dtype=np.int64)
        free = np.zeros(pos.shape, dtype=bool)
        for l, f in enumerate(feats):
            H, W = f.shape[2], f.shape[3]
            q = oracle.bilinear_corners(pos[:, :, l], H, W, "border")
            c[:, :, l, :, 0], c[:, :, l, :, 1] = q["ix0"], q["iy0"]
            for axis, size in ((0, W), (1, H)):
                x = ((pos[:, :, l, :, axis] + np.float32(1)) / np.float32(2)) * np.float32(size - 1)
                free[:, :, l, :, axis] = (x > 0) & (x < size - 1)
        cells.append(torch.from_numpy(c))
        sides.append(torch.from_numpy(free))
    return cells, sides


def rel_errors(got, want):
    """(relative L2, largest entry error / the yardstick's largest entry) of a gradient against its float64 yardstick."""
    d = got.detach().cpu().double() - want.double()
    return (d.norm() / want.double().norm().clamp_min(1e-300)).item(), (d.abs().max() / want.double().abs().max().clamp_min(1e-300)).item()
