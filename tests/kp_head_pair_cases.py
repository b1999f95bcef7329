"""The yardstick of the keypoint head on a flip-test pair, on top of kp_head_cases (imported as K, untouched): the flip / swap / shift of
HRNet's flip test written in numpy / torch, the cases, and the float64 evaluation with its bounds.  Nothing here calls the library.

A pair case of shape (Bsrc, H, W, C, J) is K.make_case at 2 * Bsrc frames: the two halves are INDEPENDENT random frames, not true mirrors --
a true mirror would hide a wrong x or a wrong swap."""
import numpy as np
import torch

import kp_head_cases as K

H36M_SWAP = (0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13)
# (Bsrc, H, W, C, J): one pixel (nothing to shift), one row, W = 2, the one interior pixel of K.ONE_INTERIOR, one tile, tiles that cut rows
# (mirrored sources in another tile), several slabs, wide C, J = 1 (swap = (0,)), J = 32 (a seeded random involution)
SHAPES = ((1, 1, 1, 32, 17), (1, 1, 5, 32, 17), (2, 3, 2, 48, 17), (1, 4, 4, 32, 17), (1, 8, 8, 32, 17), (2, 16, 12, 48, 17),
          (1, 64, 48, 32, 17), (1, 24, 18, 256, 17), (2, 8, 8, 32, 1), (2, 8, 8, 32, 32))
DTYPE_SHAPES = ((1, 8, 8, 32, 17), (2, 16, 12, 48, 17), (1, 64, 48, 32, 17))


def swap_for(J, seed=7):
    """the swap table of a J-joint case: H36M's at 17, otherwise a seeded random involution with fixed points (J = 1: (0,))"""
    if J == 17:
        return H36M_SWAP
    order = np.random.default_rng(seed).permutation(J)
    table = list(range(J))
    for a, b in zip(order[0:2 * (J // 3):2], order[1:2 * (J // 3):2]):
        table[a], table[b] = int(b), int(a)
    assert all(table[table[j]] == j for j in range(J))
    return tuple(table)


def flipped_back(hm, swap, shift):
    """F: hm [Bsrc, J, H, W], the heatmaps of the mirror frames -> what HRNet adds to the crop's own heatmaps: flip_back (x mirrored, joints
    exchanged), then SHIFT_HEATMAP: flipped[:, :, :, 1:] = flipped.clone()[:, :, :, 0:-1] (column 0 keeps its own value).  numpy or torch."""
    idx = list(swap)
    if isinstance(hm, torch.Tensor):
        f = torch.flip(hm[:, idx], [3]).clone()
        if shift:
            f[:, :, :, 1:] = f.clone()[:, :, :, 0:-1]
        return f
    f = hm[:, idx][:, :, :, ::-1].copy()
    if shift:
        f[:, :, :, 1:] = f.copy()[:, :, :, 0:-1]
    return f


def fuse(h, swap, shift):
    """h [2 Bsrc, J, H, W] (numpy or torch, any float dtype) -> 0.5 * (h[b] + F(h)[b]) in h's dtype: one rounded sum, then an exact halving"""
    Bsrc = h.shape[0] // 2
    s = h[:Bsrc] + flipped_back(h[Bsrc:], swap, shift)
    return s * 0.5 if isinstance(h, torch.Tensor) else (s * h.dtype.type(0.5)).astype(h.dtype)


def pair_case(shape, seed, dtype=torch.float32):
    """the (rounded) map [2 Bsrc, H, W, C], weights, bias and swap table of one case"""
    Bsrc, H, W, C, J = shape
    X, Wt, bias = K.make_case((2 * Bsrc, H, W, C, J), seed)
    return {"X": K.round_map(X, dtype), "Wt": Wt, "bias": bias, "swap": swap_for(J), "shape": shape}


def image_f32(kcrop, A):
    """k2d as capf.h rounds it, float32 throughout: ((A00 kx + A01 ky) + A02, (A10 kx + A11 ky) + A12)"""
    kx, ky = kcrop[..., 0].astype(np.float32), kcrop[..., 1].astype(np.float32)
    A = A.astype(np.float32)
    return np.stack([(A[:, None, 0, 0] * kx + A[:, None, 0, 1] * ky) + A[:, None, 0, 2],
                     (A[:, None, 1, 0] * kx + A[:, None, 1, 1] * ky) + A[:, None, 1, 2]], -1).astype(np.float32)


def mirrored_set(kcrop, k2d, swap, mirror_width):
    """set 1 of the stacks from set 0, float32: kcrop -> ((mirror_width - x) - 1, y) of joint swap[j]; k2d -> (-x, y) of joint swap[j]"""
    idx = list(swap)
    kc, kd = kcrop[:, idx].astype(np.float32), (None if k2d is None else k2d[:, idx].astype(np.float32))
    mc = np.stack([(np.float32(mirror_width) - kc[..., 0]) - np.float32(1.0), kc[..., 1]], -1).astype(np.float32)
    return mc, (None if kd is None else np.stack([-kd[..., 0], kd[..., 1]], -1))


def integral_pair_case(c, shift, beta, decode, to_image):
    """float64 and float32 torch evaluations of the integral decode of the fused logits of pair_case c -- K.integral_case's rule and scale
    terms: (kcrop64, k2d64, score64, bound_kcrop, bound_k2d, bound_score); nothing of the kernel's result enters a bound"""
    out, zf = {}, {}
    for dt in (torch.float64, torch.float32):
        zf[dt] = fuse(K.logits(c["X"], c["Wt"], c["bias"], dt), c["swap"], shift)
        xy, score = K.decode_integral(zf[dt], beta)
        out[dt] = K.to_outputs(xy, decode, to_image) + (score,)
    k64, a64, s64 = out[torch.float64]
    k32, a32, _ = out[torch.float32]
    H, W = c["X"].shape[1:3]
    bk = 4 * (k32.double() - k64).abs().max().item() + 1e-6 * max(H, W) * max(abs(decode[0]), abs(decode[2]), 1.0)
    ba = 4 * (a32.double() - a64).abs().max().item() + 1e-6 * max(a64.abs().max().item(), 1.0)
    bs = 4 * (zf[torch.float32].double() - zf[torch.float64]).abs().max().item() + 1e-6 * zf[torch.float64].abs().max().item()
    return k64.numpy(), a64.numpy(), s64.numpy(), bk, ba, bs
