"""capf_kp_heatmap_loss restated in numpy float64 (include/capf.h has the rules): the Gaussian target with its fp32 roundings, the
weight-zeroing rules, l_bj, both reductions with the tie rule, the analytic gradients, and per output the fp64 sum of absolute terms that
the GPU tests scale their bounds by.  Everything takes the LOGITS z [B, J, H, W] (the GPU tests pass the library's own `heat`), so only the
target, the loss arithmetic and the summation orders are under test.  No torch, no GPU."""
import math

import numpy as np

MEAN, OHKM = 0, 1
F32 = np.float32
TILE = 256          # pixels of a tile (csrc/kp_head.hip KP_THREADS)
BW_SLABS = 8        # blocks per frame (csrc/kernels.h KP_BW_SLABS)
RED_PARTS = 16      # parts of the last launch's two-stage sums


def radius(sigma):
    return int(math.ceil(float(F32(3.0) * F32(sigma))))


def centres(kcrop_gt, decode):
    """(c [B, J, 2] fp32 heatmap coordinates, mu [B, J, 2] int64 (0 where not ok), ok [B, J]): c = (k - o) / s with both operations rounded in
    fp32, mu = int(c + 0.5f) truncated toward zero; ok: both coordinates finite and |c| <= 2^20"""
    k = np.asarray(kcrop_gt, F32)
    sx, ox, sy, oy = (F32(v) for v in decode)
    with np.errstate(all="ignore"):
        c = np.stack([(k[..., 0] - ox) / sx, (k[..., 1] - oy) / sy], -1).astype(F32)
        ok = np.isfinite(c).all(-1) & (np.abs(c) <= F32(2.0 ** 20)).all(-1)
        half = (c + F32(0.5)).astype(F32)
    mu = np.zeros(c.shape, np.int64)
    mu[ok] = np.trunc(half[ok].astype(np.float64)).astype(np.int64)
    return c, mu, ok


def effective_weight(kcrop_gt, target_weight, decode, sigma, H, W):
    """w_bj [B, J] float64: target_weight (None: 1), 0 when the window lies wholly outside the map or the centre is not ok"""
    _, mu, ok = centres(kcrop_gt, decode)
    R = radius(sigma)
    w = np.ones(mu.shape[:2]) if target_weight is None else np.asarray(target_weight, F32).astype(np.float64).reshape(mu.shape[:2]).copy()
    outside = (mu[..., 0] - R >= W) | (mu[..., 1] - R >= H) | (mu[..., 0] + R < 0) | (mu[..., 1] + R < 0)
    w[~ok | outside] = 0.0
    return w


def targets(kcrop_gt, decode, sigma, H, W):
    """t [B, J, H, W] float64: exp(-d2 / (2 sigma^2)) inside the (2 R + 1)^2 window around mu, 0 elsewhere (and everywhere when not ok)"""
    _, mu, ok = centres(kcrop_gt, decode)
    R = radius(sigma)
    s = float(F32(sigma))
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    t = np.zeros(mu.shape[:2] + (H, W))
    for b in range(mu.shape[0]):
        for j in range(mu.shape[1]):
            if ok[b, j]:
                dx, dy = xs - mu[b, j, 0], ys - mu[b, j, 1]
                t[b, j] = np.where((np.abs(dx) <= R) & (np.abs(dy) <= R), np.exp(-(dx * dx + dy * dy) / (2.0 * s * s)), 0.0)
    return t


def window(kcrop_gt, decode, sigma, H, W):
    """bool [B, J, H, W]: the pixels of the map inside each item's target window"""
    _, mu, ok = centres(kcrop_gt, decode)
    R = radius(sigma)
    ys, xs = np.arange(H)[:, None], np.arange(W)[None, :]
    m = (np.abs(xs - mu[..., 0, None, None]) <= R) & (np.abs(ys - mu[..., 1, None, None]) <= R)
    return m & ok[..., None, None]


def select(lj, reduction, topk):
    """sel [B, J] in {0, 1}: all ones under MEAN; under OHKM the min(topk, J) largest l_bj of each frame, a NaN first, ties to the smaller j"""
    B, J = lj.shape
    sel = np.ones((B, J))
    if reduction == OHKM:
        sel[:] = 0.0
        for b in range(B):
            order = sorted(range(J), key=lambda j: (0 if np.isnan(lj[b, j]) else 1, -lj[b, j] if not np.isnan(lj[b, j]) else 0.0, j))
            sel[b, order[:min(topk, J)]] = 1.0
    return sel


def norm(B, J, reduction, topk):
    return float(B) * (J if reduction == MEAN else topk)


def evaluate(z, x, weight, kcrop_gt, target_weight, decode, sigma, reduction=MEAN, topk=8, scale=0.5, drop=None):
    """The whole entry in float64 from the logits z [B, J, H, W] and the map x [B, H, W, C] (None: no dweight), weight [J, C] (None: no dmap).
    drop = (b, j, y, x): that pixel's term is left out of item (b, j) -- what a kernel that skipped it would compute.
    Returns a dict: loss, joint_loss [B, J], sel, g [B, J], dweight, dbias, dmap, and `mass`, per output the fp64 sum of the absolute values
    of the terms its sum adds: (z - t)^2, |dz|, |dz X|, |dz W|, with the outputs' own factors."""
    z = np.asarray(z, np.float64)
    B, J, H, W = z.shape
    t = targets(kcrop_gt, decode, sigma, H, W)
    w = effective_weight(kcrop_gt, target_weight, decode, sigma, H, W)
    d = z - t
    da = np.abs(d)
    if drop is not None:
        d[drop] = 0.0
        da[drop] = 0.0
    sc = float(F32(scale))
    coef = sc * w * w / (H * W)
    with np.errstate(invalid="ignore"):
        lj = np.where(w == 0, 0.0, coef * (d * d).sum((2, 3)))            # an item without weight is an exact 0, whatever its logits
    sel = select(lj, reduction, topk)
    n = norm(B, J, reduction, topk)
    g = 2.0 * sc * w * w * sel / (H * W * n)
    out = {"joint_loss": lj, "sel": sel, "g": g, "w": w, "loss": np.where(sel > 0, lj, 0.0).sum() / n}
    mass = {"joint_loss": coef * (da * da).sum((2, 3))}
    mass["loss"] = (mass["joint_loss"] * sel).sum() / n
    with np.errstate(invalid="ignore"):
        dz, dza = np.where(g[..., None, None] == 0, 0.0, g[..., None, None] * d), np.where(g[..., None, None] == 0, 0.0, np.abs(g)[..., None, None] * da)
    out["dbias"], mass["dbias"] = dz.sum((0, 2, 3)), dza.sum((0, 2, 3))
    if x is not None:
        x = np.asarray(x, np.float64)
        out["dweight"], mass["dweight"] = np.einsum("bjyx,byxc->jc", dz, x), np.einsum("bjyx,byxc->jc", dza, np.abs(x))
    if weight is not None:
        wt = np.asarray(weight, np.float64)
        out["dmap"], mass["dmap"] = np.einsum("bjyx,jc->byxc", dz, wt), np.einsum("bjyx,jc->byxc", dza, np.abs(wt))
    out["mass"] = mass
    return out


def depths(B, H, W, J):
    """per output, the length of the longest chain of fp32 additions of the documented summation order (include/capf.h): what (d + 8) 2^-24
    of the sum of absolute terms bounds"""
    tiles = -(-H * W // TILE)
    bw_tiles = -(-tiles // BW_SLABS)
    nbw = -(-tiles // bw_tiles)
    item = (TILE // 8) * bw_tiles + 8 + nbw                    # a lane's pixels over the block's tiles, the 8 lanes, the blocks
    two_stage = lambda n: -(-n // RED_PARTS) + RED_PARTS
    param = TILE + bw_tiles + two_stage(B * nbw)               # a tile's pixels, the block's tiles, the blocks' partials
    return {"joint_loss": item, "loss": item + J + two_stage(B), "dweight": param, "dbias": param, "dmap": J}


def bound(name, mass, B, H, W, J):
    return (depths(B, H, W, J)[name] + 8) * 2.0 ** -24 * mass
