"""The numpy float64 restatement of capf_pck2d_counts (include/capf.h), one IEEE operation at a time, shared by the CPU and GPU tests of
the 2-D PCKh counts, of mvn/datasets/human36m.py::evaluate2d and of CA_PF.keypoint_loss(return_accuracy=True).

    u = ((double)px - (double)gx) / (double)nx,   v likewise with ny,   e = sqrt(u u + v v)
    detected at threshold k:  e <= thresholds[k]  (strict: e < thresholds[k])
    valid:  (weight is None or weight > 0) and (norm is None or both entries finite and > 0) and (segment is None or 0 <= id < n_segments)
    counts [S, K, J], valid [S, J] integers;  err_sums [S, J] = the sum of e over valid samples: lane t of 256 adds its poses
    t, t + 256, ... in order, then partial t += partial t + o for o = 128, 64, ..., 1.

numpy's float64 subtract, divide, multiply, add and sqrt are the correctly rounded IEEE operations, each rounded on its own."""
import math

import numpy as np

LANES = 256


def distances(pred, gt, norm=None):
    """e [n, J] float64 from fp32-representable pred / gt [n, J, 2] and norm [n, 2] (None: (1, 1)); entries of poses with an invalid norm
    are computed too (and may be anything): valid_mask decides what is used."""
    p, g = np.asarray(pred).astype(np.float64), np.asarray(gt).astype(np.float64)
    d = p - g
    if norm is None:
        u, v = d[..., 0] / 1.0, d[..., 1] / 1.0
    else:
        nm = np.asarray(norm).astype(np.float64)
        with np.errstate(all="ignore"):
            u, v = d[..., 0] / nm[:, None, 0], d[..., 1] / nm[:, None, 1]
    with np.errstate(all="ignore"):
        uu, vv = u * u, v * v
        return np.sqrt(uu + vv)


def valid_mask(n, J, norm=None, weight=None, segment=None, n_segments=1):
    """(mask [n, J] bool, segment id per pose [n] with every pose in 0 when segment is None)"""
    ok = np.ones((n, J), bool)
    if weight is not None:
        ok &= np.asarray(weight).reshape(n, J) > 0                       # (a NaN weight is not > 0)
    if norm is not None:
        nm = np.asarray(norm).astype(np.float64).reshape(n, 2)
        ok &= (np.isfinite(nm).all(axis=1) & (nm > 0).all(axis=1))[:, None]
    if segment is None:
        assert n_segments == 1
        sid = np.zeros(n, np.int64)
    else:
        sid = np.asarray(segment).astype(np.int64).reshape(n)
        ok &= ((sid >= 0) & (sid < n_segments))[:, None]
    return ok, sid


def ordered_sum(values, use):
    """The kernel's sum of values[i] over the poses i with use[i], in its order: 256 lanes, then the fixed tree."""
    part = np.zeros(LANES, np.float64)
    with np.errstate(all="ignore"):
        for r in range(0, len(values), LANES):
            row, m = values[r:r + LANES], use[r:r + LANES]
            part[:len(row)] = np.where(m, part[:len(row)] + np.where(m, row, 0.0), part[:len(row)])
        o = LANES // 2
        while o:
            part[:o] = part[:o] + part[o:2 * o]
            o //= 2
    return part[0]


def pck2d_counts(pred, gt, thresholds, norm=None, weight=None, strict=False, segment=None, n_segments=1):
    """-> (counts int32 [S, K, J], valid int32 [S, J], err_sums float64 [S, J], e [n, J], mask [n, J])"""
    pred, gt = np.asarray(pred), np.asarray(gt)
    n, J = gt.shape[0], gt.shape[1]
    thr = np.asarray([float(t) for t in thresholds], np.float64)
    e = distances(pred, gt, norm) if n else np.zeros((0, J))
    ok, sid = valid_mask(n, J, norm, weight, segment, n_segments)
    with np.errstate(invalid="ignore"):
        hit = (e[:, None, :] < thr[None, :, None]) if strict else (e[:, None, :] <= thr[None, :, None])      # [n, K, J]; NaN fails both
    counts = np.zeros((n_segments, len(thr), J), np.int32)
    valid = np.zeros((n_segments, J), np.int32)
    sums = np.zeros((n_segments, J), np.float64)
    for s in range(n_segments):
        use = ok & (sid == s)[:, None]
        counts[s] = (hit & use[:, None, :]).sum(axis=0)
        valid[s] = use.sum(axis=0)
        for j in range(J):
            sums[s, j] = ordered_sum(e[:, j], use[:, j])
    return counts, valid, sums, e, ok & ((sid >= 0) & (sid < n_segments))[:, None]


def fsum_bound(e, use):
    """(math.fsum of the used e, the bound (ceil(n / 256) + 8) 2^-53 sum|e| the kernel's summation order implies: at most ceil(n / 256) - 1
    additions in a lane and 8 tree levels above it)"""
    vals = [float(x) for x, m in zip(e, use) if m]
    return math.fsum(vals), (math.ceil(len(e) / LANES) + 8) * 2.0 ** -53 * math.fsum(abs(x) for x in vals)


def accuracy(counts, valid):
    """keypoint_loss's figure: the mean over joints with valid > 0 of counts / valid (threshold 0, segment 0); NaN without such a joint"""
    c, v = np.asarray(counts)[0, 0].astype(np.float64), np.asarray(valid)[0].astype(np.float64)
    ok = v > 0
    return float(np.mean(c[ok] / v[ok])) if ok.any() else float("nan")
