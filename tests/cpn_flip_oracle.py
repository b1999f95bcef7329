"""CPN's test-time flip (cpn/test.py:62-70) as include/capf.h states it for capf_cpn_decode_pair, in numpy float32 -- the yardstick of
tests/test_cpn_flip.py and tests/test_gpu_cpn_flip.py.  Everything behind the fold is tests/cpn_decode_oracle.py's, by import.

The fold is stated twice, and the two must agree bit for bit:

    fold()              the index formula of the header:  zf[b, y, x, j] = 0.5 * (z[b, y, x, j] + z[Bsrc + b, y, W - 1 - x, swap[j]])
    fold_sequential()   what the reference does to each mirror frame: channels first, every plane mirrored left to right, the symmetric
                        pairs exchanged one after the other on that copy, the result ADDED to the source frame's map in place and the
                        sum HALVED in place (float32 `+=`, then `/= 2`)

Halving a float32 is exact unless the result is subnormal, and then both forms round the same exact quotient once: 0.5 * s == s / 2.
The stacks are capf_preprocess_points(mode = 2)'s mirrored set with `mirror_width` in place of its 192."""
import numpy as np

import cpn_decode_oracle as O  # noqa: F401  (re-exported: callers take the generator and the decode from one place)


def involution(J):
    """(0)(1 2)(3 4)... on J joints: the swap table of the cases with J != 17"""
    tab = list(range(J))
    for a in range(1, J - 1, 2):
        tab[a], tab[a + 1] = a + 1, a
    return tuple(tab)


def pairs_of(swap):
    """a swap table (its own inverse) -> the list of exchanged pairs (q, w), q < w: the form of upstream's cfg.symmetry"""
    swap = [int(v) for v in swap]
    assert all(0 <= v < len(swap) and swap[v] == j for j, v in enumerate(swap)), swap
    return [(j, v) for j, v in enumerate(swap) if j < v]


def fold(z2, swap):
    """z2 [2 Bsrc, H, W, C] float32 NHWC, swap J ints (J <= C) -> zf [Bsrc, H, W, J] float32: the header's index formula"""
    z2 = np.asarray(z2, dtype=np.float32)
    B, W = z2.shape[0] // 2, z2.shape[2]
    J = len(swap)
    zf = np.empty((B,) + z2.shape[1:3] + (J,), dtype=np.float32)
    for j in range(J):
        for x in range(W):
            s = z2[:B, :, x, j] + z2[B:, :, W - 1 - x, int(swap[j])]     # float32 + float32: one rounding
            zf[:, :, x, j] = np.float32(0.5) * s
    return zf


def fold_sequential(z2, swap):
    """the same map by the reference's procedure (see the module text); J = len(swap) channels are folded"""
    z2 = np.asarray(z2, dtype=np.float32)
    B = z2.shape[0] // 2
    J = len(swap)
    score_map = np.ascontiguousarray(z2[:B, :, :, :J].transpose(0, 3, 1, 2)).copy()          # [Bsrc, J, H, W], as the network returns it
    mirror_map = np.ascontiguousarray(z2[B:, :, :, :J].transpose(0, 3, 1, 2))
    for b in range(B):
        planes = [mirror_map[b, j, :, ::-1].copy() for j in range(J)]                        # every plane mirrored left to right
        for q, w in pairs_of(swap):
            planes[q], planes[w] = planes[w], planes[q]
        score_map[b] += np.array(planes)
        score_map[b] /= 2
    return np.ascontiguousarray(score_map.transpose(0, 2, 3, 1))


def mirrored_stacks(kcrop, k2d, swap, mirror_width=192.0):
    """kcrop / k2d [Bsrc, J, 2] float32 (k2d may be None) -> the stacks [2, Bsrc, J, 2]: set 0 the keypoints, set 1 their mirror --
    slot swap[j] of set 1 holds ((mirror_width - x) - 1, y) of joint j in crop pixels (two rounded float32 subtractions) and (-x, y) in
    image coordinates"""
    f = np.float32
    kcrop = np.asarray(kcrop, dtype=f)
    B, J = kcrop.shape[:2]
    kc2 = np.empty((2, B, J, 2), dtype=f)
    kc2[0] = kcrop
    k22 = None
    if k2d is not None:
        k2d = np.asarray(k2d, dtype=f)
        k22 = np.empty((2, B, J, 2), dtype=f)
        k22[0] = k2d
    for j in range(J):
        s = int(swap[j])
        kc2[1, :, s, 0] = (f(mirror_width) - kcrop[:, j, 0]) - f(1.0)
        kc2[1, :, s, 1] = kcrop[:, j, 1]
        if k22 is not None:
            k22[1, :, s, 0] = -k2d[:, j, 0]
            k22[1, :, s, 1] = k2d[:, j, 1]
    return kc2, k22
