"""Seeded pose families for the evaluation kernels' edge tests, their float64 yardstick and the per-pose bound
(tests/test_gpu_metric_edges.py on the GPU; tests/test_metrics.py holds the oracle's own restatement of the kernel to them on the CPU).

Every family returns float32 (pred, gt) of shape [n, J, 3]; nothing is filtered out of what a seed produces."""
import zlib

import numpy as np

import metrics_oracle as mo

FAMILIES = ("near", "mirrored", "unrelated", "rotated", "exact_similarity", "identical", "planar_mirrored", "millimetres")
COLUMNS = ("MPJPE", "P_MPJPE", "N_MPJPE", "velocity")
MIN_GAP = 1e-6          # between the two largest eigenvalues of Horn's 4x4 matrix: the condition under which the bound is claimed


def _rotations(rng, n):
    """uniformly random proper rotations: Q of a Gaussian matrix's QR with R's diagonal made positive, det made +1"""
    q, r = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    q = q * np.sign(np.diagonal(r, axis1=1, axis2=2))[:, None, :]
    q[:, :, 2] *= np.linalg.det(q)[:, None]
    return q


def pose_family(name, n, J, seed=0):
    rng = np.random.default_rng([seed, n, J, zlib.crc32(name.encode())])
    gt = rng.standard_normal((n, J, 3)) * 0.3
    noise = rng.standard_normal((n, J, 3))
    if name == "near":
        pred = gt + 0.05 * noise
    elif name == "mirrored":                                   # the det(R) = -1 branch of loss.py:54-58
        pred = gt * np.array([1.0, 1.0, -1.0]) + 0.01 * noise
    elif name == "unrelated":
        pred = noise
    elif name in ("rotated", "exact_similarity"):
        R = _rotations(rng, n)
        scale = 10.0 ** rng.uniform(-1.0, 1.0, (n, 1, 1))
        shift = rng.uniform(-5.0, 5.0, (n, 1, 3))
        pred = scale * np.matmul(gt, R.transpose(0, 2, 1)) + shift + (0.01 * noise if name == "rotated" else 0.0)
    elif name == "identical":
        pred = gt.copy()
    elif name == "planar_mirrored":                            # both poses in z = 0, the prediction mirrored inside that plane
        gt[:, :, 2] = 0.0
        noise[:, :, 2] = 0.0
        pred = gt * np.array([-1.0, 1.0, 1.0]) + 0.01 * noise
    elif name == "millimetres":                                # where centring in float32 would show
        gt = gt * 1000.0 + np.array([0.0, 0.0, 5000.0])
        pred = gt + 30.0 * noise
    else:
        raise KeyError(name)
    gt = gt.astype(np.float32)
    return (gt.copy() if name == "identical" else pred.astype(np.float32)), gt


def assert_condition(pred, gt, what):
    """every pose: centred norms > 0 and an eigenvalue gap of at least MIN_GAP -> the smallest gap"""
    nX, nY, gap = mo.horn_condition(pred, gt)
    assert (nX > 0).all() and (nY > 0).all(), what
    assert gap.min() >= MIN_GAP, f"{what}: eigenvalue gap {gap.min():.3e} at pose {int(gap.argmin())}"
    return float(gap.min())


def yardstick(pred, gt, prev=None):
    """-> (want [n,4] float64, bound [n,4]): bound = 2^-23 |want| (the one float32 store) + 1e-12 s, s the Frobenius norm of the
    centred ground-truth pose (N_MPJPE, which centres nothing: of the pose as it is)."""
    n = pred.shape[0]
    want = np.zeros((n, 4))
    want[:, 0] = mo.mpjpe_per_pose(pred, gt)
    want[:, 1] = mo.p_mpjpe_per_pose(pred, gt)
    want[:, 2] = mo.n_mpjpe_per_pose(pred, gt)
    want[:, 3] = mo.velocity_errors(pred, gt, np.arange(n) - 1 if prev is None else prev)
    return want, bound(want, gt)


def bound(want, gt):
    g = gt.astype(np.float64)
    s0 = np.sqrt(((g - g.mean(1, keepdims=True)) ** 2).sum((1, 2)))
    s = np.stack([s0, s0, np.sqrt((g ** 2).sum((1, 2))), s0], 1)
    return 2.0 ** -23 * np.abs(want) + 1e-12 * s


def permuted_segments(n, n_segments, seed):
    """segment ids in a seeded random order (interleaved runs of every id)"""
    return np.random.default_rng([seed, n, n_segments]).integers(0, n_segments, n).astype(np.int32)
