"""TEST INFRASTRUCTURE ONLY — CPU restatement (numpy, float64 inside) of the evaluation metrics next to the hot
path.  Each function cites the reference lines it follows; tests/test_metrics.py pins it against
tests/golden/losses.npz, which oracle/make_goldens.py captured from the REAL ContextPose/mvn/models/loss.py.
Only tests/ may import this module."""
import numpy as np


def mpjpe_per_pose(pred, gt):
    """loss.py:16-22 before the outer mean: [N,J,3] -> [N] mean over joints of the L2 distance."""
    return np.linalg.norm(pred.astype(np.float64) - gt.astype(np.float64), axis=-1).mean(-1)


def p_mpjpe_per_pose(pred, gt):
    """loss.py:25-68 (SVD form, as the reference writes it), per pose."""
    X, Y = gt.astype(np.float64), pred.astype(np.float64)
    muX, muY = X.mean(1, keepdims=True), Y.mean(1, keepdims=True)                    # :36-37
    X0, Y0 = X - muX, Y - muY
    normX = np.sqrt((X0 ** 2).sum((1, 2), keepdims=True))                              # :42-43
    normY = np.sqrt((Y0 ** 2).sum((1, 2), keepdims=True))
    X0, Y0 = X0 / normX, Y0 / normY
    H = np.matmul(X0.transpose(0, 2, 1), Y0)                                           # :48
    U, s, Vt = np.linalg.svd(H)
    V = Vt.transpose(0, 2, 1)
    R = np.matmul(V, U.transpose(0, 2, 1))
    sign = np.sign(np.expand_dims(np.linalg.det(R), 1))                                # :54-58
    V[:, :, -1] *= sign
    s[:, -1] *= sign.flatten()
    R = np.matmul(V, U.transpose(0, 2, 1))
    tr = np.expand_dims(s.sum(1, keepdims=True), 2)
    a = tr * normX / normY                                                             # :62
    t = muX - a * np.matmul(muY, R)
    aligned = a * np.matmul(Y, R) + t                                                  # :66
    return np.linalg.norm(aligned - X, axis=-1).mean(-1)


def p_mpjpe_horn_per_pose(pred, gt):
    """The SAME quantity by the route the HIP kernel takes (csrc/metrics.hip): Horn's quaternion closed form — top
    eigenpair of the symmetric 4x4 matrix built from S = sum_j Y0_j X0_j^T — so that the algebra of the kernel is
    checked against the SVD form on the CPU, not only on the GPU."""
    X, Y = gt.astype(np.float64), pred.astype(np.float64)
    out = np.empty(X.shape[0])
    for i in range(X.shape[0]):
        muX, muY = X[i].mean(0), Y[i].mean(0)
        x0, y0 = X[i] - muX, Y[i] - muY
        nX, nY = np.sqrt((x0 ** 2).sum()), np.sqrt((y0 ** 2).sum())
        S = (y0.T @ x0) / (nX * nY)
        N = np.array([
            [S[0, 0] + S[1, 1] + S[2, 2], S[1, 2] - S[2, 1], S[2, 0] - S[0, 2], S[0, 1] - S[1, 0]],
            [S[1, 2] - S[2, 1], S[0, 0] - S[1, 1] - S[2, 2], S[0, 1] + S[1, 0], S[2, 0] + S[0, 2]],
            [S[2, 0] - S[0, 2], S[0, 1] + S[1, 0], -S[0, 0] + S[1, 1] - S[2, 2], S[1, 2] + S[2, 1]],
            [S[0, 1] - S[1, 0], S[2, 0] + S[0, 2], S[1, 2] + S[2, 1], -S[0, 0] - S[1, 1] + S[2, 2]]])
        lam, vec = np.linalg.eigh(N)
        w, x, y, z = vec[:, -1]
        R = np.array([[w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z]])
        a = lam[-1] * nX / nY
        aligned = a * (y0 @ R.T) + muX
        out[i] = np.linalg.norm(aligned - X[i], axis=-1).mean()
    return out


def n_mpjpe_per_pose(pred, gt):
    """loss.py:71-84 per pose: scale = mean_j(sum_c gt*pred) / mean_j(sum_c pred^2)."""
    X, Y = gt.astype(np.float64), pred.astype(np.float64)
    scale = (X * Y).sum(-1).mean(-1) / (Y ** 2).sum(-1).mean(-1)
    return np.linalg.norm(scale[:, None, None] * Y - X, axis=-1).mean(-1)


def _horn_matrix(pred, gt):
    """-> (N [n,4,4], nX [n], nY [n], muX, muY, X, Y): the symmetric 4x4 matrix of Horn's closed form for every pose, float64."""
    X, Y = gt.astype(np.float64), pred.astype(np.float64)
    muX, muY = X.mean(1, keepdims=True), Y.mean(1, keepdims=True)
    X0, Y0 = X - muX, Y - muY
    nX, nY = np.sqrt((X0 ** 2).sum((1, 2))), np.sqrt((Y0 ** 2).sum((1, 2)))
    with np.errstate(divide="ignore", invalid="ignore"):
        S = np.matmul(Y0.transpose(0, 2, 1), X0) * (1.0 / (nX * nY))[:, None, None]          # S[a][b] = sum_j Y0[j][a] X0[j][b]
    N = np.empty((X.shape[0], 4, 4))
    N[:, 0, 0] = S[:, 0, 0] + S[:, 1, 1] + S[:, 2, 2]
    N[:, 1, 1] = S[:, 0, 0] - S[:, 1, 1] - S[:, 2, 2]
    N[:, 2, 2] = -S[:, 0, 0] + S[:, 1, 1] - S[:, 2, 2]
    N[:, 3, 3] = -S[:, 0, 0] - S[:, 1, 1] + S[:, 2, 2]
    N[:, 0, 1] = N[:, 1, 0] = S[:, 1, 2] - S[:, 2, 1]
    N[:, 0, 2] = N[:, 2, 0] = S[:, 2, 0] - S[:, 0, 2]
    N[:, 0, 3] = N[:, 3, 0] = S[:, 0, 1] - S[:, 1, 0]
    N[:, 1, 2] = N[:, 2, 1] = S[:, 0, 1] + S[:, 1, 0]
    N[:, 1, 3] = N[:, 3, 1] = S[:, 2, 0] + S[:, 0, 2]
    N[:, 2, 3] = N[:, 3, 2] = S[:, 1, 2] + S[:, 2, 1]
    return N, nX, nY, muX, muY, X, Y


def horn_condition(pred, gt):
    """-> (nX [n], nY [n], gap [n]): the centred norms loss.py:42-43 divides by, and the distance between the two largest
    eigenvalues of the 4x4 matrix whose top eigenvector csrc/metrics.hip takes (LAPACK eigvalsh): what a test asserts about its
    inputs before it holds the kernel's eigen-solver to a bound."""
    N, nX, nY = _horn_matrix(pred, gt)[:3]
    ok = np.isfinite(N).all((1, 2))                  # (a pose with nX nY == 0 has no matrix: its gap is NaN)
    gap = np.full(N.shape[0], np.nan)
    lam = np.linalg.eigvalsh(N[ok])
    gap[ok] = lam[:, 3] - lam[:, 2]
    return nX, nY, gap


def p_mpjpe_jacobi_per_pose(pred, gt):
    """loss.py:25-68 by the arithmetic of csrc/metrics.hip, statement for statement (top_eigen4: cyclic Jacobi, at most 12 sweeps,
    stop below an off-diagonal square sum of 1e-30, rotations skipped below 1e-300; then the quaternion's rotation matrix, the
    scale and the aligned error), in numpy float64 and batched over the poses: a pose that has converged, and a rotation that is
    skipped, take c = 1, s = 0, which changes nothing.  -> (per-pose P_MPJPE [n], sweeps used [n])."""
    A, nX, nY, muX, muY, X, Y = _horn_matrix(pred, gt)
    n = A.shape[0]
    V = np.broadcast_to(np.eye(4), (n, 4, 4)).copy()
    sweeps = np.zeros(n, np.int64)
    done = np.zeros(n, bool)
    for sweep in range(12):
        off = np.zeros(n)
        for p in range(4):
            for r in range(p + 1, 4):
                off += A[:, p, r] * A[:, p, r]
        done |= off < 1e-30
        if done.all():
            break
        sweeps += ~done
        for p in range(3):
            for r in range(p + 1, 4):
                apr = A[:, p, r]
                skip = done | (np.abs(apr) < 1e-300)
                with np.errstate(divide="ignore", invalid="ignore"):
                    theta = (A[:, r, r] - A[:, p, p]) / (2.0 * apr)
                    t = np.where(theta >= 0, 1.0, -1.0) / (np.abs(theta) + np.sqrt(theta * theta + 1.0))
                c = np.where(skip, 1.0, 1.0 / np.sqrt(t * t + 1.0))
                s = np.where(skip, 0.0, t * c)
                c, s = c[:, None], s[:, None]
                akp, akr = A[:, :, p].copy(), A[:, :, r].copy()                # A <- A J (columns p, r)
                A[:, :, p], A[:, :, r] = c * akp - s * akr, s * akp + c * akr
                apk, ark = A[:, p, :].copy(), A[:, r, :].copy()                # A <- J^T A (rows p, r)
                A[:, p, :], A[:, r, :] = c * apk - s * ark, s * apk + c * ark
                vkp, vkr = V[:, :, p].copy(), V[:, :, r].copy()
                V[:, :, p], V[:, :, r] = c * vkp - s * vkr, s * vkp + c * vkr
    diag = np.stack([A[:, i, i] for i in range(4)], 1)
    best = np.zeros(n, np.int64)
    for i in range(1, 4):
        better = diag[:, i] > diag[np.arange(n), best]
        best = np.where(better, i, best)
    q = V[np.arange(n), :, best]
    tr = diag[np.arange(n), best]
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = np.empty((n, 3, 3))
    R[:, 0, 0], R[:, 0, 1], R[:, 0, 2] = w * w + x * x - y * y - z * z, 2 * (x * y - w * z), 2 * (x * z + w * y)
    R[:, 1, 0], R[:, 1, 1], R[:, 1, 2] = 2 * (x * y + w * z), w * w - x * x + y * y - z * z, 2 * (y * z - w * x)
    R[:, 2, 0], R[:, 2, 1], R[:, 2, 2] = 2 * (x * z - w * y), 2 * (y * z + w * x), w * w - x * x - y * y + z * z
    a = tr * nX / nY
    aligned = a[:, None, None] * np.matmul(Y - muY, R.transpose(0, 2, 1)) + muX
    return np.linalg.norm(aligned - X, axis=-1).mean(-1), sweeps


def velocity_errors(pred, gt, prev=None):
    """loss.py:87-101 before the mean (float32 first differences, like np.diff on fp32 arrays).  prev None: [N,J,3] -> [N-1], rows
    i and i-1.  prev [N] ints: row i against row prev[i], the pairing np.diff makes once a boolean mask has selected the rows of
    one action (human36m.py:371-376) -> [N], 0 where prev[i] < 0 (no predecessor; such a row is in no mean)."""
    if prev is None:
        vp, vg = np.diff(pred, axis=0), np.diff(gt, axis=0)
        return np.linalg.norm((vp - vg).astype(np.float64), axis=-1).mean(-1)
    prev = np.asarray(prev)
    has = prev >= 0
    out = np.zeros(pred.shape[0])
    vp, vg = pred[has] - pred[prev[has]], gt[has] - gt[prev[has]]
    out[has] = np.linalg.norm((vp - vg).astype(np.float64), axis=-1).mean(-1)
    return out


def per_action(pred, gt, action_idx, n_actions):
    """human36m.py:370-383: [n_actions, 4] = frame_count * {MPJPE, P_MPJPE, MPJVE}, frame_count."""
    out = np.zeros((n_actions, 4))
    for a in range(n_actions):
        m = action_idx == a
        n = np.count_nonzero(m)
        out[a] = [mpjpe_per_pose(pred[m], gt[m]).sum(), p_mpjpe_per_pose(pred[m], gt[m]).sum(),
                  n * velocity_errors(pred[m], gt[m]).mean(), n]
    return out


def per_action_scores(pred, gt, action_idx, action_names):
    """human36m.py:370-416 in float64: per action frame_count * mean of the per-pose errors over the rows a boolean mask selects
    (:370-384), the '-1' / '-2' trials of an action added up (:386-407), everything divided by the frame count (:409-416).
    pred / gt [N,J,3], action_idx [N] -> {name: {'MPJPE', 'P_MPJPE', 'MPJVE'}}.  An action without frames has the mean of nothing,
    NaN, as the reference's `frame_count * e1(empty)` has, and the NaN goes into the merged action.  An action of ONE frame has an
    MPJVE of NaN (no pair of rows) and finite MPJPE / P_MPJPE: the reference raises there, since `.squeeze()` (:374, :376) drops
    the frame axis as well; mvn/datasets/human36m.py documents the choice this restates."""
    action_idx = np.asarray(action_idx)
    nan = np.float64("nan")
    scores = {}
    for a, name in enumerate(action_names):
        m = action_idx == a
        n = int(np.count_nonzero(m))
        p, g = pred[m], gt[m]
        scores[name] = {"MPJPE": n * mpjpe_per_pose(p, g).mean() if n else nan,
                        "P_MPJPE": n * p_mpjpe_per_pose(p, g).mean() if n else nan,
                        "MPJVE": n * velocity_errors(p, g).mean() if n > 1 else nan, "frame_count": n}
    for base in [name[:-2] for name in action_names if name.endswith("-1")]:
        combined = {"MPJPE": np.float64(0.0), "P_MPJPE": np.float64(0.0), "MPJVE": np.float64(0.0), "frame_count": 0}
        for trial in 1, 2:
            one = scores.pop("%s-%d" % (base, trial))
            for k in combined:
                combined[k] = combined[k] + one[k]
        scores[base] = combined
    with np.errstate(divide="ignore", invalid="ignore"):
        return {k: {m: np.float64(v[m]) / np.float64(v["frame_count"]) for m in ("MPJPE", "P_MPJPE", "MPJVE")} for k, v in scores.items()}


def keypoints_loss(mode, pred, gt, validity, threshold=0.0):
    """loss.py:104-137: mode 0 MSE, 1 MSESmooth, 2 MAE.  pred/gt [...,D], validity [...,1]."""
    p, g, v = pred.astype(np.float64), gt.astype(np.float64), validity.astype(np.float64)
    D = p.shape[-1]
    if mode == 2:
        diff = np.abs(g - p) * v
    else:
        diff = (g - p) ** 2 * v
        if mode == 1:
            big = diff > threshold
            diff[big] = diff[big] ** 0.1 * threshold ** 0.9
    return diff.sum() / (D * max(1.0, v.sum()))
