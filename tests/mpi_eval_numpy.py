"""A numpy restatement of the MPI-INF-3DHP evaluation (ContextPose_mpi/3dhp_test/test_util, MATLAB), written from the formulas, for the
tests of capf_pck_counts and mvn/datasets/mpi_inf_3dhp.py.  It works on the per-pose, per-joint errors directly (the MATLAB's
`error_data(i).error`, nj x 1 x nf) and shares no code with the library.

  mpii_test_predictions_py.m:46   P = gt - gt(:, 15)                     (1-based joint 15: the root)
                            :50-51 e = sqrt(sum((pred - P).^2, 1))        (pred's root joint zeroed by run_3dhp.py:118)
  mpii_compute_3d_pck.m:20-21     thresh = 0:5:150, pck_thresh = 150
                       :30        curve_g(t) = sum(sum(e(g, :) < t, 3), 1) / (numel(g) nf)
                       :33-38     joint_count += numel(g);  curve_total += curve_g numel(g)
                       :39        auc_g = 100 sum(curve_g) / numel(thresh)
                       :40-45     pck_g = 100 sum(sum(e(g, :) < 150, 3), 1) / (numel(g) nf);  pck_total += pck_g numel(g)
                       :47-49     pck_total /= joint_count;  curve_total /= joint_count;  auc_total = 100 sum(curve_total) / numel(thresh)
  mpii_get_pck_auc_joint_groups.m:4-12  Head [1], Neck [2], Shou [3 6], Elbow [4 7], Wrist [5 8], Hip [9 12], Knee [10 13], Ankle [11 14]
  mpii_evaluate_errors.m:26-28    per sequence: mpjpe = mean(e, 3) per joint, 'Average' = mean over the 17 joints
                       :44-50     per activity 1..7 (all poses whose label is i; none -> NaN), :51-54 'All'
                       :61-64     the activity PCK / AUC rows end with 'All'."""
import numpy as np

GROUPS = ([1], [2], [3, 6], [4, 7], [5, 8], [9, 12], [10, 13], [11, 14])
THRESH = np.arange(0, 151, 5, dtype=np.float64)


def joint_errors(pred, gt, to_mm=1.0, root=14):
    """[n, 17, 3] float32 arrays -> e [n, 17] float64 in mm.  Same operation order as the kernel: ((dx^2 + dy^2) + dz^2), sqrt, x to_mm."""
    p = np.asarray(pred, dtype=np.float32).astype(np.float64).copy()
    g = np.asarray(gt, dtype=np.float32).astype(np.float64)
    P = g - g[:, root:root + 1, :]
    p[:, root, :] = 0.0
    d = p - P
    e2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return np.sqrt(e2) * to_mm


def counts(e, rows_of_pose, n_rows):
    """#(e < t) per row, joint and threshold (int64 [n_rows, 17, 31]), poses per row; rows_of_pose [n] (None: all in row 0)."""
    n, J = e.shape
    rows = np.zeros(n, np.int64) if rows_of_pose is None else np.asarray(rows_of_pose)
    c = np.zeros((n_rows, J, len(THRESH)), np.int64)
    f = np.zeros(n_rows, np.int64)
    for r in range(n_rows):
        sel = e[rows == r]
        f[r] = sel.shape[0]
        c[r] = (sel[:, :, None] < THRESH[None, None, :]).sum(axis=0)
    return c, f


def pck_auc_rows(error_rows):
    """error_rows: list of e [nf, 17] (one per table row) -> pck, auc [rows, 9] (8 groups, Total), straight from the errors."""
    pck = np.zeros((len(error_rows), 9))
    auc = np.zeros((len(error_rows), 9))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i, e in enumerate(error_rows):
            nf = e.shape[0]
            joint_count, curve_total, pck_total = 0, None, 0.0
            for j, grp in enumerate(GROUPS):
                idx = [k - 1 for k in grp]
                curve = np.array([float((e[:, idx] < t).sum()) for t in THRESH]) / (len(idx) * nf)
                joint_count += len(idx)
                curve_total = curve * len(idx) if curve_total is None else curve_total + curve * len(idx)
                auc[i, j] = 100 * curve.sum() / len(THRESH)
                pck[i, j] = 100 * float((e[:, idx] < 150).sum()) / (len(idx) * nf)
                pck_total += pck[i, j] * len(idx)
            pck[i, 8] = pck_total / joint_count
            curve_total = curve_total / joint_count
            auc[i, 8] = 100 * curve_total.sum() / len(THRESH)
    return pck, auc


def mpjpe_rows(error_rows):
    """-> per-joint means [rows, 17] and their mean over joints [rows]; NaN for an empty row (MATLAB's mean over nothing)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        per = np.stack([e.sum(axis=0) / e.shape[0] if e.shape[0] else np.full(e.shape[1], np.nan) for e in error_rows])
    return per, per.mean(axis=1)


def tables(e, sequence, activity):
    """The sequence table (TS1..TS6) and the activity table (1..7, All) of mpii_evaluate_errors.m from e [n, 17]."""
    sequence, activity = np.asarray(sequence), np.asarray(activity)
    seq_rows = [e[sequence == s] for s in range(1, 7)]
    act_rows = [e[activity == a] for a in range(1, 8)] + [e]
    out = {}
    for name, rows in (("sequence", seq_rows), ("activity", act_rows)):
        per, avg = mpjpe_rows(rows)
        pck, auc = pck_auc_rows(rows)
        out[name] = dict(mpjpe=per, mpjpe_average=avg, pck=pck, auc=auc, frames=np.array([r.shape[0] for r in rows]))
    return out


def synthetic_set(n=2929, seed=0, metres=True):
    """pred / gt [n, 17, 3] float32 with errors spread over 0 .. ~250 mm, sequence labels 1..6 and activity labels 1..7 (activity 6
    left empty when n is small, the others all present)."""
    rng = np.random.default_rng(seed)
    scale = 1e-3 if metres else 1.0
    gt = (rng.standard_normal((n, 17, 3)) * 300.0 + np.array([0.0, 0.0, 4000.0])) * scale
    noise = rng.standard_normal((n, 17, 3)) * rng.uniform(5.0, 120.0, size=(n, 17, 1)) * scale
    pred = (gt - gt[:, 14:15]) + noise
    sequence = np.sort(rng.integers(1, 7, size=n))
    activity = rng.integers(1, 8, size=n)
    return pred.astype(np.float32), gt.astype(np.float32), sequence, activity
