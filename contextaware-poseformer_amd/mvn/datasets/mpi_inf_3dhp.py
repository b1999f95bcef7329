"""MPI-INF-3DHP evaluation of gathered predictions: the tables the reference's MATLAB tool writes
(ContextPose_mpi/3dhp_test/test_util: mpii_test_predictions_py.m -> mpii_evaluate_errors.m -> mpii_compute_3d_pck.m with the joint
groups of mpii_get_pck_auc_joint_groups.m), without leaving the GPU for a .mat export.  The per-joint errors and every integer the
tables need come from ONE kernel per grouping (capf_pck_counts); the tables are rebuilt here from those integers in float64.

What the MATLAB computes, restated (1-based MATLAB joints; errors e in mm):
  * mpii_test_predictions_py.m:46, 50-51: P = gt - gt[joint 15] (root-relative ground truth, 0-based joint 14); e = |pred - P|,
    with the prediction's joint 14 zeroed by the caller (run_3dhp.py:118) -- capf_pck_counts applies both.
  * mpii_evaluate_errors.m:26-28 (sequences), 47-49 (activities 1..7), 51-54 ("All"): MPJPE per joint = mean of e over the poses
    of the row; 'Average' = mean of the 17 per-joint means.  An empty row is a mean over nothing: NaN.
  * mpii_compute_3d_pck.m:20-21: thresholds t = 0:5:150, PCK threshold 150.  Per joint group g with |g| joints and nf poses:
      :30  curve_g[t]  = #(e[g] < t) / (|g| nf)                      (strict <)
      :39  AUC_g       = 100 sum_t curve_g[t] / 31
      :40  PCK_g       = 100 #(e[g] < 150) / (|g| nf)
      :35-37, :41-48  Total: curve and PCK weighted by |g| over the groups, divided by the 14 grouped joints (not 17);
      :49  AUC_Total   = 100 sum_t curve_Total[t] / 31
  * mpii_get_pck_auc_joint_groups.m:4-12: Head [1], Neck [2], Shou [3,6], Elbow [4,7], Wrist [5,8], Hip [9,12], Knee [10,13],
    Ankle [11,14] (1-based).
  * mpii_evaluate_errors.m:61-64: the activity table's PCK / AUC rows end with an 'All' row over every pose.
Scene averages (3dhp_test/README.txt) are the frame-weighted means of sequence pairs: scene_table() below."""
import numpy as np
import torch

from capf import lib as _capf

JOINT_GROUPS = (("Head", (1,)), ("Neck", (2,)), ("Shou", (3, 6)), ("Elbow", (4, 7)), ("Wrist", (5, 8)), ("Hip", (9, 12)),
                ("Knee", (10, 13)), ("Ankle", (11, 14)))          # 1-based, mpii_get_pck_auc_joint_groups.m:4-12
GROUP_NAMES = tuple(n for n, _ in JOINT_GROUPS) + ("Total",)
THRESHOLDS = tuple(range(0, 151, 5))                               # mpii_compute_3d_pck.m:20
PCK_THRESHOLD_INDEX = THRESHOLDS.index(150)                        # :21
SEQUENCES = tuple(f"TS{i}" for i in range(1, 7))
ACTIVITIES = ("Standing/Walking", "Exercising", "Sitting", "Reaching/Crouching", "On The Floor", "Sports", "Miscellaneous")
ROOT = 14                                                          # 0-based joint 15 of mpii_test_predictions_py.m:46
SCENES = (("GS", (1, 2)), ("noGS", (3, 4)), ("Outdoor", (5, 6)))  # 3dhp_test/README.txt


def pck_auc(counts, frames):
    """counts int [rows, 17, 31] (#(e < t) per joint and threshold), frames int [rows] -> (pck [rows, 9], auc [rows, 9]) float64, the
    columns in GROUP_NAMES order (eight groups, then Total).  mpii_compute_3d_pck.m:24-50."""
    counts = np.asarray(counts, dtype=np.float64)
    frames = np.asarray(frames, dtype=np.float64)
    rows = counts.shape[0]
    pck = np.zeros((rows, len(GROUP_NAMES)))
    auc = np.zeros((rows, len(GROUP_NAMES)))
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(rows):
            nf = frames[i]
            joint_count = 0
            total_curve = np.zeros(len(THRESHOLDS))
            total_pck = 0.0
            for g, (_, joints) in enumerate(JOINT_GROUPS):
                idx = [j - 1 for j in joints]
                hits = counts[i, idx, :].sum(axis=0)                           # sum over the group's joints, per threshold
                curve = hits / (len(idx) * nf)
                joint_count += len(idx)
                total_curve = total_curve + curve * len(idx)
                auc[i, g] = 100 * curve.sum() / len(THRESHOLDS)
                pck[i, g] = 100 * hits[PCK_THRESHOLD_INDEX] / (len(idx) * nf)
                total_pck = total_pck + pck[i, g] * len(idx)
            pck[i, -1] = total_pck / joint_count
            auc[i, -1] = 100 * (total_curve / joint_count).sum() / len(THRESHOLDS)
    return pck, auc


def mpjpe_table(sums, frames):
    """sums float64 [rows, 17] (error sums), frames [rows] -> (per-joint MPJPE [rows, 17], 'Average' [rows]); NaN for an empty row."""
    sums = np.asarray(sums, dtype=np.float64)
    frames = np.asarray(frames, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        per_joint = sums / frames[:, None]
    return per_joint, per_joint.mean(axis=1)


def _table(names, counts, sums, frames):
    counts, sums, frames = counts.cpu().numpy(), sums.cpu().numpy(), frames.cpu().numpy()
    per_joint, avg = mpjpe_table(sums, frames)
    pck, auc = pck_auc(counts, frames)
    return {"names": list(names), "frames": frames.astype(np.int64), "mpjpe": per_joint, "mpjpe_average": avg, "pck": pck, "auc": auc,
            "groups": list(GROUP_NAMES)}


def evaluate(pred, gt, sequence, activity, to_mm=1.0):
    """The two tables of mpii_evaluate_errors.m for the 3DHP test set.
    pred / gt: [n, 17, 3] (torch CUDA tensors, or anything torch.as_tensor takes; a model output [n, 3, 1, 17, 1] is accepted too) in
    the same unit, to_mm = that unit in mm (1000.0 for metres); sequence: [n] ints 1..6 (TS1..TS6); activity: [n] ints 1..7
    (mpii_get_activity_name.m).  The prediction's root joint (0-based 14) is taken as 0 and the ground truth made root-relative on the
    GPU, as the reference does before it exports.
    Returns {'sequence': table of TS1..TS6, 'activity': table of the 7 activities + 'All'}; a table holds 'names', 'frames',
    'mpjpe' [rows, 17] and 'mpjpe_average' [rows] (mm), 'pck' / 'auc' [rows, 9] in 'groups' order (Head .. Ankle, Total)."""
    dev = torch.device("cuda")

    def dev32(x):
        t = torch.as_tensor(x)
        if t.dim() == 5:                                 # VolumetricTriangulationNet output [n, 3, 1, 17, 1] -> [n, 17, 3]
            t = t.permute(0, 2, 3, 4, 1).reshape(t.shape[0], -1, 3)
        return t.to(device=dev, dtype=torch.float32).contiguous()

    pred, gt = dev32(pred), dev32(gt)
    if pred.shape != gt.shape or gt.dim() != 3 or gt.shape[1:] != (17, 3):
        raise ValueError(f"pred / gt must be [n, 17, 3], got {tuple(pred.shape)} / {tuple(gt.shape)}")
    n = gt.shape[0]
    seq = torch.as_tensor(np.asarray(sequence, dtype=np.int64).reshape(-1) - 1).to(dev, torch.int32)
    act = torch.as_tensor(np.asarray(activity, dtype=np.int64).reshape(-1) - 1).to(dev, torch.int32)
    if seq.numel() != n or act.numel() != n:
        raise ValueError(f"sequence / activity need {n} labels, got {seq.numel()} / {act.numel()}")
    by_seq = _capf.pck_counts(pred, gt, ROOT, to_mm, seq, len(SEQUENCES))
    by_act = _capf.pck_counts(pred, gt, ROOT, to_mm, act, len(ACTIVITIES))
    every = _capf.pck_counts(pred, gt, ROOT, to_mm, None, 1)
    return {"sequence": _table(SEQUENCES, *by_seq),
            "activity": _table(ACTIVITIES + ("All",), *(torch.cat([a, b]) for a, b in zip(by_act, every)))}


def scene_table(seq_table):
    """The scene-setting averages of 3dhp_test/README.txt from a sequence table: studio with green screen (TS1, TS2), without
    (TS3, TS4), outdoor (TS5, TS6); each column the frame-weighted mean of its two sequences."""
    out = {}
    for name, (a, b) in SCENES:
        fa, fb = (float(seq_table["frames"][k - 1]) for k in (a, b))
        out[name] = {key: (seq_table[key][a - 1] * fa + seq_table[key][b - 1] * fb) / (fa + fb)
                     for key in ("mpjpe_average", "pck", "auc")}
    return out
