"""Per-action evaluation of gathered predictions — the part of `Human36MMultiViewDataset` the training script
calls after validation (ContextPose/mvn/datasets/human36m.py:358-435 `evaluate_using_pred` / `evaluate`;
consumed at ContextPose/train.py:381-436).  The dataset itself (labels, images, OpenCV crops) is out of scope
(DESIGN.md §7); what is here is the arithmetic: per-pose MPJPE / P-MPJPE / MPJVE on the GPU (capf_pose_errors),
per-action fp64 sums (capf_segment_sums), and the reference's merging of the '-1' / '-2' trials of an action.
The 2-D half of the class is here too (human36m.py:438-479 `evaluate_2d_joint` / `evaluate2d`): the PCKh table per joint and group at a
list of thresholds, from the integer counts of capf_pck2d_counts (evaluate2d, Pck2dAccumulator, pck2d_tables)."""
import numpy as np
import torch

from capf import lib as _capf


def pck2d_tables(counts, valid, err_sums, thresholds, group_names=('all',), joint_names=None):
    """The tables of evaluate2d (human36m.py:451-479) from the integers of capf_pck2d_counts, formed on the host in float64.
    counts [G, K, J], valid [G, J], err_sums [G, J] (numpy or tensors); thresholds: the K keys; group_names: G names; joint_names: J names
    (None: 'joint_0' ...).  Returns (name_values_dict, mean_rate_dict, mean_error_dict):
        name_values_dict[thres][group][joint_name] = counts / valid            (evaluate_2d_joint's joint_detection_rate)
        mean_rate_dict[thres][group]               = np.mean of the group's per-joint rates
        mean_error_dict[group][joint_name]         = err_sums / valid          (mean normalised error; no reference counterpart)
    A joint with valid == 0 gets NaN and is left out of the mean; a group without any valid joint has a NaN mean."""
    from collections import OrderedDict
    to_np = lambda a: a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    counts, valid, err_sums = to_np(counts), to_np(valid), to_np(err_sums).astype(np.float64)
    G, K, J = counts.shape
    thresholds, group_names = list(thresholds), list(group_names)
    joint_names = ['joint_%d' % j for j in range(J)] if joint_names is None else list(joint_names)
    if valid.shape != (G, J) or err_sums.shape != (G, J) or len(thresholds) != K or len(group_names) != G or len(joint_names) != J:
        raise ValueError('counts %s need valid / err_sums %s, %d thresholds, %d group names and %d joint names' % (counts.shape, (G, J), K, G, J))
    denom = valid.astype(np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        rates = np.where(denom[:, None, :] > 0, counts.astype(np.float64) / denom[:, None, :], np.nan)        # np.sum(detected, axis=0) / np.float(n)  (:442)
        errors = np.where(denom > 0, err_sums / denom, np.nan)
    name_values_dict, mean_rate_dict = {}, {}
    for k, thres in enumerate(thresholds):
        name_values_dict[thres], mean_rate_dict[thres] = {}, {}
        for g, group in enumerate(group_names):
            name_values_dict[thres][group] = OrderedDict((joint_names[j], rates[g, k, j]) for j in range(J))
            seen = rates[g, k][denom[g] > 0]
            mean_rate_dict[thres][group] = np.mean(seen) if seen.size else np.float64('nan')          # np.mean(joint_detection_rate)  (:449)
    mean_error_dict = {group: OrderedDict((joint_names[j], errors[g, j]) for j in range(J)) for g, group in enumerate(group_names)}
    return name_values_dict, mean_rate_dict, mean_error_dict


class Pck2dAccumulator:
    """evaluate2d over the batches of an evaluation epoch: the integer outputs of capf_pck2d_counts are added on the device batch after
    batch (no synchronisation per batch) and the tables are built once, by tables() -- the epoch's only device-to-host copy.
    thresholds, headsize, segment_names, joint_names: as evaluate2d.  Group 0 is 'all', group 1 + s the s-th of segment_names.
    counts and valid are exact integers, equal to one call on the concatenated input; err_sums is the fp64 sum of the batches' sums."""

    def __init__(self, thresholds, headsize, segment_names=None, joint_names=None):
        self.thresholds = list(thresholds)
        self.scaled = [float(headsize) * float(t) for t in self.thresholds]          # headsize * threshold in double (:440)
        self.segment_names = None if segment_names is None else list(segment_names)
        self.group_names = ['all'] + (self.segment_names or [])
        self.joint_names = None if joint_names is None else list(joint_names)
        self.counts = self.valid = self.err_sums = None

    def add(self, counts, valid, err_sums):
        """Add one batch's (counts [G, K, J], valid [G, J], err_sums [G, J]) tensors, group 0 = 'all'; stays on their device.  The running
        totals are the accumulator's own tensors: the caller's are only read and may be reused (capf.lib.pck2d_counts' out=)."""
        if self.counts is None:
            self.counts, self.valid = counts.to(torch.int64, copy=True), valid.to(torch.int64, copy=True)
            self.err_sums = err_sums.to(torch.float64, copy=True)
        else:
            self.counts += counts
            self.valid += valid
            self.err_sums += err_sums
        return self

    def update(self, keypoints_2d_gt, keypoints_2d_pred, weight=None, segment=None):
        """One batch through capf_pck2d_counts (once for 'all', once more per segment when segment_names were given)."""
        gt, pred, weight, segment = _pck2d_inputs(keypoints_2d_gt, keypoints_2d_pred, weight, segment, self.joint_names, self.segment_names)
        out = _capf.pck2d_counts(pred, gt, self.scaled, weight=weight)
        if self.segment_names is not None:
            by = _capf.pck2d_counts(pred, gt, self.scaled, weight=weight, segment=segment, n_segments=len(self.segment_names))
            out = tuple(torch.cat([a, b]) for a, b in zip(out, by))
        return self.add(*out)

    def tables(self):
        if self.counts is None:
            raise ValueError('Pck2dAccumulator.tables() before any batch')
        return pck2d_tables(self.counts, self.valid, self.err_sums, self.thresholds, self.group_names, self.joint_names)


def _pck2d_inputs(keypoints_2d_gt, keypoints_2d_pred, weight, segment, joint_names, segment_names):
    # the device of whichever input is on one already (pred first); the current CUDA device for host arrays
    dev = next((x.device for x in (keypoints_2d_pred, keypoints_2d_gt, weight, segment) if torch.is_tensor(x) and x.is_cuda), torch.device('cuda'))
    as32 = lambda x: torch.as_tensor(x).to(device=dev, dtype=torch.float32)
    if tuple(keypoints_2d_pred.shape) != tuple(keypoints_2d_gt.shape):
        raise ValueError('`keypoints_2d_pred` shape should be %s, got %s' % (tuple(keypoints_2d_gt.shape), tuple(keypoints_2d_pred.shape)))
    J = keypoints_2d_gt.shape[-2] if joint_names is None else len(joint_names)
    gt, pred = as32(keypoints_2d_gt).reshape(-1, J, 2).contiguous(), as32(keypoints_2d_pred).reshape(-1, J, 2).contiguous()      # (:456-457)
    n = gt.shape[0]
    if weight is not None:
        weight = as32(weight).reshape(n, J).contiguous()
    if (segment is None) != (segment_names is None):
        raise ValueError('segment (the group index per pose) and segment_names go together')
    if segment is not None:
        segment = torch.as_tensor(segment).to(device=dev, dtype=torch.int32).reshape(-1).contiguous()
        if segment.numel() != n:
            raise ValueError('segment needs %d labels, got %d' % (n, segment.numel()))
    return gt, pred, weight, segment


def evaluate2d(keypoints_2d_gt, keypoints_2d_pred, thresholds, headsize, weight=None, segment=None, segment_names=None, joint_names=None):
    """human36m.py:451-479 (`evaluate2d` / `evaluate_2d_joint`): the PCKh table per joint and per group at a list of thresholds.
    keypoints_2d_* [..., J, 2] (CUDA tensors or numpy; reshaped to (-1, J, 2) as the reference does), thresholds: fractions of
    headsize (the reference: config.model.image_shape[0] / 10.0); a sample is detected iff distance <= headsize * threshold.
    weight [n, J]: samples with weight <= 0 are left out (None: all count, the reference's case).  segment [n] ints with segment_names:
    one more group per name (the reference hard-codes its 's9' / 's11' split as row 5012; here the caller passes the subject index per
    pose; an index outside the names belongs to 'all' only).  joint_names: J names in joint order (None: 'joint_0' ...).
    Returns (name_values_dict[thres][group][joint_name], mean_rate_dict[thres][group]) exactly like the reference, group = 'all' + the
    segment names, and as a third value mean_error_dict[group][joint_name], the mean distance in pixels.  The distances, comparisons
    and sums run on the GPU (capf_pck2d_counts); the rates are formed here from its integers (pck2d_tables)."""
    return Pck2dAccumulator(thresholds, headsize, segment_names, joint_names).update(keypoints_2d_gt, keypoints_2d_pred, weight, segment).tables()


def previous_in_segment(segment):
    """prev[i] = largest j < i with segment[j] == segment[i], else -1: the row np.diff pairs row i with once the
    rows of one action have been selected by a boolean mask (human36m.py:371-376, loss.py:98-99)."""
    segment = np.asarray(segment)
    prev = np.full(segment.shape[0], -1, np.int32)
    last = {}
    for i, a in enumerate(segment.tolist()):
        prev[i] = last.get(a, -1)
        last[a] = i
    return prev


def evaluate_using_pred(keypoints_gt, keypoints_3d_predicted, labels_action_idx, action_names):
    """human36m.py:358-417.  keypoints_* [N,1,17,3] (CUDA tensors or numpy), labels_action_idx [N] ints,
    action_names: list of 'Name-1' / 'Name-2' strings indexed by action idx.
    Returns {action (trials merged): {'MPJPE','P_MPJPE','MPJVE'}} exactly like the reference."""
    if tuple(keypoints_3d_predicted.shape) != tuple(keypoints_gt.shape):
        raise ValueError('`keypoints_3d_predicted` shape should be %s, got %s' %
                         (tuple(keypoints_gt.shape), tuple(keypoints_3d_predicted.shape)))       # human36m.py:422-425
    from mvn.models.loss import _poses
    pred, gt = _poses(keypoints_3d_predicted), _poses(keypoints_gt)
    seg_host = np.asarray(labels_action_idx).astype(np.int32)
    dev = pred.device
    seg = torch.from_numpy(seg_host).to(dev)
    prev = torch.from_numpy(previous_in_segment(seg_host)).to(dev)
    err = _capf.pose_errors(pred, gt, prev)
    sums, counts = _capf.segment_sums(err, seg, prev, n_segments=len(action_names))
    sums, counts = sums.cpu().numpy(), counts.cpu().numpy()

    # An action with no frames in the evaluated subset: the reference's e1 / e2 / ev on empty arrays are NaN (mean of nothing) and
    # the NaN propagates into the merged action; values stay numpy scalars so n == 0 divides to NaN instead of raising.
    nan = np.float64('nan')
    action_scores = {}
    for a, name in enumerate(action_names):
        n, pairs = int(counts[a, 0]), int(counts[a, 1])
        # the reference stores frame_count * mean(...) per action (:373-376); MPJVE's mean runs over n-1 pairs
        action_scores[name] = {'MPJPE': np.float64(sums[a, 0]) if n > 0 else nan, 'P_MPJPE': np.float64(sums[a, 1]) if n > 0 else nan,
                               'MPJVE': np.float64(n * (sums[a, 3] / pairs)) if pairs > 0 else nan, 'frame_count': n}
    for base in [name[:-2] for name in action_names if name.endswith('-1')]:                   # :386-406
        combined = {'MPJPE': np.float64(0.0), 'P_MPJPE': np.float64(0.0), 'MPJVE': np.float64(0.0), 'frame_count': 0}
        for trial in 1, 2:
            key = '%s-%d' % (base, trial)
            for k in combined:
                combined[k] = combined[k] + action_scores[key][k]
            del action_scores[key]
        action_scores[base] = combined
    with np.errstate(divide='ignore', invalid='ignore'):
        for k in action_scores:                                                               # :408-415
            n = np.float64(action_scores[k]['frame_count'])
            action_scores[k] = {'MPJPE': action_scores[k]['MPJPE'] / n, 'P_MPJPE': action_scores[k]['P_MPJPE'] / n,
                                'MPJVE': action_scores[k]['MPJVE'] / n}
    return action_scores
