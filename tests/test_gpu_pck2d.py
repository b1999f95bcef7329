"""GPU: capf_pck2d_counts against its float64 restatement (pck2d_oracle.py).  counts and valid are integers produced by the same IEEE
operations on both sides and must be EQUAL; err_sums is bit-equal between calls and buffers, equals the restatement's sum taken in the
stated order, and lies within (ceil(n / 256) + 8) 2^-53 sum|e| of math.fsum.  Outputs are filled with -1 / NaN before every call, so an
element the call did not write shows.  evaluate2d and Pck2dAccumulator on the device are held to the same restatement."""
import numpy as np
import pytest
import torch

import pck2d_oracle as O
from capf import lib as capf

pytestmark = pytest.mark.gpu


def _run(pred, gt, thresholds, norm=None, weight=None, strict=False, segment=None, n_segments=1):
    """the binding on prefilled outputs -> numpy (counts, valid, err_sums)"""
    put = lambda a, dt: None if a is None else torch.as_tensor(np.asarray(a)).to(dt).cuda()
    n, J = gt.shape[0], gt.shape[1]
    K = len(thresholds)
    out = (torch.full((n_segments, K, J), -1, dtype=torch.int32, device="cuda"), torch.full((n_segments, J), -1, dtype=torch.int32, device="cuda"),
           torch.full((n_segments, J), float("nan"), dtype=torch.float64, device="cuda"))
    got = capf.pck2d_counts(put(pred, torch.float32), put(gt, torch.float32), thresholds, put(norm, torch.float32), put(weight, torch.float32),
                            strict, put(segment, torch.int32), n_segments, out=out)
    assert all(a is b for a, b in zip(got, out))
    return tuple(t.cpu().numpy() for t in got)


def _data(n, J, seed, spread=6.0):
    rng = np.random.RandomState(seed)
    gt = rng.uniform(0, 64, (n, J, 2)).astype(np.float32)
    pred = (gt + rng.normal(0, spread, gt.shape)).astype(np.float32)
    return rng, pred, gt


def _same(got, want, e, use_of):
    """integers equal; the sum equal to the ordered restatement bit for bit and within the stated bound of fsum"""
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.float64
    assert np.array_equal(got[2].view(np.int64), want[2].view(np.int64))
    S, J = want[1].shape
    for s in range(S):
        for j in range(J):
            exact, bound = O.fsum_bound(e[:, j], use_of(s)[:, j])
            assert abs(got[2][s, j] - exact) <= bound, (s, j, got[2][s, j], exact, bound)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 1000])
@pytest.mark.parametrize("J,K", [(1, 32), (17, 1), (32, 32), (17, 10)])
def test_counts_equal_the_restatement_at_every_size(n, J, K):
    rng, pred, gt = _data(n, J, 100 * n + J)
    thresholds = [6.4 * t for t in np.linspace(0.05, 2.0, K)] if K > 1 else [3.2]
    for strict in (False, True):
        got = _run(pred, gt, thresholds, strict=strict)
        c, v, s, e, ok = O.pck2d_counts(pred, gt, thresholds, strict=strict)
        _same(got, (c, v, s), e, lambda _s: ok)
        assert (v == n).all()
    if n == 0:
        assert not got[0].any() and not got[1].any() and not got[2].any()
        # no pose, three segments: an empty segment array has no address, the entry takes NULL and writes every zero
        got = _run(pred, gt, thresholds, segment=np.zeros(0, np.int32), n_segments=3)
        assert got[0].shape == (3, K, J) and not got[0].any() and not got[1].any() and not got[2].any() and not np.isnan(got[2]).any()
    else:
        assert 0 < got[0].sum() < n * J * K or K == 1


def test_ties_are_detected_under_le_and_not_under_lt():
    gt = np.zeros((3, 2, 2), np.float32) + 7
    pred = gt + np.array([[[3, 4], [6, 16]], [[4, 3], [6, 16]], [[3, 4.00001], [6, 16.00001]]], np.float32)       # two ties, one just over
    norm = np.array([[2, 4]] * 3, np.float32)
    le, lt = _run(pred, gt, [5.0]), _run(pred, gt, [5.0], strict=True)
    assert le[0][0, 0].tolist() == [2, 0] and lt[0][0, 0].tolist() == [0, 0]
    le, lt = _run(pred, gt, [5.0], norm=norm), _run(pred, gt, [5.0], norm=norm, strict=True)
    assert le[0][0, 0].tolist() == [3, 2] and lt[0][0, 0].tolist() == [3, 0]          # (joint 0 under the norm: e = sqrt(1.5^2 + 1) < 5)
    for strict in (False, True):
        for nm in (None, norm):
            want = O.pck2d_counts(pred, gt, [5.0], norm=nm, strict=strict)
            got = _run(pred, gt, [5.0], norm=nm, strict=strict)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[2].view(np.int64), want[2].view(np.int64))


def test_validity_weight_norm_and_segments():
    n, J, S = 600, 17, 3
    rng, pred, gt = _data(n, J, 7)
    w = rng.choice([1.0, 0.5, 0.0, -1.0], (n, J)).astype(np.float32)
    w[:, 4] = 0                                                     # a joint with no valid sample: valid 0, sum 0
    norm = rng.uniform(4, 8, (n, 2)).astype(np.float32)
    norm[3], norm[40], norm[300, 1], norm[301, 0], norm[599] = (0, 5), (5, -1), np.inf, np.nan, (-np.inf, 2)      # skipped for every joint
    seg = rng.randint(-1, S + 1, n).astype(np.int32)               # -1 and 3 present: skipped
    seg[seg == 1] = 0                                               # segment 1 has no poses
    assert (seg == -1).any() and (seg == S).any() and not (seg == 1).any()
    thresholds = [0.25, 0.5, 1.0]
    for kw in (dict(weight=w), dict(norm=norm), dict(segment=seg, n_segments=S), dict(weight=w, norm=norm, segment=seg, n_segments=S, strict=True)):
        got = _run(pred, gt, thresholds, **kw)
        c, v, s, e, _ = O.pck2d_counts(pred, gt, thresholds, **kw)
        ok, sid = O.valid_mask(n, J, kw.get("norm"), kw.get("weight"), kw.get("segment"), kw.get("n_segments", 1))
        _same(got, (c, v, s), e, lambda q: ok & (sid == q)[:, None])
    assert (got[1][:, 4] == 0).all() and (got[2][:, 4] == 0).all() and (got[0][:, :, 4] == 0).all()
    assert not got[1][1].any() and not got[2][1].any() and not got[0][1].any() and got[1][0].sum() > 0 and got[1][2].sum() > 0
    only_norm = _run(pred, gt, thresholds, norm=norm)
    assert (only_norm[1] == n - 5).all()


def test_non_finite_distances_stay_in_their_joint_and_segment():
    n, J = 300, 5
    rng, pred, gt = _data(n, J, 11)
    seg = (np.arange(n) % 2).astype(np.int32)
    clean = _run(pred, gt, [3.0, 9.0], segment=seg, n_segments=2)
    bad = pred.copy()
    bad[10, 1, 0] = np.nan                                          # pose 10 is in segment 0
    bad[21, 3, 1] = np.inf                                          # pose 21 in segment 1
    got = _run(bad, gt, [3.0, 9.0], segment=seg, n_segments=2)
    want = O.pck2d_counts(bad, gt, [3.0, 9.0], segment=seg, n_segments=2)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert np.array_equal(got[1], clean[1])                         # they count as valid
    assert np.isnan(got[2][0, 1]) and got[2][1, 3] == np.inf
    assert (got[0][0, :, 1] <= clean[0][0, :, 1]).all() and (got[0][1, :, 3] <= clean[0][1, :, 3]).all()      # and fail every threshold
    e_clean = O.pck2d_counts(pred, gt, [3.0, 9.0])[3]
    assert np.array_equal(clean[0][0, :, 1] - got[0][0, :, 1], (e_clean[10, 1] <= np.array([3.0, 9.0])).astype(np.int32))
    keep = np.ones((2, J), bool)
    keep[0, 1] = keep[1, 3] = False
    assert np.array_equal(got[2][keep].view(np.int64), clean[2][keep].view(np.int64))          # every other joint and segment untouched
    assert np.array_equal(got[0][:, 0][keep], clean[0][:, 0][keep]) and np.array_equal(got[0][:, 1][keep], clean[0][:, 1][keep])


def test_same_bits_on_every_call_and_in_every_buffer():
    n, J = 1000, 17
    rng, pred, gt = _data(n, J, 13)
    seg = rng.randint(0, 4, n).astype(np.int32)
    args = (torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda(), [1.0, 2.0, 4.0])
    kw = dict(segment=torch.from_numpy(seg).cuda(), n_segments=4)
    a = capf.pck2d_counts(*args, **kw)
    b = capf.pck2d_counts(*args, **kw)
    assert all(x.data_ptr() != y.data_ptr() for x, y in zip(a, b))
    c = capf.pck2d_counts(*args, out=a, **kw)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x.view(-1).view(torch.int32), y.view(-1).view(torch.int32)) and z is x


def test_evaluate2d_and_the_accumulator_on_the_device():
    from mvn.datasets.human36m import Pck2dAccumulator, evaluate2d, pck2d_tables
    n, J = 90, 17
    rng, pred, gt = _data(2 * n, J, 17, spread=4.0)
    gt4, pred4 = gt.reshape(n, 2, J, 2), pred.reshape(n, 2, J, 2)             # (b, n_views, 17, 2), as the reference's callers pass
    seg = rng.randint(0, 2, 2 * n).astype(np.int32)
    thresholds, headsize = [0.5, 0.75, 1.0], 6.4
    names = ["j%d" % j for j in range(J)]
    nv, mr, me = evaluate2d(torch.from_numpy(gt4).cuda(), pred4, thresholds, headsize, segment=seg, segment_names=["s9", "s11"], joint_names=names)
    scaled = [headsize * t for t in thresholds]
    a = O.pck2d_counts(pred, gt, scaled)[:3]
    b = O.pck2d_counts(pred, gt, scaled, segment=seg, n_segments=2)[:3]
    want = pck2d_tables(*(np.concatenate(x) for x in zip(a, b)), thresholds, ["all", "s9", "s11"], names)
    for t in thresholds:
        assert list(nv[t]) == ["all", "s9", "s11"]
        for g in nv[t]:
            assert list(nv[t][g].items()) == list(want[0][t][g].items()) and mr[t][g] == want[1][t][g]
    assert all(list(me[g].values()) == list(want[2][g].values()) for g in me)
    acc = Pck2dAccumulator(thresholds, headsize, ["s9", "s11"], names)
    for lo, hi in ((0, 50), (50, 51), (51, 2 * n)):
        acc.update(gt[lo:hi], torch.from_numpy(pred[lo:hi]).cuda(), segment=seg[lo:hi])
    assert acc.counts.is_cuda
    nv2, mr2, _ = acc.tables()
    assert all(list(nv2[t][g].items()) == list(nv[t][g].items()) and mr2[t][g] == mr[t][g] for t in thresholds for g in nv[t])
    # add() with one output buffer reused by successive calls (out=): the totals are the accumulator's own
    acc2, out = Pck2dAccumulator(thresholds, headsize, None, names), None
    d_pred, d_gt = torch.from_numpy(pred).cuda(), torch.from_numpy(gt).cuda()
    for lo, hi in ((0, 50), (50, 51), (51, 2 * n)):
        out = capf.pck2d_counts(d_pred[lo:hi], d_gt[lo:hi], acc2.scaled, out=out)
        acc2.add(*out)
    assert torch.equal(acc2.counts[0], acc.counts[0]) and torch.equal(acc2.valid[0], acc.valid[0]) and torch.equal(acc2.err_sums[0], acc.err_sums[0])
    last = O.pck2d_counts(pred[51:], gt[51:], acc2.scaled)
    assert np.array_equal(out[0].cpu().numpy(), last[0]) and np.array_equal(out[2].cpu().numpy().view(np.int64), last[2].view(np.int64))
