"""CPU: the host half of the MPI-INF-3DHP evaluation (mvn/datasets/mpi_inf_3dhp.py: PCK@150 / AUC per joint group and MPJPE tables
from integer counts and fp64 sums) against the numpy restatement of the MATLAB tool in mpi_eval_numpy.py (formulas and file:line
citations there), plus the argument checks of the two new entry points, which refuse before anything is enqueued."""
import ctypes

import numpy as np
import pytest

import mpi_eval_numpy as ref


def _host_tables(e, sequence, activity):
    from mvn.datasets import mpi_inf_3dhp as mpi
    out = {}
    for name, rows, n_rows in (("sequence", np.asarray(sequence) - 1, 6), ("activity", np.asarray(activity) - 1, 7)):
        c, f = ref.counts(e, rows, n_rows)
        s = np.stack([e[rows == r].sum(axis=0) for r in range(n_rows)])
        if name == "activity":                                   # + 'All' (mpii_evaluate_errors.m:51-54, 61-64)
            ca, fa = ref.counts(e, None, 1)
            c, f, s = np.concatenate([c, ca]), np.concatenate([f, fa]), np.concatenate([s, e.sum(axis=0)[None]])
        per, avg = mpi.mpjpe_table(s, f)
        pck, auc = mpi.pck_auc(c, f)
        out[name] = dict(mpjpe=per, mpjpe_average=avg, pck=pck, auc=auc, frames=f)
    return out


def _same_tables(got, want):
    for name in ("sequence", "activity"):
        np.testing.assert_array_equal(got[name]["frames"], want[name]["frames"])
        for k in ("mpjpe", "mpjpe_average", "pck", "auc"):
            np.testing.assert_allclose(got[name][k], want[name][k], rtol=1e-12, atol=1e-12, equal_nan=True, err_msg=f"{name} {k}")


def test_tables_match_the_matlab_restatement_on_a_synthetic_set():
    """6 sequences x 7 activities, 2929 poses (the test set's size), errors 0 .. ~250 mm in metres (to_mm = 1000)."""
    pred, gt, seq, act = ref.synthetic_set(2929, seed=5)
    e = ref.joint_errors(pred, gt, to_mm=1000.0)
    assert 0.0 < np.median(e) < 150.0 and e.max() > 150.0
    got = _host_tables(e, seq, act)
    want = ref.tables(e, seq, act)
    _same_tables(got, want)
    assert not np.isnan(got["activity"]["pck"]).any()
    assert got["activity"]["frames"][-1] == 2929 and got["sequence"]["frames"].sum() == 2929


def test_hand_cases_of_the_table_arithmetic():
    from mvn.datasets import mpi_inf_3dhp as mpi
    nf = 4
    # every grouped joint within 100 mm, the three ungrouped ones (0-based 14, 15, 16) far off: Total is over the 14 grouped joints
    e = np.full((nf, 17), 100.0)
    e[:, 14:] = 1000.0
    c, f = ref.counts(e, None, 1)
    pck, auc = mpi.pck_auc(c, f)
    assert np.all(pck[0] == 100.0)
    want_auc = 100 * (np.arange(0, 151, 5) > 100).sum() / 31
    np.testing.assert_allclose(auc[0], want_auc, rtol=1e-15)
    per, avg = mpi.mpjpe_table(e.sum(axis=0)[None], f)
    assert avg[0] == (14 * 100.0 + 3 * 1000.0) / 17                # the MPJPE average IS over all 17 joints
    # a single group off: only Elbow (1-based 4, 7) above 150 mm -> Elbow 0, Total = 12 / 14 of 100
    e = np.full((nf, 17), 10.0)
    e[:, [3, 6]] = 200.0
    c, f = ref.counts(e, None, 1)
    pck, auc = mpi.pck_auc(c, f)
    assert pck[0, 3] == 0.0 and auc[0, 3] == 0.0
    assert all(pck[0, g] == 100.0 for g in range(8) if g != 3)
    np.testing.assert_allclose(pck[0, 8], 100.0 * 12 / 14, rtol=1e-15)
    # half the frames of Head at 150 exactly (strict <: a miss), half at 0 (a hit from t = 5 on, a miss at t = 0)
    e = np.zeros((nf, 17))
    e[:2, 0] = 150.0
    c, f = ref.counts(e, None, 1)
    assert c[0, 0, 0] == 0 and c[0, 0, 1] == 2 and c[0, 0, 30] == 2 and c[0, 1, 30] == 4
    pck, auc = mpi.pck_auc(c, f)
    assert pck[0, 0] == 50.0
    np.testing.assert_allclose(auc[0, 0], 100 * (30 * 0.5) / 31, rtol=1e-15)
    # an empty row: NaN everywhere, as MATLAB's mean over nothing
    c, f = ref.counts(np.zeros((0, 17)), None, 1)
    pck, auc = mpi.pck_auc(c, f)
    per, avg = mpi.mpjpe_table(np.zeros((1, 17)), f)
    assert np.isnan(pck).all() and np.isnan(auc).all() and np.isnan(per).all() and np.isnan(avg).all()


def test_scene_table_weights_by_frames():
    from mvn.datasets import mpi_inf_3dhp as mpi
    t = dict(frames=np.array([603, 540, 505, 553, 276, 452]), mpjpe_average=np.arange(6, dtype=float),
             pck=np.arange(54, dtype=float).reshape(6, 9), auc=np.arange(54, dtype=float).reshape(6, 9))
    s = mpi.scene_table(t)
    np.testing.assert_allclose(s["GS"]["mpjpe_average"], (0 * 603 + 1 * 540) / (603 + 540))
    np.testing.assert_allclose(s["Outdoor"]["pck"], (t["pck"][4] * 276 + t["pck"][5] * 452) / (276 + 452))


def test_new_entries_refuse_bad_arguments_before_enqueueing():
    """capf_fliptest_fuse_swap: out-of-range, non-involutive or oversized tables; capf_pck_counts: bad joints / root / segments."""
    from capf.lib import MPI_SWAP, load_library
    lib = load_library()
    INVALID = -1
    fake = ctypes.c_void_p(16)                     # never dereferenced: every call below is refused on the host
    tab = lambda v: (ctypes.c_int32 * len(v))(*v)
    bad_tables = [list(range(16)) + [17], list(range(16)) + [-1], [1, 2, 0] + list(range(3, 17))]   # out of range x2, a 3-cycle
    for t in bad_tables:
        assert lib.capf_fliptest_fuse_swap(None, fake, 2, 17, tab(t), fake) == INVALID, t
    assert lib.capf_fliptest_fuse_swap(None, fake, 2, 33, tab(list(range(33))), fake) == INVALID
    assert lib.capf_fliptest_fuse_swap(None, fake, 0, 17, tab(list(MPI_SWAP)), fake) == INVALID
    assert all(MPI_SWAP[MPI_SWAP[j]] == j for j in range(17))
    assert sorted(MPI_SWAP) == list(range(17))
    for n, J, root, nseg, seg, to_mm in ((-1, 17, 14, 1, None, 1.0), (4, 0, 0, 1, None, 1.0), (4, 33, 14, 1, None, 1.0),
                                         (4, 17, 17, 1, None, 1.0), (4, 17, -1, 1, None, 1.0), (4, 17, 14, 0, None, 1.0),
                                         (4, 17, 14, 2, None, 1.0), (4, 17, 14, 1, None, 0.0)):
        assert lib.capf_pck_counts(None, fake, fake, n, J, root, to_mm, seg, nseg, fake, fake, fake) == INVALID
    assert lib.capf_pck_counts(None, None, None, 4, 17, 14, 1.0, None, 1, fake, fake, fake) == INVALID   # poses but no arrays
