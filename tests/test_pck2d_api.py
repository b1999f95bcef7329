"""CPU: the 2-D PCKh path without a device -- the float64 restatement of capf_pck2d_counts (pck2d_oracle.py) and the host tables of
mvn/datasets/human36m.py (pck2d_tables, Pck2dAccumulator), both held exactly to what the reference's own evaluate2d / evaluate_2d_joint
computed (tests/golden/pck2d_reference.json, written by tools/make_pck2d_golden.py); every refusal of the entry on a plan-free call; the
export; the NaN rule; the accumulator against one-shot counts; and the return_accuracy keyword of keypoint_loss."""
import ctypes
import inspect
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import pck2d_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = json.load(open(os.path.join(ROOT, "tests", "golden", "pck2d_reference.json")))


def _case_arrays(case):
    gt = np.asarray(case["gt"], np.float64).reshape(case["shape"])
    pred = np.asarray(case["pred"], np.float64).reshape(case["shape"])
    assert np.array_equal(gt, gt.astype(np.float32)) and np.array_equal(pred, pred.astype(np.float32))     # fp32-representable
    J = case["shape"][-2]
    return gt.reshape(-1, J, 2).astype(np.float32), pred.reshape(-1, J, 2).astype(np.float32), J


@pytest.mark.parametrize("case", GOLDEN["cases"], ids=[c["name"] for c in GOLDEN["cases"]])
def test_restatement_and_host_tables_equal_the_reference_exactly(case):
    from mvn.datasets.human36m import pck2d_tables
    gt, pred, J = _case_arrays(case)
    n, thresholds, headsize = gt.shape[0], case["thresholds"], case["headsize"]
    scaled = [headsize * t for t in thresholds]                        # the product the reference forms (human36m.py:440)
    groups, parts = ["all"], [O.pck2d_counts(pred, gt, scaled)[:3]]
    if case["split"] is not None:                                      # the reference slices rows; here: a subject index per pose
        seg = (np.arange(n) >= case["split"]).astype(np.int32)
        groups += ["first", "second"]
        parts.append(O.pck2d_counts(pred, gt, scaled, segment=seg, n_segments=2)[:3])
    counts, valid, sums = (np.concatenate(x) for x in zip(*parts))
    nv, mr, me = pck2d_tables(counts, valid, sums, thresholds, groups, case["joint_names"])
    assert list(nv) == thresholds and list(mr) == thresholds
    for k, t in enumerate(thresholds):
        assert list(nv[t]) == groups and list(mr[t]) == groups
        for g in groups:
            want = case["groups"][g]
            assert list(nv[t][g]) == case["joint_names"]
            assert [float(v) for v in nv[t][g].values()] == want["rates"][k], (t, g)          # exact, not close
            assert float(mr[t][g]) == want["mean"][k], (t, g)
    # the fixture holds ties: a threshold hit exactly is a detection under `<=` and none under `<`
    strict = O.pck2d_counts(pred, gt, scaled, strict=True)[0]
    if case["name"].startswith("ties"):
        e = O.pck2d_counts(pred, gt, scaled)[3]
        assert (e == scaled[0]).sum() > 0 and (strict[0, 0] < counts[0, 0]).any()
        assert np.array_equal(counts[0, 0] - strict[0, 0], (e == scaled[0]).sum(axis=0))
    assert set(me) == set(groups) and all(np.isfinite(list(me[g].values())).all() for g in groups)


def test_restatement_hand_cases():
    gt = np.zeros((4, 2, 2), np.float32)
    pred = np.array([[[3, 4], [6, 16]], [[3, 4], [0, 0]], [[np.nan, 0], [1, 0]], [[np.inf, 0], [0, 1]]], np.float32)
    c, v, s, e, _ = O.pck2d_counts(pred, gt, [5.0, 4.0])
    assert e[0, 0] == 5.0 and np.isnan(e[2, 0]) and np.isinf(e[3, 0])
    assert c[0].tolist() == [[2, 3], [0, 3]] and v.tolist() == [[4, 4]]
    assert np.isnan(s[0, 0]) and s[0, 1] == float(np.sqrt(np.float64(36 + 256))) + 1 + 1
    c, v, s, e, _ = O.pck2d_counts(pred[:2], gt[:2], [5.0], strict=True)
    assert c[0, 0].tolist() == [0, 1]
    # norm = (2, 4), offsets (6, 16): u = 3, v = 4 exactly; an invalid norm skips the pose for every joint
    norm = np.array([[2, 4], [0, 1], [1, -1], [np.inf, 1]], np.float32)
    c, v, s, e, _ = O.pck2d_counts(pred, gt, [5.0], norm=norm)
    assert e[0, 1] == 5.0 and v.tolist() == [[1, 1]] and c[0, 0].tolist() == [1, 1]          # (joint 0: u = 1.5, v = 1)
    assert O.pck2d_counts(pred, gt, [5.0], norm=norm, strict=True)[0][0, 0].tolist() == [1, 0]
    # weights, segments with ids outside [0, S), an empty segment
    w = np.array([[1, 0], [0.5, 0], [0, 0], [-1, 0]], np.float32)
    c, v, s, e, _ = O.pck2d_counts(pred, gt, [5.0], weight=w, segment=np.array([0, 3, -1, 2], np.int32), n_segments=3)
    assert v.tolist() == [[1, 0], [0, 0], [0, 0]] and s[0, 1] == 0.0 and c[:, 0].tolist() == [[1, 0], [0, 0], [0, 0]]
    # the ordered sum is the lanes-then-tree order, not left to right: 257 values where the difference shows
    vals = np.full(257, 0.1)
    vals[0], vals[256] = 1e16, 1.0
    lanes = vals[:256].copy()
    lanes[0] = vals[0] + vals[256]
    o = 128
    while o:
        lanes[:o] = lanes[:o] + lanes[o:2 * o]
        o //= 2
    assert O.ordered_sum(vals, np.ones(257, bool)) == lanes[0]
    assert O.accuracy(np.array([[[1, 0, 3]]]), np.array([[2, 0, 4]])) == (0.5 + 0.75) / 2 and np.isnan(O.accuracy(np.zeros((1, 1, 2)), np.zeros((1, 2))))


def _call(lib, **kw):
    fake = ctypes.c_void_p(16)                     # never dereferenced: every call below is refused on the host
    a = dict(pred=fake, gt=fake, n=4, joints=17, norm=None, weight=None, thresholds=[0.5], n_thresholds=None, strict=0, segment=None,
             n_segments=1, counts=fake, valid=fake, err_sums=fake)
    a.update(kw)
    thr = a["thresholds"]
    K = len(thr) if a["n_thresholds"] is None else a["n_thresholds"]
    arr = None if thr is None else (ctypes.c_double * max(len(thr), 1))(*thr)
    return lib.capf_pck2d_counts(None, a["pred"], a["gt"], a["n"], a["joints"], a["norm"], a["weight"], arr, K, a["strict"], a["segment"],
                                 a["n_segments"], a["counts"], a["valid"], a["err_sums"])


def test_every_refusal_comes_before_any_launch_and_needs_no_device():
    from capf.lib import load_library
    lib = load_library()
    INVALID, UNSUPPORTED = -1, -2
    fake = ctypes.c_void_p(16)
    invalid = [dict(counts=None), dict(valid=None), dict(err_sums=None), dict(thresholds=None, n_thresholds=1), dict(thresholds=[], n_thresholds=0),
               dict(thresholds=[0.5] * 33), dict(thresholds=[0.5], n_thresholds=-1), dict(thresholds=[0.5, float("nan")]),
               dict(thresholds=[float("nan")]), dict(joints=0), dict(joints=-3), dict(n=-1), dict(n_segments=0), dict(n_segments=-2),
               dict(strict=2), dict(strict=-1), dict(segment=None, n_segments=2), dict(segment=None, n_segments=3, n=1),
               dict(pred=None), dict(gt=None)]
    for kw in invalid:
        assert _call(lib, **kw) == INVALID, kw
    assert _call(lib, joints=33) == UNSUPPORTED
    assert _call(lib, joints=33, segment=fake, n_segments=4, thresholds=[0.1] * 32, strict=1) == UNSUPPORTED
    assert _call(lib, joints=0, n_segments=0) == INVALID           # (joints <= 0 is INVALID, only joints > 32 UNSUPPORTED)
    assert _call(lib, joints=33, thresholds=[float("nan")]) == INVALID


def test_symbol_is_exported_and_declared():
    from capf import lib as capf_lib
    assert "capf_pck2d_counts" in capf_lib.EXPORTS and capf_lib.load_library().capf_abi_version() == 12
    out = subprocess.run(["nm", "-D", "--defined-only", capf_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(line.split()[-1] == "capf_pck2d_counts" for line in out.splitlines())
    assert "int capf_pck2d_counts(void* stream, const float* pred, const float* gt, int n, int joints, const float* norm" in \
        open(os.path.join(ROOT, "include", "capf.h")).read()


def test_table_structure_keys_and_the_nan_rule():
    from mvn.datasets.human36m import pck2d_tables
    counts = np.array([[[2, 0, 1], [4, 0, 3]], [[0, 0, 1], [0, 0, 1]]], np.int32)          # [G=2, K=2, J=3]
    valid = np.array([[4, 0, 4], [0, 0, 1]], np.int32)
    sums = np.array([[2.0, 0.0, 6.0], [0.0, 0.0, 0.5]])
    nv, mr, me = pck2d_tables(counts, valid, sums, [0.5, 1.0], ["all", "s9"], ["a", "b", "c"])
    assert list(nv) == [0.5, 1.0] and list(nv[0.5]) == ["all", "s9"] and list(nv[0.5]["all"]) == ["a", "b", "c"]
    assert nv[0.5]["all"]["a"] == 0.5 and np.isnan(nv[0.5]["all"]["b"]) and nv[0.5]["all"]["c"] == 0.25
    assert mr[0.5]["all"] == (0.5 + 0.25) / 2 and mr[1.0]["all"] == (1.0 + 0.75) / 2          # the joint without a sample is left out
    assert np.isnan(nv[1.0]["s9"]["a"]) and nv[1.0]["s9"]["c"] == 1.0 and mr[1.0]["s9"] == 1.0
    assert me["all"]["a"] == 0.5 and np.isnan(me["all"]["b"]) and me["all"]["c"] == 1.5 and me["s9"]["c"] == 0.5
    nv, mr, me = pck2d_tables(np.zeros((1, 1, 2), np.int32), np.zeros((1, 2), np.int32), np.zeros((1, 2)), [0.5])
    assert list(nv[0.5]["all"]) == ["joint_0", "joint_1"] and np.isnan(mr[0.5]["all"]) and np.isnan(me["all"]["joint_1"])
    with pytest.raises(ValueError):
        pck2d_tables(counts, valid, sums, [0.5], ["all", "s9"], ["a", "b", "c"])


def test_accumulator_equals_one_shot_counts_on_the_concatenated_input():
    from mvn.datasets.human36m import Pck2dAccumulator, pck2d_tables
    rng = np.random.RandomState(3)
    n, J, S = 700, 5, 3
    gt = rng.uniform(0, 64, (n, J, 2)).astype(np.float32)
    pred = (gt + rng.normal(0, 4, gt.shape)).astype(np.float32)
    w = (rng.uniform(size=(n, J)) > 0.2).astype(np.float32)
    w[:, 3] = 0                                                             # a joint nobody labelled
    seg = rng.randint(-1, S + 1, n).astype(np.int32)                        # ids -1 and S: counted in 'all' only
    thresholds, headsize = [0.25, 0.5, 1.0], 6.4
    acc = Pck2dAccumulator(thresholds, headsize, ["s1", "s9", "s11"], list("abcde"))

    def both(sl):
        a = O.pck2d_counts(pred[sl], gt[sl], acc.scaled, weight=w[sl])[:3]
        b = O.pck2d_counts(pred[sl], gt[sl], acc.scaled, weight=w[sl], segment=seg[sl], n_segments=S)[:3]
        return [np.concatenate(x) for x in zip(a, b)]

    for lo, hi in ((0, 256), (256, 257), (257, 700)):
        acc.add(*(torch.from_numpy(x) for x in both(slice(lo, hi))))
    one = both(slice(None))
    assert np.array_equal(acc.counts.numpy(), one[0]) and np.array_equal(acc.valid.numpy(), one[1])          # integers: equal
    np.testing.assert_allclose(acc.err_sums.numpy(), one[2], rtol=1e-13)
    nv, mr, me = acc.tables()
    nv1, mr1, _ = pck2d_tables(one[0], one[1], one[2], thresholds, ["all", "s1", "s9", "s11"], list("abcde"))
    for t in thresholds:
        for g in ("all", "s1", "s9", "s11"):
            np.testing.assert_array_equal(list(nv[t][g].values()), list(nv1[t][g].values()))
            assert mr[t][g] == mr1[t][g] and np.isnan(nv[t][g]["d"])
    assert acc.scaled == [headsize * t for t in thresholds]
    with pytest.raises(ValueError):
        Pck2dAccumulator([0.5], 1.0).tables()


def test_accumulator_owns_its_totals_and_leaves_a_reused_buffer_alone():
    """add() twice with ONE reused (counts, valid, err_sums) buffer, as capf.lib.pck2d_counts(out=...) invites: the totals are the one-shot
    sums and the caller's tensors hold what the caller last wrote -- for int32 / float64 inputs and for inputs already int64 / float64,
    which a plain .to() would alias"""
    from mvn.datasets.human36m import Pck2dAccumulator
    rng = np.random.RandomState(8)
    gt = rng.uniform(0, 64, (300, 4, 2)).astype(np.float32)
    pred = (gt + rng.normal(0, 4, gt.shape)).astype(np.float32)
    first, second = (O.pck2d_counts(pred[sl], gt[sl], [2.0, 4.0])[:3] for sl in (slice(0, 130), slice(130, 300)))
    whole = O.pck2d_counts(pred, gt, [2.0, 4.0])[:3]
    for int_dtype in (torch.int32, torch.int64):
        acc = Pck2dAccumulator([0.5, 1.0], 4.0)
        buf = (torch.zeros(1, 2, 4, dtype=int_dtype), torch.zeros(1, 4, dtype=int_dtype), torch.zeros(1, 4, dtype=torch.float64))
        for batch in (first, second):
            for b, a in zip(buf, batch):
                b.copy_(torch.from_numpy(a))                                  # the next batch overwrites the same buffer
            acc.add(*buf)
            assert all(np.array_equal(b.numpy(), a) for b, a in zip(buf, batch))          # add() only read it
            assert all(t.data_ptr() != b.data_ptr() for t, b in zip((acc.counts, acc.valid, acc.err_sums), buf))
        assert np.array_equal(acc.counts.numpy(), whole[0]) and np.array_equal(acc.valid.numpy(), whole[1])
        assert np.array_equal(acc.err_sums.numpy(), first[2] + second[2])
        np.testing.assert_allclose(acc.err_sums.numpy(), whole[2], rtol=1e-13)
        me = acc.tables()[2]
        np.testing.assert_allclose(list(me["all"].values()), whole[2][0] / whole[1][0], rtol=1e-13)


def test_accuracy_norm_is_width_then_height_over_ten():
    """keypoint_loss's norm for capf_pck2d_counts on a crop that is not square: x is normalised by W / 10, y by H / 10, as fp32"""
    from mvn.models.conpose import CA_PF
    norm = CA_PF._accuracy_norm(3, 256, 192, "cpu")
    assert norm.dtype == torch.float32 and tuple(norm.shape) == (3, 2)
    assert np.array_equal(norm.numpy(), np.tile(np.array([19.2, 25.6], np.float32), (3, 1)))


def test_keypoint_loss_takes_return_accuracy_and_defaults_to_the_loss_alone():
    from model.conpose import VolumetricTriangulationNet
    from mvn.models.conpose import CA_PF
    for cls in (CA_PF, VolumetricTriangulationNet):
        p = inspect.signature(cls.keypoint_loss).parameters
        assert list(p)[-1] == "return_accuracy" and p["return_accuracy"].default is False
