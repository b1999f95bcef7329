"""GPU: the MPI-INF-3DHP evaluation counts (capf_pck_counts) and tables (mvn/datasets/mpi_inf_3dhp.py::evaluate) against the numpy
restatement of the MATLAB tool (mpi_eval_numpy.py), and the flip-test fusion with the 3DHP skeleton (capf_fliptest_fuse_swap) against
a torch restatement of ContextPose_mpi/run_3dhp.py:169-180."""
import numpy as np
import pytest
import torch

import mpi_eval_numpy as ref
from capf import lib as capf_lib

pytestmark = pytest.mark.gpu


def _dev(*xs):
    return [torch.as_tensor(x).cuda() for x in xs]


def test_counts_equal_numpy_exactly_and_tables_match_the_restatement():
    """2929 poses (the 3DHP test set's size) over 6 sequences x 7 activities, in metres (to_mm = 1000): every integer count equals
    numpy's, the fp64 sums agree to rounding, and evaluate()'s two tables equal the MATLAB restatement."""
    from mvn.datasets import mpi_inf_3dhp as mpi
    pred, gt, seq, act = ref.synthetic_set(2929, seed=11)
    e = ref.joint_errors(pred, gt, to_mm=1000.0)
    p, g = _dev(pred, gt)
    for rows, n_rows in ((seq - 1, 6), (act - 1, 7), (None, 1)):
        segment = torch.as_tensor(rows, dtype=torch.int32).cuda() if rows is not None else None
        counts, sums, frames = capf_lib.pck_counts(p, g, 14, 1000.0, segment, n_rows)
        want_c, want_f = ref.counts(e, rows, n_rows)
        np.testing.assert_array_equal(counts.cpu().numpy(), want_c)
        np.testing.assert_array_equal(frames.cpu().numpy(), want_f)
        rsel = np.zeros(len(e), np.int64) if rows is None else rows
        want_s = np.stack([e[rsel == r].sum(axis=0) for r in range(n_rows)])
        np.testing.assert_allclose(sums.cpu().numpy(), want_s, rtol=1e-12)
    got = mpi.evaluate(p, g, seq, act, to_mm=1000.0)
    want = ref.tables(e, seq, act)
    for name in ("sequence", "activity"):
        np.testing.assert_array_equal(got[name]["frames"], want[name]["frames"])
        for k in ("mpjpe", "mpjpe_average", "pck", "auc"):
            np.testing.assert_allclose(got[name][k], want[name][k], rtol=1e-12, equal_nan=True, err_msg=f"{name} {k}")
    assert got["activity"]["names"][-1] == "All" and got["sequence"]["names"][0] == "TS1"
    print(f"  All: MPJPE {got['activity']['mpjpe_average'][-1]:.2f} mm, PCK {got['activity']['pck'][-1, -1]:.2f}, "
          f"AUC {got['activity']['auc'][-1, -1]:.2f}")


def test_hand_cases():
    """Errors of exactly 150 mm and 0 mm (strict <), an empty activity (NaN), n = 0, and the same bits from two calls."""
    from mvn.datasets import mpi_inf_3dhp as mpi
    n = 4
    gt = np.zeros((n, 17, 3), np.float32)
    gt[:, :, 2] = 5000.0                                       # root-relative: all joints at the root
    pred = np.zeros((n, 17, 3), np.float32)
    pred[:, 0, 0] = 150.0                                      # Head exactly 150 mm off, everything else exact (0 mm)
    pred[:, 14, 0] = 77.0                                      # the root joint is taken as 0 whatever the model says
    p, g = _dev(pred, gt)
    counts, sums, frames = capf_lib.pck_counts(p, g, 14, 1.0, None, 1)
    c = counts.cpu().numpy()[0]
    assert c[0, 30] == 0 and c[0, :].sum() == 0                # 150 < 150 is false, and so is every smaller threshold
    assert c[1, 0] == 0 and (c[1, 1:] == n).all()              # 0 < 0 is false, 0 < 5 true
    assert (c[14, 1:] == n).all()
    assert sums.cpu().numpy()[0, 0] == 150.0 * n and frames.item() == n
    t = mpi.evaluate(p, g, [1, 1, 2, 2], [1, 1, 1, 3], to_mm=1.0)
    assert t["activity"]["pck"][0, 0] == 0.0 and t["activity"]["pck"][0, 1] == 100.0
    np.testing.assert_allclose(t["activity"]["pck"][0, -1], 100.0 * 13 / 14)
    empty = [1, 3, 4, 5, 6]                                    # 0-based rows of activities 2, 4, 5, 6, 7
    assert np.isnan(t["activity"]["pck"][empty]).all() and np.isnan(t["activity"]["mpjpe_average"][empty]).all()
    assert np.isnan(t["sequence"]["auc"][2:]).all() and not np.isnan(t["sequence"]["auc"][:2]).any()
    # n = 0: zero counts, zero frames, NaN tables
    z = torch.zeros(0, 17, 3, device="cuda")
    counts, sums, frames = capf_lib.pck_counts(z, z, 14, 1.0, None, 1)
    assert counts.abs().sum().item() == 0 and sums.abs().sum().item() == 0 and frames.item() == 0
    t0 = mpi.evaluate(z, z, np.zeros(0, int), np.zeros(0, int))
    assert np.isnan(t0["activity"]["pck"]).all() and (t0["activity"]["frames"] == 0).all()
    # determinism: two calls, same bits
    pred, gt, seq, act = ref.synthetic_set(2929, seed=12)
    p, g = _dev(pred, gt)
    s = torch.as_tensor(act - 1, dtype=torch.int32).cuda()
    a = capf_lib.pck_counts(p, g, 14, 1000.0, s, 7)
    b = capf_lib.pck_counts(p, g, 14, 1000.0, s, 7)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def _torch_input_augmentation_fuse(pred2):
    """run_3dhp.py:169-180 on the two predictions [2, B, 3, 1, 17, 1] (the model's layout): un-mirror the second, average."""
    joints_left, joints_right = [5, 6, 7, 11, 12, 13], [2, 3, 4, 8, 9, 10]
    flip = pred2[1].clone()
    flip[:, 0] *= -1
    flip[:, :, :, joints_left + joints_right] = flip[:, :, :, joints_right + joints_left]
    return (pred2[0] + flip) / 2


def test_fliptest_fuse_with_the_3dhp_table_equals_input_augmentation_bit_for_bit():
    B = 37
    g = torch.Generator().manual_seed(4)
    pred2 = (torch.randn(2, B, 1, 17, 3, generator=g) * 0.3).cuda()
    got = capf_lib.fliptest_fuse(pred2, swap=capf_lib.MPI_SWAP)                       # [B, 1, 17, 3]
    as_model = pred2.view(2, B, 1, 17, 3, 1).permute(0, 1, 4, 2, 3, 5)               # [2, B, 3, 1, 17, 1]
    want = _torch_input_augmentation_fuse(as_model).permute(0, 2, 3, 4, 1).reshape(B, 1, 17, 3)
    assert torch.equal(got, want)
    # the H36M table through the new entry == capf_fliptest_fuse
    h36m = (0, 4, 5, 6, 1, 2, 3, 7, 8, 9, 10, 14, 15, 16, 11, 12, 13)
    assert torch.equal(capf_lib.fliptest_fuse(pred2, swap=h36m), capf_lib.fliptest_fuse(pred2))
    # a non-involutive table is refused
    with pytest.raises(capf_lib.CapfError):
        capf_lib.fliptest_fuse(pred2, swap=(1, 2, 0) + tuple(range(3, 17)))


def test_variant_forward_flip_test():
    """VolumetricTriangulationNet.forward_flip_test: one forward of the 2B stacked views, fused with the 3DHP table; equals the torch
    restatement applied to that forward's own two halves, and has forward's output form."""
    import contextlib, copy, io
    from capf import synth
    from model.conpose import VolumetricTriangulationNet, mpi_preset
    from mvn.utils.cfg import config
    cfg = mpi_preset(copy.deepcopy(config), "hrnet_32")
    with contextlib.redirect_stdout(io.StringIO()):
        m = VolumetricTriangulationNet(cfg).eval()
    synth.load_synthetic(m, seed=21, bn_mode="random")
    m = m.cuda()
    B = 3
    img, k2d, kc = synth.synth_inputs(2 * B, 256, 192, seed=22)
    img2, k2d2, kc2 = img.view(2, B, 256, 192, 3).cuda(), k2d.view(2, B, 17, 2).cuda(), kc.view(2, B, 17, 2).cuda()
    with torch.no_grad():
        out, aux = m.forward_flip_test(img2.contiguous(), k2d2.contiguous(), kc2.clone().contiguous())
        both, _ = m(img2.reshape(2 * B, 256, 192, 3), k2d2.reshape(2 * B, 17, 2), kc2.clone().reshape(2 * B, 17, 2))
    assert aux is None and tuple(out.shape) == (B, 3, 1, 17, 1)
    assert torch.equal(out, _torch_input_augmentation_fuse(both.view(2, B, 3, 1, 17, 1)))
