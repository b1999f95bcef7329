"""GPU: the small kernels every reported figure and every training loss goes through, held to float64 at their edges.

    pose_errors / segment_sums / evaluate_using_pred    csrc/metrics.hip        (MPJPE, P-MPJPE, N-MPJPE, velocity error; per-action sums)
    capf_mpjpe / capf_mpjpe_nd / MPJPE()                 csrc/train_kernels.hip  (the training loss and its gradient)
    capf_keypoints_loss                                  csrc/metrics.hip        (the three validity-masked keypoint losses)
    capf_preprocess / fliptest_fuse                      csrc/preprocess.hip     (bit for bit against the torch expressions)

Bounds.  Per-pose errors: |got - want| <= 2^-23 |want| + 1e-12 s per pose and column (tests/metric_edge_cases.py; the 1e-12 s term rests on
tests/test_metrics.py's CPU restatement of the kernel's Jacobi solver, which stays within 1.3e-14 s of the SVD form on the same poses).
Losses and gradients: 4 x d32 + 1e-6 of the quantity's largest magnitude, d32 the distance of the same expression in torch float32 ON THE
CPU from float64 (the style of tests/test_gpu_bn_train.py).  Where they write and what they read: tests/test_gpu_op_guards.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import metric_edge_cases as mc
import metrics_oracle as mo
from capf import lib as capf

pytestmark = pytest.mark.gpu

CAPF_ERR_INVALID, CAPF_ERR_UNSUPPORTED = -1, -2          # include/capf.h


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


# ---- 1. pose_errors ------------------------------------------------------------------------------------------------------------------------------
POSE_N = (1, 2, 127, 128, 129, 1000)          # the block is 128 threads


@functools.lru_cache(maxsize=None)
def _pose_case(fam, n, J):
    """(pred, gt, want [n,4], bound [n,4]) with prev = i - 1; the condition on the inputs asserted for every pose"""
    pred, gt = mc.pose_family(fam, n, J)
    mc.assert_condition(pred, gt, f"{fam} n={n} J={J}")
    return (pred, gt) + mc.yardstick(pred, gt)


@pytest.mark.parametrize("with_prev", [False, True], ids=["prev=None", "prev=table"])
@pytest.mark.parametrize("J", [3, 4, 16, 17, 32])
def test_pose_errors_every_column_against_float64(J, with_prev):
    """n around the block size, J over the ABI's range, eight pose families (the reflection branch, unrelated poses, any rotation and scale,
    exact and identical poses, planar poses, millimetre units): every column of every pose within one float32 store of float64."""
    from mvn.datasets.human36m import previous_in_segment
    worst = {}
    for n in POSE_N:
        prev = previous_in_segment(mc.permuted_segments(n, 5, 1)) if with_prev else None
        for fam in mc.FAMILIES:
            pred, gt, want, bound = _pose_case(fam, n, J)
            if with_prev:
                want = want.copy()
                want[:, 3] = mo.velocity_errors(pred, gt, prev)
                bound = mc.bound(want, gt)
            got = capf.pose_errors(_dev(pred), _dev(gt), _dev(prev) if with_prev else None).cpu().numpy().astype(np.float64)
            assert got.shape == (n, 4) and np.isfinite(got).all(), (fam, n, J)
            ratio = np.abs(got - want) / bound
            for c, col in enumerate(mc.COLUMNS):
                worst[fam, col] = max(worst.get((fam, col), 0.0), float(ratio[:, c].max()))
    for fam in mc.FAMILIES:
        print(f"  J {J} {'prev table' if with_prev else 'prev None'} {fam}: worst error / bound " +
              ", ".join(f"{col} {worst[fam, col]:.3f}" for col in mc.COLUMNS))
    bad = {k: v for k, v in worst.items() if not v <= 1.0}
    assert not bad, bad


def test_pose_errors_degenerate_rows_are_nan_in_their_own_column_only():
    """A prediction whose joints are all one point has no Procrustes alignment (normY = 0, loss.py:43, 46) and an all-zero prediction no
    N-MPJPE scale (0 / 0, loss.py:84): the reference's numpy SVD raises on the first, so there is no parity to pin -- capf_pose_errors
    returns NaN in that column of that row, finite and correct values in its other columns, and every other row as if the row were not there."""
    n, J = 129, 17
    pred, gt = (a.copy() for a in mc.pose_family("near", n, J))
    pred[5] = pred[5, :1]
    pred[77] = 0.0
    keep = np.ones(n, bool)
    keep[[5, 77]] = False
    mc.assert_condition(pred[keep], gt[keep], "degenerate batch")
    got = capf.pose_errors(_dev(pred), _dev(gt)).cpu().numpy().astype(np.float64)
    want, bound = mc.yardstick(pred[keep], gt[keep])
    prev = np.arange(n) - 1
    vel = mo.velocity_errors(pred, gt, prev)
    assert np.isnan(got[5, 1]) and np.isnan(got[77, 2])
    assert np.isnan(got[77, 1])                                   # (an all-zero prediction is a single point as well)
    for row in (5, 77):
        assert abs(got[row, 0] - mo.mpjpe_per_pose(pred[row:row + 1], gt[row:row + 1])[0]) <= 2.0 ** -23 * got[row, 0] + 1e-12
        assert abs(got[row, 3] - vel[row]) <= 2.0 ** -23 * vel[row] + 1e-12
    assert abs(got[5, 2] - mo.n_mpjpe_per_pose(pred[5:6], gt[5:6])[0]) <= 2.0 ** -23 * got[5, 2] + 1e-12
    assert (np.abs(got[keep][:, :3] - want[:, :3]) <= bound[:, :3]).all()
    assert (np.abs(got[:, 3] - vel) <= 2.0 ** -23 * vel + 1e-12 * 4).all()          # (the neighbours of a planted row pair with it)


def test_pose_errors_refuses_what_it_does_not_cover_and_launches_nothing():
    lib = capf.load_library()
    x = torch.randn(4, 33, 3, device="cuda")
    err = torch.full((4, 4), 7.0, device="cuda")
    for n, J, want in ((4, 33, CAPF_ERR_UNSUPPORTED), (4, 0, CAPF_ERR_INVALID), (0, 17, CAPF_ERR_INVALID), (0, 33, CAPF_ERR_INVALID)):
        assert lib.capf_pose_errors(_stream(), _ptr(x), _ptr(x), n, J, _ptr(None), _ptr(err)) == want, (n, J)
    torch.cuda.synchronize()
    assert bool((err == 7.0).all())
    with pytest.raises(capf.CapfError):
        capf.pose_errors(x, x)


# ---- 2. segment_sums, evaluate_using_pred ------------------------------------------------------------------------------------------------------------
def _segments(n, S, seed=2):
    """interleaved runs; with S > 1 the last id stays empty, with S > 2 the one before it holds a single pose; from 16 poses up three ids
    outside [0, S)"""
    rng = np.random.default_rng([seed, n, S])
    pool = list(range(max(1, S - 2))) if S > 2 else [0]
    seg = np.empty(n, np.int32)
    i = 0
    while i < n:
        run = int(rng.integers(1, 10))
        seg[i:i + run] = pool[int(rng.integers(len(pool)))]
        i += run
    if S > 2 and n > 1:
        seg[n // 2] = S - 2
    if n >= 16:
        seg[[3, n // 3, n - 2]] = [-1, S, S + 5]
    return seg


@pytest.mark.parametrize("S", [1, 6, 7])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_segment_sums_counts_exact_sums_fp64_and_same_bits_twice(n, S):
    from mvn.datasets.human36m import previous_in_segment
    pred, gt = mc.pose_family("near", n, 17)
    seg = _segments(n, S)
    prev = previous_in_segment(seg)
    p, g, d_seg, d_prev = _dev(pred), _dev(gt), _dev(seg), _dev(prev)
    err = capf.pose_errors(p, g, d_prev)
    sums, counts = capf.segment_sums(err, d_seg, d_prev, n_segments=S)
    sums2, counts2 = capf.segment_sums(err, d_seg, d_prev, n_segments=S)
    assert torch.equal(sums.view(torch.int64), sums2.view(torch.int64)) and torch.equal(counts, counts2)
    e, sums, counts = err.cpu().numpy().astype(np.float64), sums.cpu().numpy(), counts.cpu().numpy()
    inside = 0
    for s in range(S):
        m = seg == s
        mp = m & (prev >= 0)
        inside += int(m.sum())
        assert counts[s].tolist() == [int(m.sum()), int(mp.sum())], (s, counts[s])
        np.testing.assert_allclose(sums[s, :3], e[m][:, :3].sum(0), rtol=1e-12, atol=0)
        np.testing.assert_allclose(sums[s, 3], e[mp][:, 3].sum(), rtol=1e-12, atol=0)
    assert counts[:, 0].sum() == inside == int(((seg >= 0) & (seg < S)).sum())          # ids outside the table are counted nowhere
    if S > 1:
        assert not (seg == S - 1).any() and counts[S - 1].tolist() == [0, 0] and (sums[S - 1] == 0).all()        # the empty segment
    if S > 2 and n > 1:
        assert counts[S - 2].tolist() == [1, 0] and sums[S - 2, 3] == 0                  # one pose: no predecessor, no pair
    # no segment table, no predecessor table: everything is segment 0 and row i pairs with row i - 1
    err1 = capf.pose_errors(p, g)
    s1, c1 = capf.segment_sums(err1)
    e1 = err1.cpu().numpy().astype(np.float64)
    assert c1.cpu().tolist() == [[n, n - 1]]
    np.testing.assert_allclose(s1.cpu().numpy()[0, :3], e1[:, :3].sum(0), rtol=1e-12, atol=0)
    np.testing.assert_allclose(s1.cpu().numpy()[0, 3], e1[1:, 3].sum(), rtol=1e-12, atol=0)


def test_evaluate_using_pred_against_float64_with_unequal_empty_and_one_frame_trials():
    """Eight action trials of unequal length in a shuffled order against mo.per_action_scores (human36m.py:370-416 in float64).  Eating-1 has
    no frame: the mean of nothing is NaN and goes into the merged action, as the reference's `0 * mean([])` does.  Posing-1 has ONE frame:
    MPJPE and P-MPJPE are finite, MPJVE is NaN (no pair of rows) -- the reference itself raises there, because `.squeeze()` (:374, :376) drops
    the frame axis too; this pins the choice mvn/datasets/human36m.py documents, not parity.
    Tolerance: every per-pose figure is one float32 store of its float64 value (2^-23 relative, test above), non-negative, and summed in fp64."""
    from mvn.datasets.human36m import evaluate_using_pred
    names = ["Walking-1", "Walking-2", "Eating-1", "Eating-2", "Posing-1", "Posing-2", "Sitting-1", "Sitting-2"]
    lengths = [40, 25, 0, 31, 1, 17, 9, 52]
    idx = np.repeat(np.arange(8), lengths)
    np.random.default_rng(6).shuffle(idx)
    pred, gt = mc.pose_family("near", len(idx), 17, seed=3)
    want = mo.per_action_scores(pred, gt, idx, names)
    got = evaluate_using_pred(_dev(gt[:, None]), _dev(pred[:, None]), idx, names)
    assert sorted(got) == sorted(want) == ["Eating", "Posing", "Sitting", "Walking"]
    for base in want:
        for k in ("MPJPE", "P_MPJPE", "MPJVE"):
            if np.isnan(want[base][k]):
                assert np.isnan(got[base][k]), (base, k, got[base][k])
            else:
                np.testing.assert_allclose(got[base][k], want[base][k], rtol=2.0 ** -23 + 1e-9, atol=0, err_msg=f"{base} {k}")
    assert all(np.isnan(v) for v in want["Eating"].values())
    assert np.isfinite(want["Posing"]["MPJPE"]) and np.isfinite(want["Posing"]["P_MPJPE"]) and np.isnan(want["Posing"]["MPJVE"])
    assert all(np.isfinite(v) for v in want["Walking"].values()) and all(np.isfinite(v) for v in want["Sitting"].values())


# ---- 3. capf_mpjpe, capf_mpjpe_nd, MPJPE() -----------------------------------------------------------------------------------------------------------
def _mpjpe_reference(pred, gt, dtype, scale=1.0):
    """loss.py:22 in torch on the CPU with autograd -> (loss, scale * dloss/dpred) as float64 tensors"""
    p = pred.detach().to(dtype, copy=True).requires_grad_(True)
    loss = torch.mean(torch.norm(p - gt.to(dtype), dim=p.dim() - 1))
    (loss * scale).backward()
    return loss.detach().double(), p.grad.double()


def _within(tag, got, w64, w32, ratios):
    """4 x d32 + 1e-6 of the largest magnitude; collects error / bound"""
    err = (got.double().cpu() - w64).abs().max().item()
    d32 = (w32 - w64).abs().max().item()
    bound = 4.0 * d32 + 1e-6 * w64.abs().max().item()
    ratios.append(err / bound if bound > 0 else (0.0 if err == 0 else float("inf")))
    assert err <= bound, (tag, err, d32, bound)


@pytest.mark.parametrize("rows", [1, 2, 1023, 1024, 1025, 8705])
def test_mpjpe_entries_loss_and_gradient_against_float64(rows):
    """rows around the block of 1024 and over eight trips of its loop; D in {1, 2, 3, 4, 7} through capf_mpjpe_nd and D = 3 through capf_mpjpe too;
    grad_scale 1, 1/8 and 3; rows with pred == gt (a zero gradient row, a finite loss); the loss bits do not depend on dpred being asked for."""
    lib = capf.load_library()
    g = torch.Generator().manual_seed(rows)
    ratios = []
    for D, entry in [(D, "nd") for D in (1, 2, 3, 4, 7)] + [(3, "3")]:
        pred, gt = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)
        same = sorted({0, rows // 2})
        pred[same] = gt[same]
        dp, dg = pred.cuda(), gt.cuda()
        for scale in (1.0, 0.125, 3.0):
            l64, g64 = _mpjpe_reference(pred, gt, torch.float64, scale)
            l32, g32 = _mpjpe_reference(pred, gt, torch.float32, scale)
            loss, loss0 = torch.full((1,), float("nan"), device="cuda"), torch.full((1,), float("nan"), device="cuda")
            dpred = torch.full((rows, D), float("nan"), device="cuda")
            for out, grad in ((loss, dpred), (loss0, None)):
                if entry == "3":
                    rc = lib.capf_mpjpe(_stream(), _ptr(dp), _ptr(dg), rows, _ptr(out), _ptr(grad), scale)
                else:
                    rc = lib.capf_mpjpe_nd(_stream(), _ptr(dp), _ptr(dg), rows, D, _ptr(out), _ptr(grad), scale)
                assert rc == 0, (rc, rows, D, entry)
            tag = f"rows {rows} D {D} entry {entry} grad_scale {scale}"
            assert torch.equal(loss.view(torch.int32), loss0.view(torch.int32)), tag
            assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(dpred).all()), tag
            assert bool((dpred[same] == 0).all()), tag
            _within(tag + " loss", loss[0], l64, l32, ratios)
            _within(tag + " dpred", dpred, g64, g32, ratios)
    print(f"  rows {rows}: worst error / bound {max(ratios):.3f}")


def test_mpjpe_module_views_widths_dtypes_and_the_target_gradient():
    from mvn.models.loss import MPJPE
    g = torch.Generator().manual_seed(21)
    ratios = []
    # a non-contiguous [B,1,17,3] view of a leaf; the target requires grad as well and receives -dloss/dpred (torch.norm(pred - gt), loss.py:22)
    base, gt = torch.randn(9, 1, 17, 6, generator=g), torch.randn(9, 1, 17, 3, generator=g)
    refs = []
    for dtype in (torch.float64, torch.float32):
        b, t = base.to(dtype, copy=True).requires_grad_(True), gt.to(dtype, copy=True).requires_grad_(True)
        loss = torch.mean(torch.norm(b[..., ::2] - t, dim=3))
        loss.backward()
        refs.append((loss.detach().double(), b.grad.double(), t.grad.double()))
    b, t = base.cuda().requires_grad_(True), gt.cuda().requires_grad_(True)
    view = b[..., ::2]
    assert not view.is_contiguous()
    loss = MPJPE()(view, t)
    loss.backward()
    assert loss.dtype == torch.float32 and loss.dim() == 0 and b.grad.shape == base.shape and t.grad.shape == gt.shape
    for name, got, k in (("loss", loss.detach(), 0), ("dloss/dbase", b.grad, 1), ("dloss/dtarget", t.grad, 2)):
        _within("view " + name, got, refs[0][k], refs[1][k], ratios)
    assert torch.equal(t.grad, -b.grad[..., ::2]) and bool((b.grad[..., 1::2] == 0).all())
    # the target alone requires grad
    t2 = gt.cuda().requires_grad_(True)
    MPJPE()(base.cuda()[..., ::2], t2).backward()
    assert torch.equal(t2.grad, t.grad)
    # [B,17,2] keypoints (capf_mpjpe_nd)
    p2, g2 = torch.randn(5, 17, 2, generator=g), torch.randn(5, 17, 2, generator=g)
    l64, d64 = _mpjpe_reference(p2, g2, torch.float64)
    l32, d32 = _mpjpe_reference(p2, g2, torch.float32)
    q = p2.cuda().requires_grad_(True)
    loss = MPJPE()(q, g2.cuda())
    loss.backward()
    _within("2-D loss", loss.detach(), l64, l32, ratios)
    _within("2-D dpred", q.grad, d64, d32, ratios)
    # other float dtypes: computed in fp32, the loss and the gradients in the inputs' dtype like the reference's
    for dtype in (torch.bfloat16, torch.float16, torch.float64):
        p, t = p2.to(dtype).cuda().requires_grad_(True), g2.to(dtype).cuda().requires_grad_(True)
        loss = MPJPE()(p, t)
        loss.backward()
        assert loss.dtype == dtype and loss.dim() == 0
        for leaf in (p, t):
            assert leaf.grad.dtype == dtype and leaf.grad.shape == p2.shape and bool(torch.isfinite(leaf.grad).all())
        want, _ = _mpjpe_reference(p2.to(dtype), g2.to(dtype), torch.float64)
        eps = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float64: 0.0}[dtype]      # one rounding of the fp32 result to the dtype
        assert abs(loss.item() - want.item()) <= (eps + 2e-6) * want.item(), (dtype, loss.item(), want.item())        # (2e-6: the fp32 evaluation)
    print(f"  MPJPE(): worst error / bound {max(ratios):.3f}")


# ---- 4. keypoint losses ------------------------------------------------------------------------------------------------------------------------------
KP_ROWS, KP_THR = (1, 17, 1023, 1024, 1025, 3000), 0.5
VALIDITY = ("ones", "binary", "zeros", "fractional")


def _kp_case(rows, D, kind, seed=0):
    """pred, gt [rows, D], validity [rows, 1] (float32).  The weighted squared difference of every element is BUILT on one side of KP_THR:
    half of the elements in [0.01, 0.9] thr, half in [1.1, 6] thr (no element is filtered out or moved afterwards); a tenth of the
    elements have pred == gt (d == 0: MAE's kink)."""
    rng = np.random.default_rng([seed, rows, D, VALIDITY.index(kind)])
    v = {"ones": np.ones(rows), "binary": (rng.random(rows) > 0.3).astype(np.float64), "zeros": np.zeros(rows),
         "fractional": rng.choice([0.25, 0.5], rows)}[kind][:, None]
    term = np.where(rng.random((rows, D)) < 0.5, rng.uniform(0.01, 0.9, (rows, D)), rng.uniform(1.1, 6.0, (rows, D))) * KP_THR
    d = np.sqrt(term / np.where(v > 0, v, 1.0)) * rng.choice([-1.0, 1.0], (rows, D))
    d[rng.random((rows, D)) < 0.1] = 0.0
    gt = rng.standard_normal((rows, D)).astype(np.float32)
    pred = (gt.astype(np.float64) - d).astype(np.float32)
    pred[d == 0] = gt[d == 0]
    return torch.from_numpy(pred), torch.from_numpy(gt), torch.from_numpy(v.astype(np.float32))


def _kp_reference(mode, pred, gt, v, thr, dtype):
    """loss.py:104-137 in torch on the CPU with autograd -> (loss, dloss/dpred, the weighted terms before the smooth branch) in float64"""
    p, t, w = pred.to(dtype, copy=True).requires_grad_(True), gt.to(dtype), v.to(dtype)
    D = p.shape[-1]
    if mode == 2:
        diff = torch.abs(t - p) * w                                                   # :135
        terms = diff.detach()
    else:
        diff = (t - p) ** 2 * w                                                       # :110, :123
        terms = diff.detach().clone()
        if mode == 1:
            big = diff > thr                                                          # :124
            diff = diff.clone()
            diff[big] = torch.pow(diff[big], 0.1) * (thr ** 0.9)
    loss = torch.sum(diff) / (D * max(1, torch.sum(w).item()))
    loss.backward()
    return loss.detach().double(), p.grad.double(), terms.double()


def _kp_conditions(mode, rows, D, kind, pred, terms):
    """what the comparison rests on, asserted on the CPU before the kernel runs"""
    if mode != 1:
        return
    rel = (terms / KP_THR - 1.0).abs()
    assert rel.min().item() >= 1e-4, (rows, D, kind, rel.min().item())               # no element near the threshold
    if kind != "zeros" and rows * D >= 17:
        share = (terms > KP_THR).double().mean().item()
        assert 0.1 <= share <= 0.9, (rows, D, kind, share)


@pytest.mark.parametrize("mode", [0, 1, 2], ids=["mse", "mse_smooth", "mae"])
def test_keypoint_losses_loss_and_gradient_against_float64(mode):
    ratios = []
    for rows in KP_ROWS:
        for D in (1, 2, 3, 4):
            for kind in VALIDITY:
                pred, gt, v = _kp_case(rows, D, kind)
                l64, g64, terms = _kp_reference(mode, pred, gt, v, KP_THR, torch.float64)
                l32, g32, _ = _kp_reference(mode, pred, gt, v, KP_THR, torch.float32)
                _kp_conditions(mode, rows, D, kind, pred, terms)
                loss, dpred = capf.keypoints_loss(mode, pred.cuda(), gt.cuda(), v.cuda(), KP_THR, want_grad=True)
                loss0, none = capf.keypoints_loss(mode, pred.cuda(), gt.cuda(), v.cuda(), KP_THR, want_grad=False)
                tag = f"mode {mode} rows {rows} D {D} validity {kind}"
                assert none is None and torch.equal(loss.view(torch.int32), loss0.view(torch.int32)), tag
                assert dpred.shape == pred.shape and bool(torch.isfinite(dpred).all()) and bool(torch.isfinite(loss).all()), tag
                if kind == "zeros":                                                   # the max(1, .) denominator
                    assert loss.item() == 0 and bool((dpred == 0).all()), tag
                if mode == 2:
                    assert bool((dpred.cpu()[pred == gt] == 0).all()), tag          # d == 0 under MAE
                _within(tag + " loss", loss[0], l64, l32, ratios)
                _within(tag + " dpred", dpred, g64, g32, ratios)
    print(f"  keypoint loss mode {mode}: worst error / bound {max(ratios):.3f}")


@pytest.mark.parametrize("D", [1, 2, 3, 4])
def test_smooth_loss_term_equal_to_the_threshold_stays_quadratic(D):
    """d = +-0.5, weight 1, threshold 0.25: the term EQUALS the threshold and loss.py:124's strict `>` keeps it quadratic.  With one such
    element per row (the others d = 0) the loss is exactly 0.25 / D; with every element +-0.5 it is exactly 0.25; the gradient exactly
    -2 d / denom either way (the smooth branch would scale it by 0.1)."""
    rows = 37
    sign = torch.where(torch.arange(rows * D).reshape(rows, D) % 3 == 0, -1.0, 1.0)
    gt = torch.randint(-8, 9, (rows, D), generator=torch.Generator().manual_seed(D)).float()
    v = torch.ones(rows, 1)
    for per_row, want_loss in ((True, 0.25 / D), (False, 0.25)):
        d = 0.5 * sign
        if per_row:
            d = d * (torch.arange(D)[None, :] == (torch.arange(rows)[:, None] % D))
        pred = gt - d                                                                # (exact: halves of small integers)
        assert torch.equal(gt - pred, d)
        loss, dpred = capf.keypoints_loss(1, pred.cuda(), gt.cuda(), v.cuda(), 0.25, want_grad=True)
        assert loss.item() == np.float32(want_loss), (loss.item(), want_loss)
        want_grad = (-2.0 * d.double() / (D * rows)).float()
        assert torch.equal(dpred.cpu(), want_grad), (dpred.cpu() - want_grad).abs().max()


def test_keypoint_loss_classes_give_the_target_the_negated_gradient():
    from mvn.models.loss import KeypointsMAELoss, KeypointsMSELoss, KeypointsMSESmoothLoss
    pred, gt, v = _kp_case(17, 3, "binary", seed=5)
    for cls in (KeypointsMSELoss(), KeypointsMSESmoothLoss(KP_THR), KeypointsMAELoss()):
        p, t = pred.cuda().requires_grad_(True), gt.cuda().requires_grad_(True)
        cls(p, t, v.cuda()).backward()
        assert p.grad is not None and t.grad is not None and torch.equal(t.grad, -p.grad) and bool((p.grad != 0).any())
        t2 = gt.cuda().requires_grad_(True)
        cls(pred.cuda(), t2, v.cuda()).backward()
        assert torch.equal(t2.grad, t.grad)


# ---- 5. capf_preprocess, fliptest_fuse ---------------------------------------------------------------------------------------------------------------
def _preprocess_case(B, H, W, backbone, mode, with_gt):
    import capf_oracle as oracle
    g = torch.Generator().manual_seed(B * 1000 + H + mode)
    img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    gt = torch.randn(B, 1, 17, 3, generator=g)
    k2d = torch.rand(B, 17, 2, generator=g) * 2 - 1
    kc = torch.rand(B, 17, 2, generator=g) * 191
    wi, wgt, wk, wc = oracle.prefetch_preprocess(img, gt, k2d, kc, backbone, is_train=(mode == 1), flip=(mode == 1), flip_test=(mode == 2))
    got = capf.preprocess(img.cuda(), gt.cuda() if with_gt else None, k2d.cuda(), kc.cuda(), backbone, mode)
    if mode == 2:      # the reference stacks on dim 1 ([B,2,...]); the kernel emits [2,B,...]
        wi, wk, wc = wi.transpose(0, 1), wk.transpose(0, 1), wc.transpose(0, 1)
    tag = (B, H, W, backbone, mode, with_gt)
    assert torch.equal(got[0].cpu().view(torch.int32), wi.contiguous().view(torch.int32)), tag
    if with_gt:
        assert torch.equal(got[1].cpu().view(torch.int32), wgt.view(torch.int32)), tag
    else:
        assert got[1] is None, tag
    assert torch.equal(got[2].cpu().view(torch.int32), wk.contiguous().view(torch.int32)), tag
    assert torch.equal(got[3].cpu().view(torch.int32), wc.contiguous().view(torch.int32)), tag


@pytest.mark.parametrize("shape", [(1, 256, 192), (3, 256, 256), (2, 384, 288), (5, 8, 8)], ids=lambda s: "x".join(map(str, s)))
def test_preprocess_bit_exact_at_every_shape_mode_and_normalisation(shape):
    for backbone in ("hrnet_32", "cpn"):
        for mode in (0, 1, 2):
            for with_gt in (True, False):
                _preprocess_case(*shape, backbone, mode, with_gt)


@pytest.mark.parametrize("backbone", ["hrnet_32", "cpn"])
def test_preprocess_bit_exact_on_the_second_trip_of_the_grid_loop(backbone):
    """17 x 256 x 256 in flip-test mode: 2,228,224 pixels over both sets, 131,072 more than the 8192 blocks of 256 threads take in one trip"""
    assert 2 * 17 * 256 * 256 > 8192 * 256
    _preprocess_case(17, 256, 256, backbone, 2, backbone == "cpn")


def _swap_table(J, seed):
    """a seeded permutation that is its own inverse: disjoint pairs swapped, the rest fixed"""
    order = np.random.default_rng([seed, J]).permutation(J)
    tab = np.arange(J)
    for a, b in zip(order[0:2 * (J // 3):2], order[1:2 * (J // 3):2]):
        tab[a], tab[b] = b, a
    return tab.tolist()


@pytest.mark.parametrize("B", [1, 128, 129])          # 128 x 17 threads are whole blocks of 128
def test_fliptest_fuse_bits_for_every_table_with_signed_zeros_and_infinities(B):
    import capf_oracle as oracle
    for J, swap in ((17, None), (1, [0]), (16, _swap_table(16, 1)), (32, _swap_table(32, 2)), (17, list(capf.MPI_SWAP))):
        g = torch.Generator().manual_seed(B * 100 + J)
        p = torch.randn(2, B, 1, J, 3, generator=g)
        flat = p.view(-1)
        flat[torch.randperm(flat.numel(), generator=g)[:flat.numel() // 8]] = 0.0
        flat[torch.randperm(flat.numel(), generator=g)[:flat.numel() // 8]] = -0.0
        # infinities where the other operand of the sum is finite or zero (component 0 of the first set, component 1 of the second): inf - inf would
        # be a NaN, whose sign and payload are the processor's choice and no property of the kernel
        p[0, 0, 0, 0, 0], p[0, B - 1, 0, J - 1, 0] = float("inf"), float("-inf")
        p[1, 0, 0, 0, 1], p[1, B - 1, 0, J - 1, 1] = float("-inf"), float("inf")
        tab = list(range(J)) if swap is None else swap
        flip = p[1].clone()                                                           # train.py:177-180, run_3dhp.py:169-180
        flip[:, :, :, 0] *= -1
        flip = flip[:, :, tab]                                                        # joint j takes the mirrored prediction's joint swap[j]
        want = oracle.fliptest_fuse(p[0], p[1]) if swap is None else torch.mean(torch.cat((p[0], flip), dim=1), dim=1, keepdim=True)
        assert not bool(torch.isnan(want).any()) and bool(torch.isinf(want).any())
        got = capf.fliptest_fuse(p.cuda(), swap)
        assert got.shape == (B, 1, J, 3)
        assert torch.equal(got.cpu().view(torch.int32), want.view(torch.int32)), (B, J, swap)
