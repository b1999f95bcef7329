"""GPU: capf_keypoints_l2_loss, capf_limb_length_errors / capf_limb_length_sums and capf_uncertainty_loss (csrc/pose_losses.hip) and the
classes of mvn.models.loss on top of them.

    reference goldens   tests/golden/losses_extra.npz, the tolerances of tests/test_loss_extra.py
    float64             loss, per-pose errors and every gradient element against tests/loss_extra_cases.py on the device's own inputs,
                        |got - want| <= 2^-23 |want| + 1e-12 mass (loss_extra_cases.bound: one float32 store; where want and mass are 0 the
                        element must BE 0)
    singular points     pred == gt, validity 0 / all 0 / fractional, coincident joints in pred / gt / both, equal lengths: finite everywhere,
                        exact zeros where the header says so -- also where the reference expression's autograd returns NaN
    reproducibility     two calls, and the call without gradients: the same bits"""
import numpy as np
import pytest
import torch

import loss_extra_cases as lc
from capf import lib as capf
from conftest import load_golden
from metric_edge_cases import permuted_segments

pytestmark = pytest.mark.gpu


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


def _same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    view = {4: torch.int32, 8: torch.int64}[a.element_size()]
    return a.shape == b.shape and torch.equal(a.contiguous().view(view), b.contiguous().view(view))


def _held(tag, got, want, mass, worst):
    """every element finite and within the one-store bound; notes the worst error / bound"""
    got, want, mass = np.asarray(got, np.float64), np.asarray(want, np.float64), np.asarray(mass, np.float64)
    assert got.shape == want.shape, (tag, got.shape, want.shape)
    assert np.isfinite(got).all(), f"{tag}: non-finite output"
    err, bnd = np.abs(got - want), lc.bound(want, mass)
    bad = err > bnd
    assert not bad.any(), f"{tag}: {int(bad.sum())} elements beyond the bound, worst {float((err - bnd).max()):.3e} at {np.argwhere(bad)[0].tolist()}"
    live = bnd > 0
    if live.any():
        worst.append(float((err[live] / bnd[live]).max()))


# ---- 1. the classes against the reference's numbers ------------------------------------------------------------------------------------------------
def test_classes_equal_the_reference_on_metric_inputs():
    from mvn.models.loss import UNCERTAINTY, KeypointsL2Loss, LimbLengthError
    gold = load_golden("losses_extra")
    pred, gt, validity, sigmas = lc.golden_inputs()
    p, g = _dev(pred), _dev(gt)
    l2 = KeypointsL2Loss()(p, g, _dev(validity))
    unc = UNCERTAINTY([_dev(s) for s in sigmas], p, g)
    limb, limb_np = LimbLengthError()(p, g), LimbLengthError()(pred, gt)
    assert l2.dim() == 0 and l2.dtype == torch.float32 and unc.dim() == 0 and unc.dtype == torch.float32
    assert type(limb) is float and type(limb_np) is float and limb == limb_np
    print(f"  relative distance from the reference: L2 {abs(l2.item() / gold['l2_loss'] - 1):.2e}, limb {abs(limb / gold['limb_error'] - 1):.2e}, "
          f"uncertainty {abs(unc.item() / gold['uncertainty_loss'] - 1):.2e}")
    np.testing.assert_allclose(l2.item(), gold["l2_loss"], rtol=lc.GOLDEN_RTOL, atol=0)
    np.testing.assert_allclose(unc.item(), gold["uncertainty_loss"], rtol=lc.GOLDEN_RTOL, atol=0)
    np.testing.assert_allclose(limb, gold["limb_error"], rtol=lc.GOLDEN_RTOL, atol=lc.LIMB_ATOL_ULPS * lc.mean_limb_length(pred, gt))


def test_gradients_equal_the_reference_autograd_where_it_is_finite():
    from mvn.models.loss import UNCERTAINTY, KeypointsL2Loss
    gold = load_golden("losses_extra")
    pred, gt, _, sigmas = lc.golden_inputs()
    n = lc.GRAD_POSES
    p = _dev(pred[:n]).requires_grad_(True)
    loss = KeypointsL2Loss()(p, _dev(gt[:n]), torch.ones(n, 17, 1, device="cuda"))
    loss.backward()
    np.testing.assert_allclose(loss.item(), gold["l2_ones_loss"], rtol=lc.GOLDEN_RTOL, atol=0)
    np.testing.assert_allclose(_np(p.grad), gold["l2_ones_dpred"], rtol=0, atol=lc.GOLDEN_RTOL * np.abs(gold["l2_ones_dpred"]).max())
    p = _dev(pred[:n]).requires_grad_(True)
    sg = [_dev(s[:n]).requires_grad_(True) for s in sigmas]
    loss = UNCERTAINTY(sg, p, _dev(gt[:n]))
    loss.backward()
    np.testing.assert_allclose(loss.item(), gold["uncertainty_grad_loss"], rtol=lc.GOLDEN_RTOL, atol=0)
    for got, name in [(p.grad, "uncertainty_dpred")] + [(sg[k].grad, f"uncertainty_dsigma{k}") for k in range(2)]:
        assert tuple(got.shape) == gold[name].shape, name
        np.testing.assert_allclose(_np(got), gold[name], rtol=0, atol=lc.GOLDEN_RTOL * np.abs(gold[name]).max(), err_msg=name)


# ---- 2. capf_keypoints_l2_loss ---------------------------------------------------------------------------------------------------------------------------
def _reference_l2_grad(pred, gt, v):
    """loss.py:145-146 in torch float64 on the CPU with autograd: NaN as soon as one square root sits at 0"""
    p = torch.from_numpy(pred).double().requires_grad_(True)
    w = torch.from_numpy(v).double()
    loss = torch.sum(torch.sqrt(torch.sum((torch.from_numpy(gt).double() - p) ** 2 * w, dim=-1)))
    (loss / max(1, torch.sum(w).item())).backward()
    return p.grad


@pytest.mark.parametrize("rows", [1, 17, 1023, 1025, 512 * 17])
def test_keypoints_l2_loss_and_gradient_against_float64(rows):
    worst = []
    for D in (1, 2, 3, 5):
        for kind in ("ones", "binary", "zeros", "fractional"):
            pred, gt, v = lc.l2_case(rows, D, kind)
            p, g, w = _dev(pred), _dev(gt), _dev(v)
            for scale in (1.0, 1.0 / 3.0):
                tag = f"rows {rows} D {D} validity {kind} grad_scale {scale:.3f}"
                want = lc.keypoints_l2(pred, gt, v, scale)
                loss, dpred = capf.keypoints_l2_loss(p, g, w, want_grad=True, grad_scale=scale)
                loss2, dpred2 = capf.keypoints_l2_loss(p, g, w, want_grad=True, grad_scale=scale)
                loss0, none = capf.keypoints_l2_loss(p, g, w, want_grad=False)
                assert none is None and _same_bits(loss, loss2) and _same_bits(loss, loss0) and _same_bits(dpred, dpred2), tag
                _held(tag + " loss", _np(loss)[0], want["loss"], want["loss_mass"], worst)
                _held(tag + " dpred", _np(dpred), want["dpred"], want["dpred_mass"], worst)
                dead = (v[:, 0] == 0) | (pred == gt).all(1)
                assert (rows < 5 or dead[4]) and bool((dpred[_dev(dead)] == 0).all()), tag          # exact zeros: the masked row, the exact hit
                if kind == "zeros":
                    assert loss.item() == 0 and bool((dpred == 0).all()), tag        # the denominator is max(1, 0)
            if rows == 17:
                assert torch.isnan(_reference_l2_grad(pred, gt, v)).any(), "the reference expression's gradient should be NaN on this case"
    print(f"  rows {rows}: worst error / bound {max(worst, default=0.0):.3f}")


def test_keypoints_l2_class_target_gradient_views_and_dtypes():
    from mvn.models.loss import KeypointsL2Loss
    pred, gt, v = lc.l2_case(34, 3, "binary", seed=4)
    pred, gt, v = pred.reshape(2, 17, 3), gt.reshape(2, 17, 3), v.reshape(2, 17, 1)
    want = lc.keypoints_l2(pred, gt, v)
    worst = []
    p, t = _dev(pred).requires_grad_(True), _dev(gt).requires_grad_(True)
    loss = KeypointsL2Loss()(p, t, _dev(v))
    loss.backward()
    _held("class loss", loss.item(), want["loss"], want["loss_mass"], worst)
    _held("class dpred", _np(p.grad), want["dpred"], want["dpred_mass"], worst)
    assert torch.equal(t.grad, -p.grad) and bool((p.grad != 0).any())
    t2 = _dev(gt).requires_grad_(True)
    KeypointsL2Loss()(_dev(pred), t2, _dev(v)).backward()                             # the target alone requires grad
    assert torch.equal(t2.grad, t.grad)
    base = torch.zeros(2, 17, 6, device="cuda")                                       # a non-contiguous view of a leaf
    base[..., ::2] = _dev(pred)
    base.requires_grad_(True)
    KeypointsL2Loss()(base[..., ::2], _dev(gt), _dev(v)).backward()
    assert torch.equal(base.grad[..., ::2], p.grad) and bool((base.grad[..., 1::2] == 0).all())
    for dtype, eps in ((torch.bfloat16, 2.0 ** -8), (torch.float16, 2.0 ** -11), (torch.float64, 0.0)):
        q, s = _dev(pred).to(dtype).requires_grad_(True), _dev(gt).to(dtype)
        loss = KeypointsL2Loss()(q, s, _dev(v))
        loss.backward()
        ref = lc.keypoints_l2(q.detach().float().cpu().numpy(), s.float().cpu().numpy(), v)["loss"]
        assert loss.dtype == dtype and q.grad.dtype == dtype and bool(torch.isfinite(q.grad).all())
        assert abs(loss.item() - ref) <= (eps + 2e-6) * ref, (dtype, loss.item(), ref)          # one rounding of the fp32 result to the dtype


# ---- 3. capf_limb_length_errors, capf_limb_length_sums ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 1023, 1025, 4097])
def test_limb_errors_gradients_and_sums_against_float64(n):
    worst = []
    for name, (J, limbs) in lc.LIMB_TABLES.items():
        pred, gt = lc.limb_case(n, J)
        p, g = _dev(pred), _dev(gt)
        L, scale = len(limbs), 1.0 / (n * len(limbs))
        tag = f"n {n} table {name}"
        want, want_gt = lc.limb_errors(pred, gt, limbs, scale), lc.limb_errors(gt, pred, limbs, scale)
        err, dpred = capf.limb_length_errors(p, g, limbs, want_grad=True, grad_scale=scale)
        err2, dpred2 = capf.limb_length_errors(p, g, limbs, want_grad=True, grad_scale=scale)
        err0, none = capf.limb_length_errors(p, g, limbs)
        errx, dgt = capf.limb_length_errors(g, p, limbs, want_grad=True, grad_scale=scale)          # the roles exchanged: the target's gradient
        assert none is None and err.shape == (n, L) and dpred.shape == (n, J, 3)
        assert _same_bits(err, err2) and _same_bits(err, err0) and _same_bits(err, errx) and _same_bits(dpred, dpred2), tag
        _held(tag + " err", _np(err), want["err"], want["err_mass"], worst)
        _held(tag + " dpred", _np(dpred), want["dpred"], want["dpred_mass"], worst)
        _held(tag + " dgt", _np(dgt), want_gt["dpred"], want_gt["dpred_mass"], worst)
        if n >= 8 and name == "h36m":
            k = _dev(np.arange(n) % 8)
            assert bool((err[k == 1] == 0).all()) and bool((dpred[k == 1] == 0).all()), tag + ": pred == gt"
            assert bool((err[k == 2] == 0).all()) and bool((dpred[k == 2] == 0).all()) and bool((dgt[k == 2] == 0).all()), tag + ": equal lengths"
            assert bool((dpred[k == 6] == 0).all()) and bool((err[k == 6] > 0).all()), tag + ": all of pred one point"
            assert bool((err[k == 5][:, 0] == 0).all()), tag + ": limb (0, 1) has length 0 in both"
        if name == "a_equals_b":
            assert bool((err[:, 1] == 0).all()) and bool((err[:, 3] == 0).all()) and bool((dpred[:, 2] == 0).all()), tag
        # the sums: one segment without a table; three segments, ids in a seeded random order, the last one empty
        e64 = _np(err)
        for S in (1, 3):
            seg = None if S == 1 else permuted_segments(n, 2, seed=7)
            d_seg = None if seg is None else _dev(seg)
            sums, counts = capf.limb_length_sums(err, d_seg, n_segments=S)
            sums2, counts2 = capf.limb_length_sums(err, d_seg, n_segments=S)
            assert _same_bits(sums, sums2) and torch.equal(counts, counts2), tag
            assert sums.dtype == torch.float64 and counts.dtype == torch.int64 and sums.shape == (S, L) and counts.shape == (S,)
            for s in range(S):
                m = np.ones(n, bool) if seg is None else seg == s
                assert int(counts[s]) == int(m.sum()), (tag, S, s)
                np.testing.assert_allclose(_np(sums[s]), e64[m].sum(0), rtol=1e-12, atol=0, err_msg=f"{tag} segment {s} of {S}")
            if S == 3:
                assert int(counts[2]) == 0 and bool((sums[2] == 0).all()), tag       # the empty segment
    print(f"  n {n}: worst error / bound {max(worst, default=0.0):.3f}")


def test_limb_length_loss_value_both_gradients_and_shapes():
    from mvn.models.loss import LimbLengthError, limb_length_loss
    n = 24
    pred, gt = lc.limb_case(n, 17, seed=2)
    scale = 1.0 / (n * 16)
    want, want_gt = lc.limb_errors(pred, gt, grad_scale=scale), lc.limb_errors(gt, pred, grad_scale=scale)
    worst = []
    p, t = _dev(pred).requires_grad_(True), _dev(gt).requires_grad_(True)
    loss = limb_length_loss(p, t)
    loss.backward()
    assert loss.dim() == 0 and loss.dtype == torch.float32
    figure = lc.limb_length_error(pred, gt)
    _held("limb_length_loss", loss.item(), figure, want["err_mass"].mean(), worst)
    _held("dloss/dpred", _np(p.grad), want["dpred"], want["dpred_mass"], worst)
    _held("dloss/dgt", _np(t.grad), want_gt["dpred"], want_gt["dpred_mass"], worst)
    assert bool(torch.isfinite(p.grad).all()) and bool(torch.isfinite(t.grad).all())
    assert abs(LimbLengthError()(p, t) - figure) <= 2.0 ** -23 * figure + 1e-12 * want["err_mass"].mean()
    # [b, 1, 17, 3] as the model returns it; a weight on the loss scales the gradient; a table of the caller's
    q = _dev(pred[:, None]).requires_grad_(True)
    (0.1 * limb_length_loss(q, _dev(gt[:, None]))).backward()
    assert q.grad.shape == (n, 1, 17, 3) and torch.equal(q.grad[:, 0], p.grad * 0.1)
    limbs = lc.LIMB_TABLES["repeated"][1]
    q = _dev(pred[:, :5]).requires_grad_(True)
    loss = limb_length_loss(q, _dev(gt[:, :5]), limbs=limbs)
    loss.backward()
    w5 = lc.limb_errors(pred[:, :5], gt[:, :5], limbs, 1.0 / (n * len(limbs)))
    _held("caller's table", loss.item(), w5["err"].mean(), w5["err_mass"].mean(), worst)
    _held("caller's table dpred", _np(q.grad), w5["dpred"], w5["dpred_mass"], worst)
    # no gradient wanted: the same value
    assert limb_length_loss(_dev(pred), _dev(gt)).item() == limb_length_loss(p, t).item()


# ---- 4. capf_uncertainty_loss ------------------------------------------------------------------------------------------------------------------------------
def _unc_inputs(rows, D, seed=0):
    """pred, gt [rows, D]; rows 4, 9, 14, ... have pred == gt: a scaled residual of norm 0"""
    rng = np.random.default_rng([seed, rows, D])
    gt = rng.standard_normal((rows, D)).astype(np.float32)
    pred = (gt + 0.1 * rng.standard_normal((rows, D))).astype(np.float32)
    pred[4::5] = gt[4::5]
    return pred, gt


@pytest.mark.parametrize("rows", [1, 17, 1023, 1025, 512 * 17])
def test_uncertainty_loss_and_every_gradient_against_float64(rows):
    worst = []
    for D in (1, 2, 3, 5):
        pred, gt = _unc_inputs(rows, D)
        p, g = _dev(pred), _dev(gt)
        for K, widths in lc.SIGMA_SETS.items():
            sig = lc.sigma_case(rows, D, widths)
            d_sig = [_dev(s) for s in sig]
            for scale in (1.0, 1.0 / 3.0):
                tag = f"rows {rows} D {D} K {K} grad_scale {scale:.3f}"
                want = lc.uncertainty(pred, gt, sig, scale)
                loss, dpred, dsig = capf.uncertainty_loss(p, g, d_sig, want_dpred=True, want_dsigma=[True] * K, grad_scale=scale)
                loss2, dpred2, dsig2 = capf.uncertainty_loss(p, g, d_sig, want_dpred=True, want_dsigma=[True] * K, grad_scale=scale)
                loss0, none, nones = capf.uncertainty_loss(p, g, d_sig)
                assert none is None and nones == [None] * K and _same_bits(loss, loss2) and _same_bits(loss, loss0) and _same_bits(dpred, dpred2), tag
                assert all(_same_bits(a, b) for a, b in zip(dsig, dsig2)), tag
                _held(tag + " loss", _np(loss)[0], want["loss"], want["loss_mass"], worst)
                _held(tag + " dpred", _np(dpred), want["dpred"], want["dpred_mass"], worst)
                for k in range(K):
                    assert dsig[k].shape == d_sig[k].shape, tag
                    _held(f"{tag} dsigma {k}", _np(dsig[k]), want["dsigma"][k], want["dsigma_mass"][k], worst)
                assert bool((dpred[4::5] == 0).all()), tag                             # pred == gt: the norm term gives 0, not NaN
            if K == 2:                                                                # some gradients only: the others untouched, the same bits
                _, only_p, none2 = capf.uncertainty_loss(p, g, d_sig, want_dpred=True)
                _, no_p, one = capf.uncertainty_loss(p, g, d_sig, want_dsigma=[False, True])
                l1, dp1, ds1 = capf.uncertainty_loss(p, g, d_sig, want_dpred=True, want_dsigma=[True, True])
                assert none2 == [None, None] and no_p is None and one[0] is None
                assert _same_bits(only_p, dp1) and _same_bits(one[1], ds1[1]), (rows, D)
    print(f"  rows {rows}: worst error / bound {max(worst, default=0.0):.3f}")


def test_uncertainty_class_at_zero_residuals_and_nan_where_sigma_is_not_positive():
    """Rows with pred == gt: the scaled residual has norm 0 and the norm term contributes 0 to every gradient (what torch.norm's backward
    does at 0 depends on the torch version; the kernel's rule does not).  sigma + 1e-6 <= 0: NaN, unclamped."""
    from mvn.models.loss import UNCERTAINTY
    pred, gt = _unc_inputs(34, 3, seed=1)
    pred, gt = pred.reshape(2, 17, 3), gt.reshape(2, 17, 3)
    sig = [s.reshape(2, 17, -1) for s in lc.sigma_case(34, 3, ("full", "one"), seed=1)]
    want = lc.uncertainty(pred, gt, sig)
    assert (pred[0, 4] == gt[0, 4]).all() and (want["dpred"][0, 4] == 0).all()
    worst = []
    p, t = _dev(pred).requires_grad_(True), _dev(gt).requires_grad_(True)
    sg = [_dev(s).requires_grad_(True) for s in sig]
    loss = UNCERTAINTY(sg, p, t)
    loss.backward()
    _held("loss", loss.item(), want["loss"], want["loss_mass"], worst)
    _held("dpred", _np(p.grad), want["dpred"], want["dpred_mass"], worst)
    assert torch.equal(t.grad, -p.grad)
    for k in range(2):
        assert sg[k].grad.shape == sg[k].shape
        _held(f"dsigma {k}", _np(sg[k].grad), want["dsigma"][k], want["dsigma_mass"][k], worst)
    # sigma + 1e-6 <= 0 is not clamped: s < 0 in row 3 of the full sigma and, barely, in row 20 of the [.., 1] one
    bad = [s.copy() for s in sig]
    bad[0][0, 3, 1] = -0.25
    bad[1][1, 3, 0] = -1.5e-6
    assert np.float64(bad[1][1, 3, 0]) + 1e-6 < 0
    loss, dpred, dsig = capf.uncertainty_loss(_dev(pred), _dev(gt), [_dev(s) for s in bad], want_dpred=True, want_dsigma=[True, True])
    assert torch.isnan(loss).all()
    dp, d0, d1 = _np(dpred).reshape(34, 3), _np(dsig[0]).reshape(34, 3), _np(dsig[1]).reshape(34)
    assert np.isnan(dp[[3, 20]]).all() and np.isfinite(np.delete(dp, [3, 20], 0)).all()
    assert np.isnan(d0[3]).all() and np.isfinite(np.delete(d0, 3, 0)).all()
    assert np.isnan(d1[20]) and np.isfinite(np.delete(d1, 20)).all()


def test_uncertainty_dtypes_and_target_alone():
    from mvn.models.loss import UNCERTAINTY
    pred, gt = _unc_inputs(34, 2, seed=2)
    sig = lc.sigma_case(34, 2, ("one", "full"), seed=2)
    t = _dev(gt).requires_grad_(True)
    UNCERTAINTY([_dev(s) for s in sig], _dev(pred), t).backward()
    want = lc.uncertainty(pred, gt, sig)
    _held("target alone", _np(t.grad), -want["dpred"], want["dpred_mass"], [])
    q = _dev(pred).to(torch.bfloat16).requires_grad_(True)
    s16 = [_dev(s).to(torch.bfloat16).requires_grad_(True) for s in sig]
    loss = UNCERTAINTY(s16, q, _dev(gt).to(torch.bfloat16))
    loss.backward()
    assert loss.dtype == torch.bfloat16 and q.grad.dtype == torch.bfloat16 and all(s.grad.dtype == torch.bfloat16 and s.grad.shape == s.shape for s in s16)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(q.grad).all())
