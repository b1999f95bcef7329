"""CPU: KeypointsL2Loss, LimbLengthError / limb_length_loss and UNCERTAINTY without a device -- the float64 restatements of
tests/loss_extra_cases.py against what the reference returned (tests/golden/losses_extra.npz, tools/make_loss_goldens.py), the four C
entries in the binding, the header and the built library, and every refusal that is decided before a launch.

Tolerances against the reference: rtol 2e-6 (tests/test_metrics.py's figure for the sibling losses: the reference is torch float32);
LimbLengthError also atol 2^-21 x the mean limb length, because the reference subtracts two float32 norms, each good to a few ulp of a
length and not of their difference.  Gradient fixtures: 2e-6 of the gradient's largest entry."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import loss_extra_cases as lc
from conftest import ROOT, load_golden

INVALID, UNSUPPORTED = -1, -2          # include/capf.h :: CAPF_ERR_INVALID, CAPF_ERR_UNSUPPORTED
NEW = ("capf_keypoints_l2_loss", "capf_limb_length_errors", "capf_limb_length_sums", "capf_uncertainty_loss")


# ---- the restatements against the reference ------------------------------------------------------------------------------------------------------
def test_restatements_equal_the_reference_on_metric_inputs():
    gold = load_golden("losses_extra")
    pred, gt, validity, sigmas = lc.golden_inputs()
    assert pred.shape == (96, 17, 3) and (validity == 0).any() and [s.shape[-1] for s in sigmas] == [3, 1]
    assert all(0.05 <= s.min() and s.max() <= 0.55 for s in sigmas)
    l2 = lc.keypoints_l2(pred, gt, validity)["loss"]
    limb = lc.limb_length_error(pred, gt)
    unc = lc.uncertainty(pred, gt, sigmas)["loss"]
    print(f"  relative distance from the reference: L2 {abs(l2 / gold['l2_loss'] - 1):.2e}, limb {abs(limb / gold['limb_error'] - 1):.2e}, "
          f"uncertainty {abs(unc / gold['uncertainty_loss'] - 1):.2e}")
    np.testing.assert_allclose(l2, gold["l2_loss"], rtol=lc.GOLDEN_RTOL, atol=0)
    np.testing.assert_allclose(unc, gold["uncertainty_loss"], rtol=lc.GOLDEN_RTOL, atol=0)
    atol = lc.LIMB_ATOL_ULPS * lc.mean_limb_length(pred, gt)
    np.testing.assert_allclose(limb, gold["limb_error"], rtol=lc.GOLDEN_RTOL, atol=atol)
    np.testing.assert_allclose(limb, gold["limb_error_numpy_arguments"], rtol=lc.GOLDEN_RTOL, atol=atol)


def test_restated_gradients_equal_the_reference_autograd_where_it_is_finite():
    gold = load_golden("losses_extra")
    pred, gt, _, sigmas = lc.golden_inputs()
    n = lc.GRAD_POSES
    l2 = lc.keypoints_l2(pred[:n], gt[:n], np.ones((n, 17, 1), np.float32))
    np.testing.assert_allclose(l2["loss"], gold["l2_ones_loss"], rtol=lc.GOLDEN_RTOL, atol=0)
    np.testing.assert_allclose(l2["dpred"], gold["l2_ones_dpred"], rtol=0, atol=lc.GOLDEN_RTOL * np.abs(gold["l2_ones_dpred"]).max())
    unc = lc.uncertainty(pred[:n], gt[:n], [s[:n] for s in sigmas])
    np.testing.assert_allclose(unc["loss"], gold["uncertainty_grad_loss"], rtol=lc.GOLDEN_RTOL, atol=0)
    for got, name in [(unc["dpred"], "uncertainty_dpred")] + [(unc["dsigma"][k], f"uncertainty_dsigma{k}") for k in range(2)]:
        assert got.shape == gold[name].shape, name
        np.testing.assert_allclose(got, gold[name], rtol=0, atol=lc.GOLDEN_RTOL * np.abs(gold[name]).max(), err_msg=name)


def test_restated_gradients_are_the_derivatives_of_the_restated_losses():
    """central differences in float64 at a regular point: the closed forms of loss_extra_cases are the gradients of its own loss values"""
    rng = np.random.default_rng(3)
    pred, gt = rng.standard_normal((5, 4, 3)).astype(np.float32), rng.standard_normal((5, 4, 3)).astype(np.float32)
    v = rng.choice([0.5, 1.0], (5, 4, 1)).astype(np.float32)
    sig = [rng.uniform(0.2, 0.6, (5, 4, w)).astype(np.float32) for w in (3, 1)]
    limbs = ((0, 1), (1, 2), (3, 1), (0, 1))
    h = 2.0 ** -10            # (exact in float32 beside values of order 1, so the perturbed inputs are the float32 numbers the functions see)

    def numeric(f, x):
        g = np.zeros(x.shape)
        for idx in np.ndindex(*x.shape):
            up, dn = x.copy(), x.copy()
            up[idx] += np.float32(h)
            dn[idx] -= np.float32(h)
            g[idx] = (f(up) - f(dn)) / (float(up[idx]) - float(dn[idx]))
        return g

    pairs = [(lc.keypoints_l2(pred, gt, v)["dpred"], numeric(lambda x: lc.keypoints_l2(x, gt, v)["loss"], pred)),
             (lc.limb_errors(pred, gt, limbs)["dpred"], numeric(lambda x: lc.limb_errors(x, gt, limbs)["err"].sum(), pred)),
             (lc.uncertainty(pred, gt, sig)["dpred"], numeric(lambda x: lc.uncertainty(x, gt, sig)["loss"], pred)),
             (-lc.uncertainty(pred, gt, sig)["dpred"], numeric(lambda x: lc.uncertainty(pred, x, sig)["loss"], gt))]
    pairs += [(lc.uncertainty(pred, gt, sig)["dsigma"][k], numeric(lambda x, k=k: lc.uncertainty(pred, gt, sig[:k] + [x] + sig[k + 1:])["loss"], sig[k]))
              for k in range(2)]
    for closed, num in pairs:
        assert closed.shape == num.shape
        assert np.abs(closed - num).max() <= 1e-4 * np.abs(num).max()          # (h^2 truncation of the central difference)


# ---- the entries in the binding, the header and the library ----------------------------------------------------------------------------------------
def test_new_entries_are_exported_declared_and_bound_inside_revision_12():
    from capf import lib as capf_lib
    lib = capf_lib.load_library()
    assert lib.capf_abi_version() == 12 == capf_lib.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "capf.h")).read()
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", capf_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = {line.split()[-1] for line in out.splitlines() if line.strip()}
    for name in NEW:
        assert name in capf_lib.EXPORTS and name in capf_lib.PROTOTYPES and hasattr(lib, name), name
        assert f"int {name}(void* stream, " in header and name in defined, name
    for ref_line in ("loss.py:140-147", "loss.py:181-201", "loss.py:7-13"):
        assert ref_line in header


def test_the_new_names_import_from_the_loss_module():
    from mvn.models.loss import CONNECTIVITY_DICT, UNCERTAINTY, KeypointsL2Loss, LimbLengthError, limb_length_loss
    assert tuple(LimbLengthError().CONNECTIVITY_DICT) == CONNECTIVITY_DICT == lc.CONNECTIVITY and len(CONNECTIVITY_DICT) == 16
    assert callable(UNCERTAINTY) and callable(limb_length_loss) and isinstance(KeypointsL2Loss(), torch.nn.Module)


# ---- refusals of the C entries before a launch (the pointers are never dereferenced) ----------------------------------------------------------------
F = 4096


def _table(*pairs):
    return (ctypes.c_int32 * (2 * len(pairs)))(*[v for p in pairs for v in p])


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    from capf.lib import load_library
    lib = load_library()
    l2 = lambda pred=F, gt=F, v=F, rows=4, dim=3, loss=F: lib.capf_keypoints_l2_loss(None, pred, gt, v, rows, dim, loss, None, 1.0)
    assert [l2(pred=None), l2(gt=None), l2(v=None), l2(loss=None), l2(rows=0), l2(dim=0)] == [INVALID] * 6
    limb = lambda table=_table((0, 1)), L=1, J=17, n=4, err=F: lib.capf_limb_length_errors(None, F, F, n, J, table, L, err, None, 1.0)
    assert limb(table=_table((0, 17))) == INVALID and limb(table=_table((0, 1), (-1, 2)), L=2) == INVALID        # an index outside [0, joints)
    assert limb(table=_table((1, 2)), J=2) == INVALID
    assert limb(L=0) == INVALID and limb(table=_table(*[(0, 1)] * 65), L=65) == INVALID and limb(table=None) == INVALID
    assert limb(n=0) == INVALID and limb(J=0) == INVALID and limb(err=None) == INVALID
    assert limb(J=33) == UNSUPPORTED
    sums = lambda seg=None, n=4, L=16, S=1, out=F, cnt=F: lib.capf_limb_length_sums(None, F, seg, n, L, S, out, cnt)
    assert [sums(S=2), sums(S=0), sums(n=0), sums(L=0), sums(L=65), sums(out=None), sums(cnt=None)] == [INVALID] * 7

    def unc(K=2, widths=(3, 1), dim=3, rows=4, sig=(F, F), dsig=None, loss=F):
        ptrs = (ctypes.c_void_p * max(len(sig), 1))(*sig)
        w = (ctypes.c_int32 * max(len(widths), 1))(*widths)
        return lib.capf_uncertainty_loss(None, F, F, rows, dim, ptrs, w, K, loss, None, dsig, 1.0)

    assert unc(K=0) == INVALID and unc(K=9, widths=(3,) * 9, sig=(F,) * 9) == INVALID
    assert unc(widths=(3, 2)) == INVALID and unc(widths=(0, 1)) == INVALID and unc(widths=(3, 3), dim=2) == INVALID      # neither dim nor 1
    assert unc(sig=(F, None)) == INVALID and unc(rows=0) == INVALID and unc(dim=0) == INVALID and unc(loss=None) == INVALID
    assert lib.capf_uncertainty_loss(None, F, F, 4, 3, None, None, 1, F, None, None, 1.0) == INVALID


# ---- refusals of the host package ------------------------------------------------------------------------------------------------------------------
def test_host_classes_refuse_cpu_tensors_and_bad_shapes_without_a_gpu():
    from capf.lib import CapfError
    from mvn.models.loss import UNCERTAINTY, KeypointsL2Loss, LimbLengthError, limb_length_loss
    p, g, v = torch.zeros(2, 17, 3), torch.ones(2, 17, 3), torch.ones(2, 17, 1)
    sig = [torch.full((2, 17, 3), 0.3), torch.full((2, 17, 1), 0.3)]
    for call in (lambda: KeypointsL2Loss()(p, g, v), lambda: LimbLengthError()(p, g), lambda: limb_length_loss(p, g),
                 lambda: UNCERTAINTY(sig, p, g)):
        with pytest.raises(CapfError, match="MI355X only"):
            call()
    # a shape mismatch
    with pytest.raises(CapfError, match="differ in shape"):
        KeypointsL2Loss()(p, g[:, :16], v)
    with pytest.raises(CapfError, match=r"\[b, joints, 3\]"):
        LimbLengthError()(p, g[:1])
    with pytest.raises(CapfError, match=r"\[\.\.\., joints, 3\]"):
        limb_length_loss(p[..., :2], g[..., :2])
    with pytest.raises(CapfError, match="differ in shape"):
        UNCERTAINTY(sig, p, g[:1])
    # a limb index out of range (the 17-joint table on 16 joints; an explicit table)
    with pytest.raises(CapfError, match=r"outside \[0, 16\)"):
        LimbLengthError()(p[:, :16].numpy(), g[:, :16].numpy())
    with pytest.raises(CapfError, match=r"outside \[0, 17\)"):
        limb_length_loss(p, g, limbs=[(0, 1), (3, 17)])
    with pytest.raises(CapfError, match="1..64 pairs"):
        limb_length_loss(p, g, limbs=[])
    # K of 0 and of 9, a sigma of another width
    with pytest.raises(CapfError, match="1..8 sigma"):
        UNCERTAINTY([], p, g)
    with pytest.raises(CapfError, match="1..8 sigma"):
        UNCERTAINTY([sig[0]] * 9, p, g)
    with pytest.raises(CapfError, match="sigma 1 must be"):
        UNCERTAINTY([sig[0], torch.full((2, 17, 2), 0.3)], p, g)
    with pytest.raises(CapfError, match="sigma 0 must be"):
        UNCERTAINTY([torch.full((17, 3), 0.3)], p, g)          # the reference would broadcast it; one sigma per row is what the kernel takes


def test_binding_wrappers_refuse_before_they_touch_a_device():
    from capf import lib as capf
    p, g = torch.zeros(4, 17, 3), torch.ones(4, 17, 3)
    with pytest.raises(capf.CapfError, match="validity must be"):
        capf.keypoints_l2_loss(p, g, torch.ones(4, 16, 1))
    with pytest.raises(capf.CapfError, match="MI355X only"):
        capf.keypoints_l2_loss(p, g, torch.ones(4, 17, 1))
    with pytest.raises(capf.CapfError, match=r"outside \[0, 17\)"):
        capf.limb_length_errors(p, g, [(0, 17)])
    with pytest.raises(capf.CapfError, match="MI355X only"):
        capf.limb_length_errors(p, g, lc.CONNECTIVITY)
    with pytest.raises(capf.CapfError, match="segment table"):
        capf.limb_length_sums(torch.zeros(4, 16), None, n_segments=3)
    with pytest.raises(capf.CapfError, match="MI355X only"):
        capf.limb_length_sums(torch.zeros(4, 16))
    with pytest.raises(capf.CapfError, match="1..8 sigma"):
        capf.uncertainty_loss(p, g, [])
    with pytest.raises(capf.CapfError, match="sigma 0 must be"):
        capf.uncertainty_loss(p, g, [torch.ones(4, 17, 2)])
    with pytest.raises(capf.CapfError, match="one entry per sigma"):
        capf.uncertainty_loss(p, g, [torch.ones(4, 17, 1)], want_dsigma=[True, False])
    table, L = capf.limb_table(lc.CONNECTIVITY, 17)
    assert L == 16 and list(table) == [v for pair in lc.CONNECTIVITY for v in pair]
