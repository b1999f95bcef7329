"""CPU: gradients w.r.t. the keypoints (capf_backward_points, CA_PF's keypoint arguments under autograd) -- what can be checked without a GPU.

  * the entry is declared, exported and bound, inside ABI revision 12;
  * its argument, dtype and state checks on plan-only handles;
  * the host's refusals (a 16-bit model cannot return keypoint gradients and says so instead of dropping them);
  * the yardstick of the GPU tests (test_gpu_points_grad.py) checks itself: capf_oracle.lifter_forward in float64 with k2d and ref as
    leaves against central differences of the loss, and the margin rule of points_grad_cases on every case's reference points."""
import copy
import ctypes
import os
import re
import subprocess

import pytest
import torch

from conftest import ROOT, make_model
from feature_cases import HRNET32_128x96
from points_grad_cases import (HRNET32_32x32, MARGIN_PX, case_inputs, margin_px, normalise, off_map_, points64, small_inputs, tame_)

INVALID, UNSUPPORTED, STATE = -1, -2, -4          # include/capf.h: CAPF_ERR_*
FAKE = ctypes.c_void_p(0x1000)                    # a non-NULL pointer that is never dereferenced: every check below fails before a launch
ENTRY = "capf_backward_points"


def _plan(dtype="fp32"):
    from capf.lib import Engine
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), "hrnet_32")
    return Engine(_native.make_capf_config(cfg, 128, 96, compute_dtype=dtype), device=None)


def _four(value=0x1000):
    return (ctypes.c_void_p * 4)(*([value] * 4))


# ---- the entry exists, everywhere it has to -------------------------------------------------------------------------------------------
def test_the_entry_is_declared_exported_and_bound_in_revision_12():
    import capf
    from capf.lib import EXPORTS
    header = open(os.path.join(ROOT, "include", "capf.h")).read()
    assert re.search(r"^int capf_backward_points\(capf_handle\* h, void\* stream, const float\* grad_out, int batch, float\* flat_grad, "
                     r"const float\* drop_masks,\s*float\* const dfeat_nhwc\[4\], float\* dk2d, float\* dref\);", header, re.M)
    assert re.search(r"#define CAPF_ABI_VERSION 12\b", header)
    assert ENTRY in EXPORTS and EXPORTS.count(ENTRY) == 1
    lib = capf.load_library()
    assert hasattr(lib, ENTRY)
    assert lib.capf_abi_version() == 12
    so = os.path.join(ROOT, "contextaware-poseformer_amd", "capf", "libcapf.so")
    dyn = subprocess.run(["nm", "-D", "--defined-only", so], check=True, capture_output=True, text=True).stdout.split()
    assert ENTRY in dyn
    table = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`" + ENTRY + "`" in table


# ---- argument, dtype and state checks on plan-only handles ----------------------------------------------------------------------------
def test_null_arguments_are_invalid_and_leave_the_message_alone():
    eng = _plan()
    lib = eng.lib
    before = lib.capf_last_error(eng.h)
    holes = _four()
    holes[1] = None
    for rc in (lib.capf_backward_points(None, None, FAKE, 2, FAKE, None, None, FAKE, FAKE),
               lib.capf_backward_points(eng.h, None, None, 2, FAKE, None, None, FAKE, FAKE),
               lib.capf_backward_points(eng.h, None, FAKE, 2, None, None, None, FAKE, FAKE),
               lib.capf_backward_points(eng.h, None, FAKE, 0, FAKE, None, None, FAKE, FAKE),
               lib.capf_backward_points(eng.h, None, FAKE, 2, FAKE, None, holes, FAKE, FAKE)):
        assert rc == INVALID
        assert lib.capf_last_error(eng.h) == before
    assert lib.capf_backward_points(eng.h, None, FAKE, 2, FAKE, None, _four(0x1004), FAKE, FAKE) == INVALID      # 16-byte alignment, as capf_backward_maps
    assert ENTRY in lib.capf_last_error(eng.h).decode()
    eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_16_bit_handles_are_refused_with_the_entry_and_the_dtype(dtype):
    eng = _plan(dtype)
    for dfeat, dk2d, dref in ((None, FAKE, FAKE), (_four(), None, None), (None, None, None)):
        assert eng.lib.capf_backward_points(eng.h, None, FAKE, 2, FAKE, None, dfeat, dk2d, dref) == UNSUPPORTED
        reason = eng.lib.capf_last_error(eng.h).decode()
        assert reason.startswith(ENTRY + ":") and "fp32" in reason and reason.endswith(dtype), reason
    eng.close()


def test_a_handle_without_a_saved_step_reports_state():
    eng = _plan()
    lib = eng.lib
    gen = lib.capf_train_generation(eng.h)
    assert lib.capf_backward(eng.h, None, FAKE, 2, FAKE, None) == STATE
    want = lib.capf_last_error(eng.h)
    for dfeat, dk2d, dref in ((None, FAKE, FAKE), (_four(), FAKE, None), (None, None, None)):
        assert lib.capf_backward_points(eng.h, None, FAKE, 2, FAKE, None, dfeat, dk2d, dref) == STATE
        assert lib.capf_last_error(eng.h) == want             # capf_backward's rule and capf_backward's words
    assert lib.capf_train_generation(eng.h) == gen
    eng.close()


# ---- the host's refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("which", ["k2d", "kcrop"])
def test_a_16_bit_model_refuses_keypoints_that_require_grad(dtype, which):
    from feature_cases import synth_maps
    model, _ = make_model("hrnet_32", compute_dtype=dtype)
    k2d, kc = torch.zeros(2, 17, 2), torch.full((2, 17, 2), 50.0)
    (k2d if which == "k2d" else kc).requires_grad_(True)
    img = torch.zeros(2, 128, 96, 3)
    for call in (lambda: model(img, k2d, kc),
                 lambda: model.forward_u8(torch.zeros(2, 128, 96, 3, dtype=torch.uint8), k2d, kc),
                 lambda: model.forward_features(synth_maps(2, HRNET32_128x96, 1), k2d, kc)):
        with pytest.raises(NotImplementedError, match="fp32"):
            call()
    assert torch.equal(kc.detach(), torch.full((2, 17, 2), 50.0))
    with torch.no_grad():                                     # nothing to drop without a graph: the usual refusal of CPU tensors
        from capf.lib import CapfError
        with pytest.raises(CapfError, match="no CPU fallback"):
            model(img, k2d, kc)


def test_an_fp32_model_gets_past_the_keypoint_check_to_the_device_check():
    from capf.lib import CapfError
    model, _ = make_model("hrnet_32")
    k2d, kc = torch.zeros(2, 17, 2, requires_grad=True), torch.full((2, 17, 2), 50.0, requires_grad=True)
    with pytest.raises(CapfError, match="no CPU fallback"):
        model(torch.zeros(2, 128, 96, 3), k2d, kc)
    assert torch.equal(kc.detach(), torch.full((2, 17, 2), 50.0))


# ---- the yardstick checks itself -------------------------------------------------------------------------------------------------------
def test_every_case_keeps_its_reference_points_off_the_cell_boundaries():
    for B in (1, 2, 3, 6):
        _, _, kc, ref, _ = case_inputs(B)
        assert torch.equal(normalise(kc), ref)
        m = margin_px(ref)
        print(f"  128 x 96, B = {B}: nearest cell boundary {m:.2e} px")
        assert m >= MARGIN_PX, (B, m)
    m = margin_px(normalise(off_map_(case_inputs(1)[2].clone())))
    print(f"  128 x 96, the hand-made frame: {m:.2e} px")
    assert m >= MARGIN_PX, m
    m = margin_px(normalise(off_map_(case_inputs(3)[2].clone())))
    assert m >= MARGIN_PX, m
    for B in (1, 3):
        m = margin_px(small_inputs(B)[3], HRNET32_32x32)
        print(f"  32 x 32, B = {B}: {m:.2e} px")
        assert m >= MARGIN_PX, (B, m)


def test_the_float64_yardstick_equals_central_differences_of_the_loss():
    """Step 1e-6 in float64: truncation ~ h^2 |L'''| and roundoff ~ 1e-16 |L| / h ~ 1e-10 are both far below 1e-6 of a gradient entry of
    1e-3 .. 1e-1; a coordinate next to a cell boundary of a DEFORMABLE sample (pos = tanh(offset) + ref, no margin rule) would show as an
    error of order 1, not 1e-6."""
    import capf_oracle as oracle
    torch.set_num_threads(min(16, torch.get_num_threads()))
    _, sd = make_model("hrnet_32", wseed=43)
    P = tame_({k: v.clone() for k, v in sd.items() if k.startswith("volume_net.")})
    maps, k2d, _, ref, gt = case_inputs(2)
    _, dk2d, dref, _, loss = points64(P, k2d, ref, gt, maps)
    assert dk2d.abs().max() > 0 and dref.abs().max() > 0
    P64 = {k: v.double() for k, v in P.items()}
    f64 = [m.double() for m in maps]

    def loss_at(k, r):
        with torch.no_grad():
            return oracle.mpjpe(oracle.lifter_forward(P64, k, r, f64), gt.double()).item()

    h = 1e-6
    for name, grad, at in (("ref", dref, (0, 3, 0)), ("ref", dref, (1, 11, 1)), ("k2d", dk2d, (1, 5, 0))):
        k, r = k2d.double().clone(), ref.double().clone()
        t = r if name == "ref" else k
        t[at] += h
        up = loss_at(k, r)
        t[at] -= 2 * h
        down = loss_at(k, r)
        fd, an = (up - down) / (2 * h), grad[at].item()
        print(f"  d loss / d {name}{list(at)}: autograd {an:+.9e}, central difference {fd:+.9e}  (loss {loss:.6f})")
        assert abs(fd - an) <= 1e-6 * abs(an) + 1e-9, (name, at, fd, an)
