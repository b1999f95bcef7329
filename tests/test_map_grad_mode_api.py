"""CPU: the summation mode of the map gradient (capf_set_map_grad_mode / capf_map_grad_mode, CA_PF.map_grad_mode) -- what can be checked
without a GPU: the symbols, the state change on plan-only handles, its refusals, that it costs no workspace, and how CA_PF's attribute
resolves (tests/test_gpu_map_grad_ordered.py runs the ordered kernels)."""
import copy
import os
import re
import subprocess

import pytest
import torch

from capf.lib import EXPORTS, CapfError, Engine, load_library

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("capf_set_map_grad_mode", "capf_map_grad_mode")


def _plan(dtype="fp32", backbone="hrnet_32", hw=(128, 96)):
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), backbone)
    return Engine(_native.make_capf_config(cfg, hw[0], hw[1], compute_dtype=dtype), device=None)


def test_both_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "capf.h")).read()
    assert re.search(r"^int capf_set_map_grad_mode\(capf_handle\* h, int mode\);$", header, re.M)
    assert re.search(r"^int capf_map_grad_mode\(const capf_handle\* h\);$", header, re.M)
    assert re.search(r"^#define CAPF_ABI_VERSION 12$", header, re.M)          # additive inside revision 12
    lib = load_library()
    table = subprocess.run(["nm", "-D", "--defined-only", lib._name], check=True, capture_output=True, text=True).stdout
    exported = {line.split()[-1] for line in table.splitlines() if line.strip()}
    for name in SYMBOLS:
        assert name in EXPORTS and name in exported and hasattr(lib, name), name


def test_mode_is_a_state_change_on_a_plan_only_handle():
    eng = _plan()
    assert eng.map_grad_mode() == 0                                           # the default is the atomic route
    eng.set_map_grad_mode(1)
    assert eng.map_grad_mode() == 1
    for bad in (2, -1):
        with pytest.raises(CapfError, match=r"\(-1\)"):                       # CAPF_ERR_INVALID
            eng.set_map_grad_mode(bad)
        assert eng.map_grad_mode() == 1                                       # (a refused call changes nothing)
    eng.set_map_grad_mode(0)
    assert eng.map_grad_mode() == 0
    assert eng.lib.capf_set_map_grad_mode(None, 1) == -1 and eng.lib.capf_map_grad_mode(None) == -1
    eng.close()


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_a_16_bit_plan_refuses_the_ordered_mode_with_the_fp32_only_reason(dtype):
    eng = _plan(dtype)
    with pytest.raises(CapfError, match=r"\(-2\).*fp32 only.*" + dtype):      # CAPF_ERR_UNSUPPORTED, maps_f32_only's text
        eng.set_map_grad_mode(1)
    assert eng.map_grad_mode() == 0
    eng.close()


@pytest.mark.parametrize("backbone,hw", [("hrnet_32", (128, 96)), ("hrnet_48", (256, 192)), ("cpn", (256, 192))])
def test_the_ordered_mode_needs_no_workspace(backbone, hw):
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    cfg = _native.make_capf_config(backbone_preset(copy.deepcopy(config), backbone), hw[0], hw[1])
    cfg.training = 1
    eng = Engine(cfg, device=None)
    sizes = {}
    for mode in (0, 1, 0):
        eng.set_map_grad_mode(mode)
        got = [eng.workspace_bytes(B) for B in (1, 64, 512)]
        assert all(n > 0 for n in got)
        assert sizes.setdefault("bytes", got) == got, (mode, got)
    eng.close()


def test_ca_pf_attribute_resolves_through_one_helper():
    from mvn.models.conpose import CA_PF, resolve_map_grad_mode
    assert resolve_map_grad_mode("atomic") == 0 and resolve_map_grad_mode("ordered") == 1
    for bad in ("sorted", "", 1, True):
        with pytest.raises(ValueError, match="map_grad_mode"):
            resolve_map_grad_mode(bad)
    before = torch.are_deterministic_algorithms_enabled()
    try:
        torch.use_deterministic_algorithms(False)
        assert resolve_map_grad_mode(None) == 0
        torch.use_deterministic_algorithms(True)
        assert resolve_map_grad_mode(None) == 1                               # the torch switch selects the deterministic form
        assert resolve_map_grad_mode("atomic") == 0                           # an explicit choice wins
    finally:
        torch.use_deterministic_algorithms(before)
    import inspect
    assert "self.map_grad_mode = None" in inspect.getsource(CA_PF.__init__)


def test_forward_features_refuses_an_unknown_mode_before_it_touches_a_device():
    from conftest import make_model
    from feature_cases import HRNET32_128x96, synth_maps
    model, _ = make_model("hrnet_32", wseed=5, bn="random")
    assert model.map_grad_mode is None
    model.map_grad_mode = "sorted"
    with pytest.raises(ValueError, match="map_grad_mode.*'sorted'"):
        model.forward_features(synth_maps(2, HRNET32_128x96, 6), torch.zeros(2, 17, 2), torch.zeros(2, 17, 2))


def test_the_variant_without_context_blocks_inherits_the_attribute():
    from model.conpose import VolumetricTriangulationNet
    from mvn.models.conpose import CA_PF
    assert issubclass(VolumetricTriangulationNet, CA_PF)
    assert "map_grad_mode" not in vars(VolumetricTriangulationNet)            # one attribute, CA_PF's
