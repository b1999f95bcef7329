"""CPU: the forward from uint8 crops (capf_forward_u8 and its siblings) as far as it can be held without a GPU -- the host copy of the
normalisation rule, the ABI surface, the argument checks that come before any launch, and the routing promise: the uint8 stem op runs
the ",u8" form of exactly the kernel the float stem op runs at the same shape, batch and dtype.  The kernels themselves:
tests/test_gpu_u8_input.py."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

from conftest import ROOT

HRNET_MEAN, HRNET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)          # ContextPose/mvn/datasets/utils.py:24-26
CPN_MEAN_255 = (122.7717, 115.9465, 102.9801)                                  # :27-29, divided by 255 in fp32
STATE, INVALID = -4, -1                                                         # include/capf.h :: CAPF_ERR_STATE, CAPF_ERR_INVALID

NEW = ["capf_forward_u8", "capf_backbone_forward_u8", "capf_forward_train_u8", "capf_preprocess_points", "capf_input_rule_host",
       "capf_op_conv_u8", "capf_op_conv_u8_kernel_name", "capf_op_conv_stem_kernel_name"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_error_codes_are_the_headers():
    text = open(os.path.join(ROOT, "include", "capf.h")).read()
    for name, value in (("CAPF_ERR_STATE", STATE), ("CAPF_ERR_INVALID", INVALID)):
        m = re.search(name + r"\s*=\s*(-?\d+)", text)
        assert m and int(m.group(1)) == value, name


@pytest.mark.parametrize("channel", [0, 1, 2])
def test_host_rule_is_the_fp32_expression_hrnet(channel):
    """all 256 byte values: (fp32(u) * fp32(1/255) - mean) / std, every step one rounded fp32 operation"""
    from capf import lib
    u = np.arange(256, dtype=np.uint8)
    got = lib.input_rule_host(u, channel, HRNET_MEAN, HRNET_STD)
    want = (u.astype(np.float32) * np.float32(1.0 / 255.0) - np.float32(HRNET_MEAN[channel])) / np.float32(HRNET_STD[channel])
    assert want.dtype == np.float32 and got.dtype == np.float32
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("channel", [0, 1, 2])
def test_host_rule_is_the_fp32_expression_cpn_mean_only(channel):
    from capf import lib
    mean = (np.array(CPN_MEAN_255, dtype=np.float32) / np.float32(255.0)).astype(np.float32)
    u = np.arange(256, dtype=np.uint8)
    got = lib.input_rule_host(u, channel, mean, None)
    want = u.astype(np.float32) * np.float32(1.0 / 255.0) - mean[channel]
    assert np.array_equal(_bits(got), _bits(want))
    # ... and the constants the host package hands the engine are those (capf.lib.preprocess's)
    m3, s3 = lib.input_constants("cpn")
    assert s3 is None and np.array_equal(_bits(np.array(list(m3), dtype=np.float32)), _bits(mean))
    m3, s3 = lib.input_constants("hrnet_32")
    assert np.array_equal(_bits(list(m3)), _bits(HRNET_MEAN)) and np.array_equal(_bits(list(s3)), _bits(HRNET_STD))


def test_host_rule_rejects_bad_arguments():
    from capf import lib
    L = lib.load_library()
    u = (ctypes.c_uint8 * 4)(0, 1, 2, 255)
    out = (ctypes.c_float * 4)()
    m3 = (ctypes.c_float * 3)(*HRNET_MEAN)
    assert L.capf_input_rule_host(u, 4, 3, m3, None, out) == INVALID
    assert L.capf_input_rule_host(u, 4, -1, m3, None, out) == INVALID
    assert L.capf_input_rule_host(None, 4, 0, m3, None, out) == INVALID
    assert L.capf_input_rule_host(u, 0, 0, m3, None, out) == 0


def test_new_entries_are_declared_bound_and_exported_inside_revision_12():
    from capf import lib
    text = open(os.path.join(ROOT, "include", "capf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(capf_[a-z_0-9]+)\s*\(", code))
    L = lib.load_library()
    for name in NEW:
        assert name in declared, f"{name} is not declared in include/capf.h"
        assert name in lib.EXPORTS, f"{name} is not in capf.lib.EXPORTS"
        assert hasattr(L, name), f"libcapf.so does not export {name}"
        assert getattr(L, name).argtypes is not None, f"{name} has no binding"
    assert re.search(r"#define\s+CAPF_ABI_VERSION\s+12\b", text)
    assert L.capf_abi_version() == 12 and lib.ABI_VERSION == 12
    assert L.capf_version() == b"capf 0.12 (gfx950)"
    assert "datasets/utils.py:45-50, 55-56, 67-68" in text
    for m in ("forward_u8", "backbone_forward_u8", "forward_train_u8"):
        assert callable(getattr(lib.Engine, m))
    for f in ("preprocess_points", "op_conv_u8", "input_rule_host"):
        assert callable(getattr(lib, f))


def _plan_only(training=0):
    import copy
    from capf import Engine
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    c = backbone_preset(copy.deepcopy(config), "hrnet_32")
    c.model.backbone.fix_weights = True
    cfg = _native.make_capf_config(c, 64, 64)
    cfg.training = training
    return Engine(cfg, device=None)


def test_return_codes_on_a_plan_only_handle():
    """the argument checks come first, then check_run's (a plan-only handle: CAPF_ERR_STATE); no pointer is read through"""
    from capf import lib
    eng = _plan_only()
    L, P = eng.lib, ctypes.c_void_p
    dummy = P(4096)
    m3, s3 = lib.input_constants("hrnet_32")
    fwd = lambda mode, batch: L.capf_forward_u8(eng.h, P(0), dummy, m3, s3, mode, dummy, dummy, batch, dummy)
    assert fwd(0, 2) == STATE and b"plan-only" in L.capf_last_error(eng.h)
    assert fwd(1, 3) == STATE and fwd(2, 4) == STATE
    assert fwd(3, 2) == INVALID and fwd(-1, 2) == INVALID
    assert fwd(2, 3) == INVALID and b"even" in L.capf_last_error(eng.h)
    assert L.capf_forward_u8(eng.h, P(0), None, m3, s3, 0, dummy, dummy, 2, dummy) == INVALID
    assert L.capf_forward_u8(eng.h, P(0), dummy, None, s3, 0, dummy, dummy, 2, dummy) == INVALID
    assert L.capf_forward_u8(eng.h, P(0), dummy, m3, None, 0, dummy, dummy, 2, dummy) == STATE      # std3 == NULL is the mean-only form
    bb = lambda mode, batch: L.capf_backbone_forward_u8(eng.h, P(0), dummy, m3, s3, mode, batch)
    assert bb(0, 2) == STATE and bb(5, 2) == INVALID and bb(2, 5) == INVALID
    tr = lambda mode, batch: L.capf_forward_train_u8(eng.h, P(0), dummy, m3, s3, mode, dummy, dummy, batch, dummy, None)
    assert tr(0, 2) == STATE and b"training = 0" in L.capf_last_error(eng.h)     # an inference handle, like capf_forward_train
    eng.close()
    eng = _plan_only(training=1)
    tr = lambda mode, batch: eng.lib.capf_forward_train_u8(eng.h, P(0), dummy, m3, s3, mode, dummy, dummy, batch, dummy, None)
    assert tr(1, 2) == STATE and tr(4, 2) == INVALID and tr(2, 7) == INVALID
    eng.close()


def test_standalone_entries_reject_bad_arguments_before_any_launch():
    from capf import lib
    L, P = lib.load_library(), ctypes.c_void_p
    dummy = P(4096)
    m3, s3 = lib.input_constants("hrnet_32")
    conv = lambda img, mode, dtype, Bsrc=2: L.capf_op_conv_u8(P(0), img, dummy, dummy, dummy, Bsrc, mode, 8, 8, 64, 3, 2, 1, m3, s3, dtype)
    assert conv(None, 0, 0) == INVALID and conv(dummy, 3, 0) == INVALID and conv(dummy, 0, 7) == INVALID and conv(dummy, 0, 0, Bsrc=0) == INVALID
    pts = lambda mode, batch, k=dummy: L.capf_preprocess_points(P(0), batch, mode, None, None, k, dummy, dummy, dummy)
    assert pts(3, 2) == INVALID and pts(0, 0) == INVALID and pts(0, 2, None) == INVALID
    assert L.capf_preprocess_points(P(0), 2, 0, dummy, None, dummy, dummy, dummy, dummy) == INVALID     # gt_in without gt_out
    assert lib.op_conv_u8_kernel_name(2, 3, 8, 8, 64, 3, 2) == "" and lib.stem_kernel_name(0, 8, 8, 64, 3, 2) == ""


# ---- routes ----------------------------------------------------------------------------------------------------------------------------
# (ks, Cout, H, W): fp32 ks 3 with Cout <= 64 (the streaming kernel) and Cout = 68 (past its one column tile), ks 7 (CPN), a 6 x 6 image
# whose Wo < 4 leaves the streaming kernels, and ks 5 -- no run-based kernel: the 16-bit element-wise gather
STEMS = [(3, 64, 256, 256), (3, 32, 64, 48), (3, 68, 256, 256), (7, 64, 384, 288), (3, 64, 6, 6), (7, 64, 6, 6), (5, 64, 33, 35)]
F32, BF16, F16 = 0, 1, 2


def route_cases():
    return [(dt, ks, co, H, W, B) for dt in (F32, BF16, F16) for ks, co, H, W in STEMS for B in (1, 64)]


@pytest.mark.parametrize("dtype,ks,cout,H,W,B", route_cases())
def test_u8_op_names_the_u8_form_of_the_float_ops_kernel(dtype, ks, cout, H, W, B):
    from capf import lib
    want = lib.stem_kernel_name(B, H, W, cout, ks, 2, dtype)
    assert want.endswith(">") and "u8" not in want
    got_u8 = []
    for mode, bsrc in ((0, B), (1, B), (2, (B + 1) // 2)):
        frames = 2 * bsrc if mode == 2 else bsrc
        ref = lib.stem_kernel_name(frames, H, W, cout, ks, 2, dtype)
        got_u8.append(lib.op_conv_u8_kernel_name(bsrc, mode, H, W, cout, ks, 2, dtype))
        assert got_u8[-1] == ref[:-1] + ",u8>"
    # ... and both are, character for character, the names recorded before the stem got one route and one name function
    with open(os.path.join(ROOT, "tests", "golden", "stem_routes.json")) as f:
        recorded = json.load(f)[f"{dtype},{ks},{cout},{H},{W},{B}"]
    assert want == recorded["stem_kernel_name"] and got_u8 == recorded["op_conv_u8_kernel_name"]


def test_the_enumerated_routes_are_the_five_stem_kernels():
    """the table above reaches every Cin = 3 kernel: two fp32, three per 16-bit format"""
    from capf import lib
    names = {lib.stem_kernel_name(B, H, W, co, ks, 2, dt).split("<")[0] for dt, ks, co, H, W, B in route_cases()}
    assert names == {"igemm_f32_stem_stream", "igemm_f32_smallc", "igemm_bf16_stem_stream", "igemm_bf16_stem", "igemm_bf16_smallc",
                     "igemm_f16_stem_stream", "igemm_f16_stem", "igemm_f16_smallc"}
    assert lib.stem_kernel_name(64, 256, 256, 64, 3, 2, F32) == "igemm_f32_stem_stream<w4,64x64>"
    assert lib.op_conv_u8_kernel_name(64, 0, 256, 256, 64, 3, 2, F32) == "igemm_f32_stem_stream<w4,64x64,u8>"


def test_the_plans_stem_op_is_the_op_the_standalone_query_describes():
    """the engine's stem op (capf_op_info) and the stand-alone float query agree, so the u8 query speaks for the plan's stem too"""
    import copy
    from capf import Engine, lib
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    for backbone, H, W, dtype, code, ks in (("hrnet_32", 64, 96, "fp32", F32, 3), ("hrnet_32", 64, 64, "bf16", BF16, 3),
                                            ("hrnet_32", 64, 64, "fp16", F16, 3), ("cpn", 64, 96, "fp32", F32, 7), ("cpn", 64, 96, "bf16", BF16, 7)):
        c = backbone_preset(copy.deepcopy(config), backbone)
        c.model.backbone.fix_weights = True
        eng = Engine(_native.make_capf_config(c, H, W, compute_dtype=dtype), device=None)
        for B in (1, 6):
            stem = eng.op_table(B)[0]
            assert stem[1] == lib.stem_kernel_name(B, H, W, 64, ks, 2, code), (backbone, dtype, B, stem)
        eng.close()
