"""CPU: the interface of the keypoint head on a flip-test pair -- the two C entries (declared, exported, bound, inside ABI revision 12,
documented), every refusal the header lists (none needs a device: each returns before anything is launched, with pointers that are
never dereferenced -- only `swap`, a HOST table, is real), the binding's table, and the host refusals of the two model methods."""
import contextlib
import copy
import io
import os
import re

import pytest
import torch

import kp_head_cases as K  # noqa: F401  (the cases and bounds of the GPU files; imported here so that a broken yardstick fails on the CPU too)
from capf import lib as capf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"capf_kp_head_pair_scratch_bytes", "capf_kp_head_forward_pair"}
INVALID = -1
P = 0x10000        # a well-aligned non-NULL "pointer": every call below is refused before anything could read it
H36M = (capf.c_int32 * 17)(*capf.H36M_SWAP)


def test_entries_declared_exported_bound_and_documented():
    lib = capf.load_library()
    assert lib.capf_abi_version() == 12 == capf.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "capf.h")).read()
    assert re.search(r"#define CAPF_ABI_VERSION 12\b", header)
    declared = set(re.findall(r"^[a-z][\w \*]*?\b(capf_\w+)\(", header, re.M))
    assert ENTRIES <= declared and ENTRIES <= set(capf.EXPORTS) and declared == set(capf.EXPORTS)
    for s in ENTRIES:
        assert hasattr(lib, s), s
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert all(f"`{s}`" in doc for s in ENTRIES)
    for word in ("zf = 0.5f * (zo + zm)", "W - 1 - xs", "swap[j]", "mirror_width", "summation orders are unchanged", "its own inverse"):
        assert word in header, word
    assert callable(capf.kp_head_forward_pair)
    # the binding's table is the one the H36M entries apply (csrc/preprocess.hip, mvn/datasets/utils.py) and its own inverse
    from mvn.datasets.utils import joints_left, joints_right
    want = list(range(17))
    for l, r in zip(joints_left, joints_right):
        want[l], want[r] = r, l
    assert list(capf.H36M_SWAP) == want and all(capf.H36M_SWAP[capf.H36M_SWAP[j]] == j for j in range(17))


def test_scratch_bytes():
    lib = capf.load_library()
    assert lib.capf_kp_head_pair_scratch_bytes(2, 64, 64, 32, 17) > 0
    # sized by the SOURCE frames: the single entry's scratch at Bsrc, linear in Bsrc (the tiling is a function of H * W alone)
    assert lib.capf_kp_head_pair_scratch_bytes(2, 64, 48, 32, 17) == lib.capf_kp_head_scratch_bytes(2, 64, 48, 32, 17, 0)
    assert lib.capf_kp_head_pair_scratch_bytes(6, 64, 48, 32, 17) == 3 * lib.capf_kp_head_pair_scratch_bytes(2, 64, 48, 32, 17)
    for bad in ((0, 8, 8, 32, 17), (2, 0, 8, 32, 17), (2, 8, 0, 32, 17), (2, 8, 8, 30, 17), (2, 8, 8, 516, 17), (2, 8, 8, 0, 17),
                (2, 8, 8, 32, 0), (2, 8, 8, 32, 33), ((1 << 30) + 1, 1, 1, 32, 17)):
        assert lib.capf_kp_head_pair_scratch_bytes(*bad) == 0, bad


def _args(**kw):
    a = dict(stream=None, map=P, dtype=capf.F32, weight=P, bias=P, B=2, H=8, W=8, C=32, J=17, mode=0, beta=1.0, swap=H36M, shift=1,
             decode=(capf.c_float * 4)(1, 0, 1, 0), to_image=None, mirror_width=192.0, kcrop2=P, k2d2=None, score=None, heat=None, scratch=P,
             nbytes=1 << 30)
    a.update(kw)
    return list(a.values())


def _table(*entries):
    return (capf.c_int32 * len(entries))(*entries)


NOT_INVOLUTIVE = list(range(17))
NOT_INVOLUTIVE[1:4] = [2, 3, 1]            # a permutation (a 3-cycle), but not its own inverse
REPEATED = list(range(17))
REPEATED[5] = 4                            # not a permutation at all
REFUSALS = [
    ("NULL map", dict(map=None)), ("NULL weight", dict(weight=None)), ("NULL decode", dict(decode=None)), ("NULL swap", dict(swap=None)),
    ("NULL kcrop2", dict(kcrop2=None)), ("NULL scratch", dict(scratch=None)), ("k2d2 without to_image", dict(k2d2=P, to_image=None)),
    ("Bsrc = 0", dict(B=0)), ("Bsrc > 2^30", dict(B=(1 << 30) + 1, H=1, W=1)), ("H = 0", dict(H=0)), ("W = -1", dict(W=-1)), ("J = 0", dict(J=0)), ("J = 33", dict(J=33)),
    ("C = 30", dict(C=30)), ("C = 0", dict(C=0)), ("C = 516", dict(C=516)),
    ("beta = 0", dict(beta=0.0)), ("beta < 0", dict(beta=-1.0)), ("beta = inf", dict(beta=float("inf"))), ("beta = NaN", dict(beta=float("nan"))),
    ("mirror_width = inf", dict(mirror_width=float("inf"))), ("mirror_width = NaN", dict(mirror_width=float("nan"))),
    ("shift 2", dict(shift=2)), ("shift -1", dict(shift=-1)),
    ("mode 2", dict(mode=2)), ("mode -1", dict(mode=-1)), ("dtype 3", dict(dtype=3)), ("dtype -1", dict(dtype=-1)),
    ("misaligned map", dict(map=P + 4)), ("misaligned 16-bit map", dict(map=P + 4, dtype=capf.F16)),
    ("scratch too small", dict(nbytes=16)),
    ("swap entry = J", dict(swap=_table(*([17] + list(range(1, 17)))))), ("swap entry < 0", dict(swap=_table(*([-1] + list(range(1, 17)))))),
    ("swap not involutive", dict(swap=_table(*NOT_INVOLUTIVE))), ("swap repeats a joint", dict(swap=_table(*REPEATED))),
    ("swap of J = 1 out of range", dict(J=1, swap=_table(1))),
]


@pytest.mark.parametrize("why,kw", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_need_no_device(why, kw):
    assert capf.load_library().capf_kp_head_forward_pair(*_args(**kw)) == INVALID, why


def test_scratch_of_the_pair_is_enough_and_one_byte_less_is_not():
    """the last refusal before the swap table is read: with exactly the stated scratch a bad table is still INVALID, and so is a good
    table with one byte less (nothing else distinguishes the two calls)"""
    lib = capf.load_library()
    need = lib.capf_kp_head_pair_scratch_bytes(2, 8, 8, 32, 17)
    assert lib.capf_kp_head_forward_pair(*_args(nbytes=need - 1)) == INVALID
    assert lib.capf_kp_head_forward_pair(*_args(nbytes=need, swap=_table(*NOT_INVOLUTIVE))) == INVALID


# ---- the binding and the model methods: host refusals ----------------------------------------------------------------------------------
def _model(**kw):
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    with contextlib.redirect_stdout(io.StringIO()):
        return CA_PF(backbone_preset(copy.deepcopy(config), "hrnet_32"), **kw)


def _mpi_model(**kw):
    from model.conpose import VolumetricTriangulationNet, mpi_preset
    from mvn.utils.cfg import config
    with contextlib.redirect_stdout(io.StringIO()):
        return VolumetricTriangulationNet(mpi_preset(copy.deepcopy(config), "hrnet_32"), **kw)


def test_binding_refuses_on_the_host():
    w = torch.zeros(17, 32)
    with pytest.raises(capf.CapfError, match="2 \\* Bsrc frames"):
        capf.kp_head_forward_pair(torch.zeros(3, 4, 4, 32), w)
    with pytest.raises(capf.CapfError, match="H36M table"):
        capf.kp_head_forward_pair(torch.zeros(2, 4, 4, 32), torch.zeros(16, 32))
    with pytest.raises(capf.CapfError, match="swap has 3 entries"):
        capf.kp_head_forward_pair(torch.zeros(2, 4, 4, 32), w, swap=(0, 2, 1))
    with pytest.raises(capf.CapfError, match="to_image"):
        capf.kp_head_forward_pair(torch.zeros(4, 4, 4, 32), w, to_image=torch.zeros(4, 2, 3))        # [Bsrc, 2, 3], not [2 Bsrc, 2, 3]
    with pytest.raises(capf.CapfError, match="NHWC map"):
        capf.kp_head_forward_pair(torch.zeros(2, 4, 4, 32, dtype=torch.float64), w)


def test_model_methods_refuse_instead_of_computing_something_else():
    x, x5, A = torch.zeros(2, 64, 64, 3), torch.zeros(2, 2, 64, 64, 3), torch.zeros(2, 2, 3)
    for make in (_model, _mpi_model):
        m = make()
        with pytest.raises(capf.CapfError, match="no keypoint head"):
            m.detect_flip_test(x)
        with pytest.raises(capf.CapfError, match="no keypoint head"):
            m.forward_detect_flip_test(x, A)
    m = _model(keypoint_head="argmax")
    with pytest.raises(ValueError, match="to_image"):
        m.forward_detect_flip_test(x, None)
    with pytest.raises(TypeError, match="float32 or uint8"):
        m.detect_flip_test(x.double())
    with pytest.raises(TypeError, match="float32 \\[2,B,H,W,3\\] stack"):
        m.detect_flip_test(x5.to(torch.uint8))
    with pytest.raises(TypeError, match="float32 \\[2,B,H,W,3\\] stack"):
        m.detect_flip_test(torch.zeros(3, 2, 64, 64, 3))
    # (shapes and devices are judged behind the device check, as in detect: tests/test_gpu_kp_head_pair_model.py)
    for bad in ((0, 2, 1), [17] + list(range(1, 17)), list(NOT_INVOLUTIVE), list(REPEATED)):
        with pytest.raises(ValueError, match="flip_pairs"):
            m.detect_flip_test(x, flip_pairs=bad)
    # everything host-side accepted: the call stops at the device check (CPU tensors), for each of the three image forms
    for images in (x, x5, x.to(torch.uint8)):
        for table in (None, capf.H36M_SWAP, list(capf.MPI_SWAP)):
            with pytest.raises(capf.CapfError, match="MI355X only"):
                m.forward_detect_flip_test(images, A, flip_pairs=table)
    # grad mode does not matter: an argmax head with trainable parameters is refused by forward_detect under grad, not here
    assert torch.is_grad_enabled() and m.keypoint_head.final_layer.weight.requires_grad
    # a batch-statistics backbone in train mode: the 2B-frame pair would change the statistics
    m = _model(keypoint_head="integral", backbone_bn="batch")
    m.train()
    with pytest.raises(NotImplementedError, match="backbone.eval\\(\\)"):
        m.detect_flip_test(x)
    with pytest.raises(NotImplementedError, match="backbone.eval\\(\\)"):
        m.forward_detect_flip_test(x5, A)
    m.backbone.eval()
    with pytest.raises(capf.CapfError, match="MI355X only"):
        m.detect_flip_test(x)
