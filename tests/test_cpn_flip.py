"""CPU: CPN's test-time flip -- the yardstick of the fold (tests/cpn_flip_oracle.py: its two restatements of cpn/test.py:62-70 agree bit for
bit; how many folded generated maps leave the peaks undecided), capf_cpn_decode_pair's refusals (none needs a device: each returns before
anything is launched, with pointers that are never dereferenced -- only `swap`, a HOST table, is real), header / exports / binding, the two
swap tables, and the host refusals of CA_PF.detect_cpn_flip / forward_detect_cpn_flip."""
import contextlib
import copy
import io
import os
import re

import numpy as np
import pytest
import torch

import cpn_decode_oracle as O
import cpn_flip_oracle as F
from capf import lib as capf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID, UNSUPPORTED = -1, -2          # include/capf.h :: CAPF_ERR_INVALID, CAPF_ERR_UNSUPPORTED
ENTRY = "capf_cpn_decode_pair"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_the_two_restatements_of_the_fold_agree(dtype):
    for si, (H, W) in enumerate(O.SHAPES):
        for Jn, C in O.JC:
            z2 = O.make_maps(4, H, W, C, Jn, seed=31 * si + Jn + C, dtype=dtype)
            for swap in ((capf.H36M_SWAP, capf.COCO_SWAP, F.involution(Jn)) if Jn == 17 else (F.involution(Jn), tuple(range(Jn)))):
                a, b = F.fold(z2, swap), F.fold_sequential(z2, swap)
                assert a.shape == (2, H, W, Jn) and a.dtype == np.float32
                assert np.array_equal(_bits(a), _bits(b)), (H, W, Jn, C, swap)
    # the identity table with a frame that is its own mirror image folds to the frame itself; and halving agrees down to the subnormals
    z = O.make_maps(1, 7, 5, 3, 3, seed=5, dtype=dtype)
    own = np.concatenate([z, z[:, :, ::-1, :]])
    assert np.array_equal(_bits(F.fold(own, (0, 1, 2))), _bits(z))
    tiny = np.full((2, 1, 2, 1), np.float32(1e-45))
    tiny[1] = np.float32(3e-45)
    assert np.array_equal(_bits(F.fold(tiny, (0,))), _bits(F.fold_sequential(tiny, (0,))))


def test_fold_indexing_by_hand():
    """one pixel in the mirror frame, joint 2 of 3 with swap (0)(1 2): it lands on joint 1, column W - 1 - x, halved"""
    z2 = np.zeros((2, 2, 4, 3), dtype=np.float32)
    z2[1, 1, 0, 2] = 6.0
    for f in (F.fold, F.fold_sequential):
        zf = f(z2, (0, 2, 1))
        want = np.zeros((1, 2, 4, 3), dtype=np.float32)
        want[0, 1, 3, 1] = 3.0
        assert np.array_equal(zf, want)
    assert F.pairs_of(capf.H36M_SWAP) == [(1, 4), (2, 5), (3, 6), (11, 14), (12, 15), (13, 16)]
    assert F.involution(1) == (0,) and F.involution(4) == (0, 2, 1, 3) and F.involution(5) == (0, 2, 1, 4, 3)


def test_stack_formulas_by_hand():
    kcrop = np.array([[[10.5, 3.0], [100.25, 7.0], [0.0, 9.0]]], dtype=np.float32)
    k2d = np.array([[[0.25, -0.5], [-0.125, 0.75], [0.0, 1.0]]], dtype=np.float32)
    kc2, k22 = F.mirrored_stacks(kcrop, k2d, (0, 2, 1), 192.0)
    assert np.array_equal(kc2[0], kcrop) and np.array_equal(k22[0], k2d)
    assert np.array_equal(kc2[1, 0], np.array([[180.5, 3.0], [191.0, 9.0], [90.75, 7.0]], dtype=np.float32))
    assert np.array_equal(k22[1, 0], np.array([[-0.25, -0.5], [-0.0, 1.0], [0.125, 0.75]], dtype=np.float32))
    assert F.mirrored_stacks(kcrop, None, (0, 2, 1))[1] is None


def test_folded_generated_maps_leave_few_cases_undecided():
    """The generator and the shapes of the GPU test, folded with the H36M table, fp32 and bf16 values: at most 2 % of the (frame, joint)
    cases outside the 1 x 1 maps may fail the decode oracle's `decided` (the cap of tests/test_cpn_detect.py; every 1 x 1 case is an exact
    tie by construction there, and stays one here: a fold of two 1 x 1 maps is a 1 x 1 map)."""
    bad = total = 0
    for H, W in O.SHAPES:
        for dtype in ("fp32", "bf16"):
            zf = F.fold(O.make_maps(6, H, W, 20, 17, seed=100 * H + W + 1, dtype=dtype), capf.H36M_SWAP)
            res = [O.decode(zf[b, :, :, j]) for b in range(3) for j in range(17)]
            u = sum(not r["decided"] for r in res)
            if (H, W) == (1, 1):
                assert u == len(res)
                continue
            print(f"{H} x {W} {dtype}: {u} of {len(res)} undecided")
            bad += u
            total += len(res)
    print(f"undecided after the fold: {bad} of {total} (frame, joint) cases")
    assert total == 612 and bad <= 0.02 * total, (bad, total)


def test_swap_tables_are_involutions():
    for tab in (capf.H36M_SWAP, capf.COCO_SWAP, capf.MPI_SWAP):
        assert len(tab) == 17 and sorted(tab) == list(range(17)) and all(tab[tab[j]] == j for j in range(17))
    assert capf.COCO_SWAP == (0, 2, 1, 4, 3, 6, 5, 8, 7, 10, 9, 12, 11, 14, 13, 16, 15)
    assert capf.COCO_SWAP != capf.H36M_SWAP


# ---- the C entry: declared, exported, bound, documented ------------------------------------------------------------------------------------
def test_entry_declared_exported_bound_and_documented():
    lib = capf.load_library()
    assert lib.capf_abi_version() == 12 == capf.ABI_VERSION
    header = open(os.path.join(ROOT, "include", "capf.h")).read()
    declared = set(re.findall(r"^[a-z][\w \*]*?\b(capf_\w+)\(", header, re.M))
    assert ENTRY in declared and capf.EXPORTS.count(ENTRY) == 1 and declared == set(capf.EXPORTS) and hasattr(lib, ENTRY)
    revisions = header[:header.index("#define CAPF_ABI_VERSION 12")]
    assert ENTRY in revisions                                            # the revision-12 list at the top
    for word in ("zf = 0.5f * (zo + zm)", "z[Bsrc + b, y, W - 1 - x, swap[j]]", "NO column shift", "test.py:62-70", "frames b and Bsrc + b alone",
                 "PARITY UNPINNED", "its own inverse", "mirror_width", "tools/bench_cpn_detect.py --pair"):
        assert word in header, word
    assert f"`{ENTRY}`" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert callable(capf.cpn_decode_pair)
    proto = re.search(r"^int capf_cpn_decode_pair\((.*?)\);", header, re.M | re.S).group(1)
    assert len(proto.split(",")) == 17 == len(lib.capf_cpn_decode_pair.argtypes)


# ---- capf_cpn_decode_pair: refusals before any launch ----------------------------------------------------------------------------------------
P = 0x10000        # a well-aligned non-NULL "pointer": every call below is refused before anything could read it
H36M = (capf.c_int32 * 17)(*capf.H36M_SWAP)


def _table(*entries):
    return (capf.c_int32 * len(entries))(*entries)


def _args(**kw):
    a = dict(stream=None, map=P, dtype=capf.F32, B=2, H=8, W=6, C=20, J=17, swap=H36M, decode=(capf.c_float * 4)(4, 2, 4, 2), to_image=None,
             mirror_width=192.0, kcrop2=P, k2d2=None, score=None, blurred=None, fused=None)
    a.update(kw)
    return list(a.values())


NOT_INVOLUTIVE = list(range(17))
NOT_INVOLUTIVE[1:4] = [2, 3, 1]            # a permutation (a 3-cycle), but not its own inverse
REPEATED = list(range(17))
REPEATED[5] = 4                            # not a permutation at all
REFUSALS = [
    ("NULL map", dict(map=None), INVALID), ("NULL decode", dict(decode=None), INVALID), ("NULL swap", dict(swap=None), INVALID),
    ("NULL kcrop2", dict(kcrop2=None), INVALID), ("k2d2 without to_image", dict(k2d2=P), INVALID),
    ("Bsrc = 0", dict(B=0), INVALID), ("Bsrc < 0", dict(B=-2), INVALID), ("H = 0", dict(H=0), INVALID), ("W = 0", dict(W=0), INVALID),
    ("J = 0", dict(J=0, swap=_table(0)), INVALID), ("J > C", dict(J=21, swap=_table(*range(21))), INVALID),
    ("C > 32", dict(C=33, J=33, swap=_table(*range(33))), INVALID), ("C = 36", dict(C=36), INVALID),
    ("dtype 3", dict(dtype=3), INVALID), ("dtype -1", dict(dtype=-1), INVALID),
    ("misaligned fp32 map", dict(map=P + 8), INVALID), ("misaligned 16-bit map", dict(map=P + 4, dtype=capf.BF16), INVALID),
    ("misaligned kcrop2", dict(kcrop2=P + 2), INVALID), ("misaligned blurred", dict(blurred=P + 4), INVALID),
    ("misaligned fused", dict(fused=P + 2), INVALID),
    ("mirror_width = inf", dict(mirror_width=float("inf")), INVALID), ("mirror_width = NaN", dict(mirror_width=float("nan")), INVALID),
    ("swap entry = J", dict(swap=_table(*([17] + list(range(1, 17))))), INVALID),
    ("swap entry < 0", dict(swap=_table(*([-1] + list(range(1, 17))))), INVALID),
    ("swap not involutive", dict(swap=_table(*NOT_INVOLUTIVE)), INVALID), ("swap repeats a joint", dict(swap=_table(*REPEATED)), INVALID),
    ("swap of J = 1 out of range", dict(J=1, swap=_table(1)), INVALID),
    ("plane too large for the LDS", dict(H=128, W=128), UNSUPPORTED), ("far too large", dict(H=4096, W=4096), UNSUPPORTED),
    ("a grid of 2^31 blocks", dict(B=1 << 27, J=16, swap=_table(*range(16))), UNSUPPORTED),
]


@pytest.mark.parametrize("why,kw,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_pair_refusals_need_no_device(why, kw, code):
    assert capf.load_library().capf_cpn_decode_pair(*_args(**kw)) == code, why


def test_pair_refusal_edges():
    lib = capf.load_library()
    # a 16-bit map needs 8-byte alignment only: the call gets as far as the LDS limit
    assert lib.capf_cpn_decode_pair(*_args(map=P + 8, dtype=capf.BF16, H=128, W=128)) == UNSUPPORTED
    # one block below 2^31 passes the grid rule (and is then stopped by the next one asked for here: the plane)
    assert lib.capf_cpn_decode_pair(*_args(B=(1 << 27) - 1, J=16, swap=_table(*range(16)), H=128, W=128)) == UNSUPPORTED
    assert lib.capf_cpn_decode_pair(*_args(B=(1 << 27) - 1, J=16, swap=_table(*NOT_INVOLUTIVE[:16]))) == INVALID
    # a bad table is INVALID even where the shape alone would be UNSUPPORTED: the arguments are judged before the device limits
    assert lib.capf_cpn_decode_pair(*_args(H=128, W=128, swap=_table(*NOT_INVOLUTIVE))) == INVALID


def test_binding_refuses_on_the_host():
    with pytest.raises(capf.CapfError, match="2 \\* Bsrc frames"):
        capf.cpn_decode_pair(torch.zeros(3, 4, 4, 20), 17)
    with pytest.raises(capf.CapfError, match="H36M table"):
        capf.cpn_decode_pair(torch.zeros(2, 4, 4, 20), 16)
    with pytest.raises(capf.CapfError, match="swap has 3 entries"):
        capf.cpn_decode_pair(torch.zeros(2, 4, 4, 20), 17, swap=(0, 2, 1))
    with pytest.raises(capf.CapfError, match="to_image"):
        capf.cpn_decode_pair(torch.zeros(4, 4, 4, 20), 17, to_image=torch.zeros(4, 2, 3))          # [Bsrc, 2, 3], not [2 Bsrc, 2, 3]
    with pytest.raises(capf.CapfError, match="NHWC map"):
        capf.cpn_decode_pair(torch.zeros(2, 4, 4, 20, dtype=torch.float64), 17)


# ---- the host module -------------------------------------------------------------------------------------------------------------------
def _module(backbone, **kw):
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    c = backbone_preset(copy.deepcopy(config), backbone)
    c.model.backbone.fix_weights = True
    with contextlib.redirect_stdout(io.StringIO()):
        return CA_PF(c, **kw)


def test_new_entries_need_the_cpn_head():
    x, A = torch.zeros(2, 256, 192, 3), torch.zeros(2, 2, 3)
    for m in (_module("hrnet_32", keypoint_head="argmax"), _module("hrnet_32"), _module("cpn"), _module("cpn", keypoint_head="integral")):
        with pytest.raises(ValueError, match="keypoint_head='cpn'"):
            m.detect_cpn_flip(x)
        with pytest.raises(ValueError, match="keypoint_head='cpn'"):
            m.forward_detect_cpn_flip(x, A)


def test_old_entries_still_raise_and_new_ones_refuse_on_the_host():
    m = _module("cpn", keypoint_head="cpn")
    x, x5, A = torch.zeros(2, 256, 192, 3), torch.zeros(2, 2, 256, 192, 3), torch.zeros(2, 2, 3)
    with pytest.raises(NotImplementedError, match="flip"):
        m.detect_flip_test(x)
    with pytest.raises(NotImplementedError, match="detect_cpn_flip"):
        m.forward_detect_flip_test(x, A)
    with pytest.raises(ValueError, match="to_image"):
        m.forward_detect_cpn_flip(x, None)
    with pytest.raises(TypeError, match="float32 or uint8"):
        m.detect_cpn_flip(x.double())
    with pytest.raises(TypeError, match="float32 \\[2,B,H,W,3\\] stack"):
        m.detect_cpn_flip(x5.to(torch.uint8))
    for bad in ((0, 2, 1), [17] + list(range(1, 17)), list(NOT_INVOLUTIVE), list(REPEATED)):
        with pytest.raises(ValueError, match="flip_pairs"):
            m.detect_cpn_flip(x, flip_pairs=bad)
    # everything host-side accepted: the call stops at the device check (CPU tensors), for each of the three image forms
    for images in (x, x5, x.to(torch.uint8)):
        for table in (None, capf.H36M_SWAP, list(capf.COCO_SWAP)):
            with pytest.raises(capf.CapfError, match="MI355X only"):
                m.forward_detect_cpn_flip(images, A, flip_pairs=table)
            with pytest.raises(capf.CapfError, match="MI355X only"):
                m.detect_cpn_flip(images, flip_pairs=table)
    # the head has no derivative: a final_predict parameter that asks for a gradient is refused under grad, before anything runs
    next(m.backbone.refine_net.final_predict.parameters()).requires_grad_(True)
    assert torch.is_grad_enabled()
    with pytest.raises(NotImplementedError, match="final_predict"):
        m.detect_cpn_flip(x)
    with pytest.raises(NotImplementedError, match="final_predict"):
        m.forward_detect_cpn_flip(x, A)
    with torch.no_grad(), pytest.raises(capf.CapfError, match="MI355X only"):
        m.detect_cpn_flip(x)
    assert "detect_cpn_flip" in type(m).__init__.__doc__
