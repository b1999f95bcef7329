"""CPU (no device): CAPF_PLAN_BF16_F32_STREAM -- the bf16 HRNet plan whose activation stream stays fp32 (bf16 only as conv operands,
capf_oracle.BF16_STREAM_FP32).  Which combinations capf_create accepts, where every backbone tensor is stored (the storage rule of
include/capf.h), what capf_op_bytes counts, and that the kernels it adds do not spill registers."""
import copy
import ctypes
import os
import re

import pytest

from conftest import ROOT

BATCHES = (1, 4, 16, 64, 256)


def _cfg(backbone):
    from mvn.utils.cfg import backbone_preset, config
    c = backbone_preset(copy.deepcopy(config), backbone)
    c.model.backbone.fix_weights = True
    return c


def _engine(backbone, dtype="bf16", flags=0):
    from capf import Engine
    from mvn.models import _native
    return Engine(_native.make_capf_config(_cfg(backbone), 256, 256, compute_dtype=dtype, plan_flags=flags), device=None)


def _stream():
    from capf.lib import PLAN_BF16_F32_STREAM
    return PLAN_BF16_F32_STREAM


def _n_backbone(eng):
    return sum(1 for i in range(eng.lib.capf_num_ops(eng.h)) if eng.op_describe(i).backbone)


def _sched(eng):
    """[(reads[5], writes[6])] per op, slots kept (capf_op_schedule: reads 0..3 inputs, 4 residual; writes 0 output)"""
    out = []
    for i in range(eng.lib.capf_num_ops(eng.h)):
        rg, lv, ln = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        rd, wr = (ctypes.c_int32 * 5)(), (ctypes.c_int32 * 6)()
        assert eng.lib.capf_op_schedule(eng.h, i, ctypes.byref(rg), ctypes.byref(lv), ctypes.byref(ln), rd, wr) == 0
        out.append((list(rd), list(wr)))
    return out


def _readers(sched):
    """buffer id -> [(op index, slot)] over the whole plan"""
    out = {}
    for i, (reads, _) in enumerate(sched):
        for slot, b in enumerate(reads):
            if b >= 0:
                out.setdefault(b, []).append((i, slot))
    return out


def test_flag_value_and_accepted_combinations():
    from capf.lib import CapfError, PLAN_NO_WS, PLAN_NO_ROW_HALO, PLAN_NO_BNECK, PLAN_LIFTER_FP32
    assert _stream() == 1 << 15
    for bb in ("hrnet_32", "hrnet_48"):
        eng = _engine(bb, "bf16", _stream())
        assert eng.lib.capf_num_ops(eng.h) == _engine(bb, "bf16").lib.capf_num_ops(_engine(bb, "bf16").h)
    with pytest.raises(CapfError):
        _engine("hrnet_32", "fp32", _stream())                   # the flag only has meaning for a bf16 backbone
    with pytest.raises(CapfError):
        _engine("cpn", "bf16", _stream())                        # HRNet only (the oracle's stream_fp32 asserts HRNet)
    for other in (PLAN_NO_WS, PLAN_NO_ROW_HALO, PLAN_NO_BNECK, PLAN_LIFTER_FP32):
        with pytest.raises(CapfError):
            _engine("hrnet_48", "bf16", _stream() | other)       # not run by the layer-wise test: refused, never mis-computed
    with pytest.raises(CapfError):
        _engine("hrnet_32", "bf16", 1 << 14)                     # still unassigned


@pytest.mark.parametrize("backbone", ["hrnet_32", "hrnet_48"])
def test_storage_rule_of_the_stream_plan(backbone):
    base, eng = _engine(backbone), _engine(backbone, "bf16", _stream())
    n, nbb = eng.lib.capf_num_ops(eng.h), _n_backbone(eng)
    assert nbb == _n_backbone(base)
    sched = _sched(base)
    readers = _readers(sched)
    written = {sched[j][1][0] for j in range(nbb)} - {-1}
    feats = set()
    for i in range(nbb, n):                                      # the lifter's samplers read the four context maps
        feats |= {b for b in sched[i][0][:4] if b in written}
    assert len(feats) == 4
    n_f32, bf16_sums = 0, []
    for i in range(nbb):
        d = eng.op_describe(i)
        if d.kind not in (0, 1):
            continue
        out = sched[i][1][0]
        rd = readers.get(out, [])
        conv_only = out not in feats and all(j < nbb and base.op_describe(j).kind == 0 and base.op_describe(j).conv and s == 0
                                             for j, s in rd)
        if d.kind == 0 and d.conv:
            assert d.mfma_bf16 == 1, base.op_table(1)[i][0]
        name = base.op_table(1)[i][0]
        if d.kind == 1 or out in feats:
            assert d.out_dtype == 0, name
        if d.has_residual and d.out_dtype == 2:
            # rule 1 wins over "a residual add stores fp32": e.g. layer1's last bottleneck sum is read by the two transition1 convs only
            bf16_sums.append(name)
        assert d.out_dtype == (2 if conv_only else 0), name
        if d.kind == 1:
            assert d.in_dtype == 0
        n_f32 += d.out_dtype == 0
        # a conv takes a shadow exactly where its producer stores fp32: its operand stays bf16
        if d.kind == 0 and d.conv and sched[i][0][0] >= 0:
            assert d.in_dtype == 2
    # (and the last module's branches 1..3, which only its fuse layer's 1x1 convs read: multi_scale_output=False)
    assert n_f32 > 0 and bf16_sums == ["backbone.layer1.3.conv3"] + [f"backbone.stage4.2.branches.{b}.3.conv2" for b in (1, 2, 3)]
    for l in range(4):
        ptr, shape, nd = ctypes.c_void_p(), (ctypes.c_int64 * 4)(), ctypes.c_int()
        assert eng.lib.capf_tensor(eng.h, f"feat{l}".encode(), ctypes.byref(ptr), shape, ctypes.byref(nd)) == 0
        assert base.lib.capf_tensor(base.h, f"feat{l}".encode(), ctypes.byref(ptr), shape, ctypes.byref(nd)) == 2
    for batch in BATCHES:
        got, want = eng.op_table(batch), base.op_table(batch)
        assert [r[0] for r in got] == [r[0] for r in want]
        # layer1 on one launch per conv under the flag (the fused bottleneck / pointwise-chain kernels have no fp32-stream epilogue)
        assert not any(k.startswith(("bneck", "igemm_bf16_pwchain")) for _, k, _ in got)
        assert not any(k.startswith("igemm_bf16_rh") for _, k, _ in got)
        if batch >= 16:
            assert any(k.startswith("bneck") for _, k, _ in want)
        if batch >= 64:
            assert any(k.startswith("igemm_bf16_ws") for _, k, _ in got[:nbb])


@pytest.mark.parametrize("backbone", ["hrnet_32", "hrnet_48"])
def test_op_bytes_count_the_fp32_stream(backbone):
    base, eng = _engine(backbone), _engine(backbone, "bf16", _stream())
    nbb = _n_backbone(eng)
    for batch in BATCHES:
        b0, b1 = base.op_bytes(batch), eng.op_bytes(batch)
        assert len(b0) == len(b1)
        for i, (x, y) in enumerate(zip(b0, b1)):
            assert y >= x, (i, x, y)
            if i < nbb:
                d, d0 = eng.op_describe(i), base.op_describe(i)
                if d.kind in (0, 1) and d.out_dtype == 0 and d0.out_dtype == 2:
                    assert y > x, (i, x, y)


def test_stream_kernels_do_not_spill_registers():
    """The no-spill build guard of test_abi.py over the sources this plan adds kernels to.  igemm_bf16_group_ws_kernel (the DEFAULT 2-D halo
    tile, unchanged here) already spills 17 VGPRs with this compiler at its (256, 2) launch bound: pinned, so that it cannot get worse."""
    import concurrent.futures, shutil, subprocess, tempfile
    hipcc = shutil.which("hipcc")
    if hipcc is None:
        pytest.skip("hipcc not on PATH")
    csrc = os.path.join(ROOT, "contextaware-poseformer_amd", "csrc")

    def spills(name):
        with tempfile.TemporaryDirectory() as d:
            out = os.path.join(d, name + ".s")
            subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                            "-S", "--cuda-device-only", os.path.join(csrc, name + ".hip"), "-o", out],
                           check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
            text = open(out).read()
        names = re.findall(r"^\s+\.name:\s+(\S+)", text, flags=re.M)
        counts = [int(v) for v in re.findall(r"^\s+\.vgpr_spill_count:\s+(\d+)", text, flags=re.M)]
        assert len(names) == len(counts) and counts
        return list(zip(names, counts))

    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        got = dict(sum(ex.map(spills, ["igemm_bf16", "igemm_bf16_ws", "bneck_bf16", "elementwise"]), []))
    stream = [k for k in got if "stream" in k or "shadow" in k]
    assert len(stream) >= 5, stream          # single / ring / ping-pong / 2-D halo conv kernels, fuse sums with a shadow
    pinned = {"_ZN4capf26igemm_bf16_group_ws_kernelENS_11WsGroupArgsE": 17}
    bad = [(k, c) for k, c in got.items() if c > pinned.get(k, 0)]
    assert not bad, f"kernels with register spills: {bad}"


@pytest.mark.parametrize("backbone", ["hrnet_32", "hrnet_48"])
def test_stream_plan_schedule_orders_every_shadow_before_its_readers(backbone):
    """A conv reading a shadow must sit on a later dependency level of its region than the op that writes the shadow (capf_op_schedule
    reports the shadow among the op's writes): the grouped schedule issues a level as one launch."""
    eng = _engine(backbone, "bf16", _stream())
    sched, rows = _sched(eng), eng.op_schedule()
    writer = {}
    for i, (_, wr) in enumerate(sched):
        for b in wr:
            if b >= 0:
                writer[b] = i
    checked = 0
    for i, (rd, _) in enumerate(sched):
        for b in rd:
            j = writer.get(b, -1)
            if b < 0 or j < 0 or j >= i or rows[i][0] < 0 or rows[i][0] != rows[j][0]:
                continue
            assert rows[j][1] < rows[i][1], (i, j, b)
            checked += 1
    assert checked > 100
