"""CPU: the C-ABI library loads, exports every symbol include/capf.h declares, and its parameter
schema / host module state_dict equal the reference's state_dict (captured in tests/golden/schema_*.json
by oracle/make_goldens.py).  No compute calls — there is no GPU here."""
import copy
import ctypes
import json
import os
import re

import pytest

from conftest import ROOT


def _header_symbols():
    text = open(os.path.join(ROOT, "include", "capf.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(capf_[a-z_0-9]+)\s*\(", text)))


def test_library_exports_every_declared_symbol():
    import capf
    from capf.lib import EXPORTS
    lib = capf.load_library()
    declared = _header_symbols()
    assert declared, "no declarations parsed"
    for sym in declared:
        assert hasattr(lib, sym), f"libcapf.so does not export {sym}"
    assert sorted(EXPORTS) == declared
    assert b"gfx950" in lib.capf_version()


def test_library_exports_nothing_but_the_c_abi():
    """-fvisibility=hidden + csrc/capf.map: the dynamic symbol table is the header, not the C++ internals (`nm -D` showed
    capf::launch_* beside the 81 C symbols)."""
    import shutil
    import subprocess
    from capf import lib as capf_lib
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-D", "--defined-only", capf_lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    defined = sorted(line.split()[-1] for line in out.splitlines() if line.strip())
    assert defined == _header_symbols()


def _cfg(backbone):
    from mvn.utils.cfg import backbone_preset, config
    c = backbone_preset(copy.deepcopy(config), backbone)
    c.model.backbone.fix_weights = True
    return c


@pytest.mark.parametrize("backbone", ["hrnet_32", "hrnet_48", "cpn"])
def test_schema_equals_reference_state_dict(backbone):
    from capf import Engine
    from mvn.models import _native
    want = json.load(open(os.path.join(ROOT, "tests", "golden", f"schema_{backbone}.json")))
    c = _native.make_capf_config(_cfg(backbone), 256, 192)
    eng = Engine(c, device=None)
    got = {n: list(s) for n, s, k in eng.schema()}
    assert got == want
    launches, flops = eng.stats(1)
    assert launches > 100 and flops > 1e10
    assert eng.workspace_bytes(4) > eng.workspace_bytes(1) > 0          # inference + training regions
    layout, total = eng.grad_layout()
    lifter = {n: s for n, s in want.items() if n.startswith("volume_net.")}
    assert set(layout) == set(lifter) and total == sum(int(__import__("math").prod(s)) for s in lifter.values())
    c.training = 0
    inf = Engine(c, device=None)
    assert inf.workspace_bytes(4) == 4 * inf.workspace_bytes(1) > 0      # activations scale with the batch


@pytest.mark.parametrize("backbone", ["hrnet_32", "cpn"])
def test_host_module_state_dict_and_freeze(backbone):
    import contextlib, io
    from mvn.models.conpose import CA_PF
    want = json.load(open(os.path.join(ROOT, "tests", "golden", f"schema_{backbone}.json")))
    with contextlib.redirect_stdout(io.StringIO()):
        m = CA_PF(_cfg(backbone))
    sd = m.state_dict()
    assert {k: list(v.shape) for k, v in sd.items()} == want
    assert not any(p.requires_grad for p in m.backbone.parameters())          # conpose.py:22-25
    assert all(p.requires_grad for p in m.volume_net.parameters())
    m.load_state_dict(sd, strict=True)
    # callers' access patterns (train.py:147-148, 339): .backbone.eval(), .volume_net.named_parameters()
    m.backbone.eval(); m.volume_net.train()
    assert len(list(m.volume_net.named_parameters())) == 191 - 0 if backbone == "hrnet_32" else True


def test_flops_match_survey():
    """Algorithmic FLOPs reported by the plan == SURVEY.md §8d (probed on the reference)."""
    from capf import Engine
    from mvn.models import _native
    for bb, hw, gflop in (("hrnet_32", (256, 256), 20.995), ("hrnet_48", (256, 256), 42.469), ("cpn", (384, 288), 23.182)):
        eng = Engine(_native.make_capf_config(_cfg(bb), *hw), device=None)
        _, f = eng.stats(1)
        assert abs(f / 1e9 - gflop) / gflop < 0.01, (bb, f / 1e9)


def test_errors_are_reported():
    from capf import CapfError, Engine
    from mvn.models import _native
    c = _native.make_capf_config(_cfg("hrnet_32"), 250, 192)      # not a multiple of 32
    with pytest.raises(CapfError):
        Engine(c, device=None)
    bad = _cfg("hrnet_32")
    bad.model.backbone.STAGE3.NUM_BLOCKS = [4, 4]
    with pytest.raises(ValueError):                                # pose_hrnet.py:159-175 semantics
        _native.make_capf_config(bad)
    import torch
    from mvn.models.conpose import CA_PF
    import contextlib, io
    with contextlib.redirect_stdout(io.StringIO()):
        m = CA_PF(_cfg("hrnet_32"))
    with pytest.raises(CapfError):                                 # no CPU fallback
        m(torch.zeros(1, 256, 192, 3), torch.zeros(1, 17, 2), torch.zeros(1, 17, 2))


@pytest.mark.parametrize("backbone", ["hrnet_32", "hrnet_48", "cpn"])
def test_region_schedule_is_a_valid_topological_order(backbone):
    """capf_set_lanes mode 2 issues every fork/join region level by level (the fp32 convs of a level in one
    grouped launch).  Host-side check on the static plan: inside a region an op's level is above the level of
    every earlier op it conflicts with on a workspace buffer, and the ops of one level are pairwise
    independent (so one grid may run them concurrently)."""
    from capf import Engine
    from mvn.models import _native
    eng = Engine(_native.make_capf_config(_cfg(backbone), 256, 192), device=None)
    sched = eng.op_schedule()
    regions = {}
    for i, (rg, lv, ln, rd, wr) in enumerate(sched):
        if rg >= 0:
            assert lv >= 0, f"op {i} of region {rg} has no level"
            regions.setdefault(rg, []).append(i)
    assert len(regions) >= (20 if backbone != "cpn" else 5)
    widest = 0
    for rg, ops in regions.items():
        by_level = {}
        for a_pos, a in enumerate(ops):
            _, la, _, ra, wa = sched[a]
            by_level.setdefault(la, []).append(a)
            for b in ops[:a_pos]:                       # b precedes a in program order
                _, lb, _, rb, wb = sched[b]
                conflict = (set(wb) & (set(ra) | set(wa))) or (set(rb) & set(wa))
                if conflict:
                    assert la > lb, f"op {a} (level {la}) depends on op {b} (level {lb}) via buffers {conflict}"
        for lv, members in by_level.items():
            widest = max(widest, len(members))
            for x in members:
                for y in members:
                    if x < y:
                        assert not (set(sched[x][4]) & (set(sched[y][3]) | set(sched[y][4])))
                        assert not (set(sched[y][4]) & set(sched[x][3]))
    assert widest >= 4          # e.g. the four branches of a stage-4 module / the CPN refine cascades


def test_tile_choice_avoids_a_second_round_for_the_lifter_gemms():
    """Static plan, no GPU: the cost model behind pick_tile (igemm_f32.hip) must not give the lifter's
    M = 17 * 64 = 1088-row GEMMs 128-row tiles (9 x 30 = 270 tiles = two rounds on 256 CUs); the 32-channel
    64x64 branch keeps its tall 256x32 tile when it is launched on its own."""
    from capf import Engine
    from mvn.models import _native
    from capf.lib import PLAN_NO_F32H2_GEMM
    eng = Engine(_native.make_capf_config(_cfg("hrnet_32"), 256, 256), device=None)
    table = {name: kern for name, kern, _ in eng.op_table(64)}
    # round 5: from batch 5 the lifter's projections run the two-fp16-piece GEMM (64 x 64 tiles as well), the LayerNorm-folded ones
    # (K = 128: res blocks' qkv / fc1, context blocks' fc1) included; every batch below 5 stays on the fp32 MFMA kernel
    assert table["joint0.qkv"] == "igemm_f32h2g<64x64,rows>" and table["joint0.fc2"] == "igemm_f32h2g<64x64,rows>"
    assert table["ctx0.mlp"] == "mlp_chain" and "ctx0.fc1" not in table       # (round 6: a context block's MLP half is one launch)
    # round 6: the res blocks are ONE launch at every batch (lifter_chain.hip) ...
    assert table["res.chain"] == "res_chain" and not any(n.startswith("res0.") for n in table)
    assert {name: kern for name, kern, _ in eng.op_table(1)}["res.chain"] == "res_chain"
    assert {name: kern for name, kern, _ in eng.op_table(4)}["joint0.qkv"].startswith("igemm_f32<")
    eng_f = Engine(_native.make_capf_config(_cfg("hrnet_32"), 256, 256, plan_flags=PLAN_NO_F32H2_GEMM), device=None)
    table_f = {name: kern for name, kern, _ in eng_f.op_table(64)}
    assert table_f["joint0.qkv"] == "igemm_f32<w4,64x64,rows>"
    assert table_f["res0.qkv"].startswith("igemm_f32<") and "res.chain" not in table_f       # ... unless the plan has no two-piece packs
    assert table_f["ctx0.fc1"].startswith("igemm_f32<") and "ctx0.mlp" not in table_f
    assert table_f["joint0.fc2"] == "igemm_f32<w4,64x64,rows>"
    assert not any(k.startswith("igemm_f32h2g") for k in table_f.values())
    # the 3x3 stride-1 convs run the direct kernel (tall 256x32 tile for the 32-channel 64x64 branch launched on its own) below batch 5 and
    # the split-fp32 tile from 370 MFLOP per conv (batch 5 for these branches); a plan without that tile (CAPF_PLAN_NO_F32X3) runs them on
    # the Winograd kernel from batch 24
    assert table["backbone.stage2.0.branches.0.0.conv1"] == "igemm_f32h2_group_ws"       # (round 5: two fp16 pieces, three products)
    assert {name: kern for name, kern, _ in eng.op_table(6)}["backbone.stage2.0.branches.0.0.conv1"] == "igemm_f32h2_group_ws"
    from capf.lib import PLAN_NO_F32X3, PLAN_F32X3_EXACT
    eng_x = Engine(_native.make_capf_config(_cfg("hrnet_32"), 256, 256, plan_flags=PLAN_F32X3_EXACT), device=None)   # round 4's exact three-piece tile
    assert {name: kern for name, kern, _ in eng_x.op_table(64)}["backbone.stage2.0.branches.0.0.conv1"] == "igemm_f32x3_group_ws"
    assert [k for _, k, _ in eng_x.op_table(64) if not k.startswith("igemm_f32x3")] == [k for _, k, _ in eng.op_table(64) if not k.startswith("igemm_f32h2_")]
    eng_w = Engine(_native.make_capf_config(_cfg("hrnet_32"), 256, 256, plan_flags=PLAN_NO_F32X3), device=None)
    assert {name: kern for name, kern, _ in eng_w.op_table(24)}["backbone.stage2.0.branches.0.0.conv1"] == "igemm_wino43_group"   # F(4,3): row length 64 is a multiple of 4
    # (between batch 5 and the Winograd kernels' batch 24 the direct route is the two-fp16-piece GEMM; the whole fp32-pipe plan of round 3
    # is CAPF_PLAN_NO_F32X3 | CAPF_PLAN_NO_F32H2_GEMM)
    assert {name: kern for name, kern, _ in eng_w.op_table(16)}["backbone.stage2.0.branches.0.0.conv1"].startswith("igemm_f32h2g<")
    eng_p = Engine(_native.make_capf_config(_cfg("hrnet_32"), 256, 256, plan_flags=PLAN_NO_F32X3 | PLAN_NO_F32H2_GEMM), device=None)
    assert {name: kern for name, kern, _ in eng_p.op_table(16)}["backbone.stage2.0.branches.0.0.conv1"].startswith("igemm_f32<")
    assert not any(k.startswith(("igemm_f32h2", "igemm_f32x3")) for _, k, _ in eng_p.op_table(64))
    small = {name: kern for name, kern, _ in eng.op_table(4)}
    assert small["backbone.stage2.0.branches.0.0.conv1"].startswith("igemm_f32<")
    # layer1's HBM-bound 1x1 bottleneck convs: the pointwise kernel from 2048 tiles per launch, the general tile below
    assert table["backbone.layer1.0.conv3"] == "igemm_f32_pw<w4,128x64>"
    assert table["backbone.layer1.1.conv1"] == "igemm_f32_pw<w4,128x64>"
    # (the conv3 -> next conv1 pairs stay on the fp32 kernels at every batch: the chained and the two-launch routes must give the same bits)
    assert {name: kern for name, kern, _ in eng.op_table(8)}["backbone.layer1.0.conv3"].startswith("igemm_f32<")
    assert {name: kern for name, kern, _ in eng.op_table(8)}["backbone.layer1.0.conv1"].startswith("igemm_f32h2g<")
    assert {name: kern for name, kern, _ in eng_f.op_table(8)}["backbone.layer1.0.conv1"].startswith("igemm_f32<")
    big = {name: kern for name, kern, _ in eng.op_table(512)}
    assert big["joint0.qkv"] == "igemm_f32h2g<128x128,rows>" and big["joint0.fc1"] == "igemm_f32h2g<128x64,rows>"     # (1020 / 680 tiles of 128 x 128)
    assert {name: kern for name, kern, _ in eng_f.op_table(512)}["joint0.qkv"] in ("igemm_f32<w4,128x128,rows>", "igemm_f32<w4,128x64,rows>")


def test_conv_group_rejects_bad_arguments_without_a_gpu():
    """capf_op_conv_group validates before it launches: the error paths need no device."""
    import capf
    from capf.lib import ConvDesc
    lib = capf.load_library()
    d = (ConvDesc * 9)()
    for i in range(9):
        d[i].x = d[i].w_packed = d[i].bias = d[i].y = 4096          # never dereferenced on these paths
        d[i].B, d[i].H, d[i].W, d[i].Cin, d[i].Cout, d[i].ks, d[i].stride, d[i].act = 1, 8, 8, 32, 32, 3, 1, 0
    assert lib.capf_op_conv_group(None, 0, d) != 0                  # empty group
    assert lib.capf_op_conv_group(None, 9, d) != 0                  # more than MAXG = 8 problems
    assert lib.capf_op_conv_group(None, 2, None) != 0
    d[1].Cin = 3                                                    # the small-Cin stem kernel cannot be grouped
    assert lib.capf_op_conv_group(None, 2, d) != 0
    d[1].Cin, d[1].ks = 32, 7                                       # 49 taps do not fit the 32-bit tap mask
    assert lib.capf_op_conv_group(None, 2, d) != 0


INVALID, UNSUPPORTED = -1, -2          # include/capf.h :: CAPF_ERR_INVALID, CAPF_ERR_UNSUPPORTED

# The exact status of every error path of the stand-alone conv / linear / pack entry points that returns before a launch (recorded
# from the library these entry points were first written in).  Each problem below is one that the family's own check rejects, so no
# call reaches a kernel: the pointers are never dereferenced.
_GROUP_CALLS = {
    "capf_op_conv_group": lambda lib, n, d: lib.capf_op_conv_group(None, n, d),
    "capf_op_conv_wino_group": lambda lib, n, d: lib.capf_op_conv_wino_group(None, n, d, 23),
    "capf_op_conv_bf16_group": lambda lib, n, d: lib.capf_op_conv_bf16_group(None, n, d, None, None),
    "capf_op_conv_bf16_ws_group": lambda lib, n, d: lib.capf_op_conv_bf16_ws_group(None, n, d),
    "capf_op_conv_f32x3_group": lambda lib, n, d: lib.capf_op_conv_f32x3_group(None, n, d),
    "capf_op_conv_f32h2_group": lambda lib, n, d: lib.capf_op_conv_f32h2_group(None, n, d),
    "capf_op_conv_f32h2g_group": lambda lib, n, d: lib.capf_op_conv_f32h2g_group(None, n, d),
}
# (entry point, field of problem 1, value) -> status; problem 0 is a plain 3x3 conv
_GROUP_BAD_PROBLEM = {
    ("capf_op_conv_group", "Cin", 3): UNSUPPORTED,                # Cin % 4
    ("capf_op_conv_bf16_group", "Cin", 4): UNSUPPORTED,           # Cin % 8
    ("capf_op_conv_wino_group", "ks", 5): UNSUPPORTED,
    ("capf_op_conv_wino_group", "stride", 2): UNSUPPORTED,
    ("capf_op_conv_wino_group", "act", 2): UNSUPPORTED,           # GELU
    ("capf_op_conv_bf16_ws_group", "ks", 5): UNSUPPORTED,
    ("capf_op_conv_bf16_ws_group", "stride", 2): UNSUPPORTED,
    ("capf_op_conv_bf16_ws_group", "act", 2): UNSUPPORTED,
    ("capf_op_conv_f32x3_group", "ks", 5): UNSUPPORTED,
    ("capf_op_conv_f32x3_group", "stride", 2): UNSUPPORTED,
    ("capf_op_conv_f32x3_group", "act", 2): UNSUPPORTED,
    ("capf_op_conv_f32h2_group", "ks", 5): UNSUPPORTED,
    ("capf_op_conv_f32h2_group", "stride", 2): UNSUPPORTED,
    ("capf_op_conv_f32h2_group", "act", 2): UNSUPPORTED,
    ("capf_op_conv_f32h2g_group", "ks", 0): INVALID,
    ("capf_op_conv_f32h2g_group", "stride", 0): INVALID,
    ("capf_op_conv_f32h2g_group", "Cin", 3): UNSUPPORTED,         # Cin % 4
}


def _conv_descs(n, **problem1):
    from capf.lib import ConvDesc
    d = (ConvDesc * n)()
    for c in d:
        c.x = c.w_packed = c.bias = c.y = 4096
        c.B, c.H, c.W, c.Cin, c.Cout, c.ks, c.stride, c.act = 1, 8, 8, 32, 32, 3, 1, 0
    for k, v in problem1.items():
        setattr(d[1], k, v)
    return d


@pytest.mark.parametrize("name", sorted(_GROUP_CALLS))
def test_conv_group_entry_points_validate_n_and_d_without_a_gpu(name):
    import capf
    lib, call = capf.load_library(), _GROUP_CALLS[name]
    assert call(lib, 0, _conv_descs(9)) == INVALID                 # empty group
    assert call(lib, 9, _conv_descs(9)) == INVALID                 # more than MAXG = 8 problems
    assert call(lib, 2, None) == INVALID


@pytest.mark.parametrize("case", sorted(_GROUP_BAD_PROBLEM), ids=lambda c: f"{c[0]}-{c[1]}={c[2]}")
def test_conv_group_entry_points_reject_a_problem_without_a_gpu(case):
    import capf
    name, field, value = case
    assert _GROUP_CALLS[name](capf.load_library(), 2, _conv_descs(2, **{field: value})) == _GROUP_BAD_PROBLEM[case]


def test_standalone_op_pre_launch_return_codes_without_a_gpu():
    import ctypes
    import capf
    lib = capf.load_library()
    F = 4096
    assert lib.capf_op_conv_wino_group(None, 2, _conv_descs(2), 22) == INVALID                   # not a Winograd variant
    conv_wino = lambda Cin=32, act=0, variant=23: lib.capf_op_conv_wino(None, F, F, F, None, F, 1, 8, 8, Cin, 32, act, variant)
    assert conv_wino(variant=22) == UNSUPPORTED
    assert conv_wino(Cin=16) == UNSUPPORTED                                                        # Cin % 32
    assert conv_wino(act=2) == UNSUPPORTED
    conv_h2g = lambda Cin=32, ks=3, stride=1: lib.capf_op_conv_f32h2g(None, F, F, F, None, F, 1, 8, 8, Cin, 32, ks, stride, 0)
    assert conv_h2g(ks=0) == INVALID
    assert conv_h2g(stride=0) == INVALID
    assert conv_h2g(Cin=3) == UNSUPPORTED
    planes = lambda d, ein=None, eout=None: lib.capf_op_conv_f32h2_planes(None, d, ein, eout)
    one = lambda **kw: ctypes.byref(_conv_descs(2, **kw)[1])
    assert planes(None) == UNSUPPORTED
    assert planes(one(ks=5)) == UNSUPPORTED
    assert planes(one(stride=2)) == UNSUPPORTED
    assert planes(one(act=2)) == UNSUPPORTED
    assert planes(one(), F, F) == UNSUPPORTED                                                      # planes in and out
    linear = lambda K=64: lib.capf_op_linear(None, F, F, F, None, F, 16, 32, K, 0)
    linear_h2g = lambda N=32, K=64: lib.capf_op_linear_f32h2g(None, F, F, F, None, F, 16, N, K, 0)
    linear_ln = lambda g=F, b=F, K=64: lib.capf_op_linear_ln_f32h2g(None, F, g, b, 1e-5, F, F, None, F, 16, 32, K, 0)
    assert linear(K=48) == UNSUPPORTED
    assert linear_h2g(K=48) == UNSUPPORTED
    assert linear_h2g(N=6) == UNSUPPORTED                                                          # N % 4
    assert linear_ln(K=48) == UNSUPPORTED
    assert linear_ln(g=None) == UNSUPPORTED
    assert linear_ln(b=None) == UNSUPPORTED
    assert linear_ln(K=512) == UNSUPPORTED                                                         # LayerNorm over more than 256 columns
    assert lib.capf_op_wgrad(None, F, F, 16, 6, 32, F, 0) == UNSUPPORTED                          # N % 4
    assert lib.capf_op_wgrad(None, F, F, 16, 64, 64, F, 1) == UNSUPPORTED                         # two pieces: N, K % 128
    pack = lambda name, *dims: getattr(lib, name)(None, F, None, None, None, None, 1e-5, F, F, *dims)
    assert pack("capf_op_pack_conv_bf16_rh", 32, 20) == UNSUPPORTED                                # no row-halo channel width for Cin 20
    assert pack("capf_op_pack_conv_bf16_ws", 32, 8) == UNSUPPORTED                                 # Cin % 16
    assert pack("capf_op_pack_conv_f32x3", 6, 32) == UNSUPPORTED                                   # Cout % 4
    assert pack("capf_op_pack_conv_f32h2", 32, 8) == UNSUPPORTED
    assert pack("capf_op_pack_f32h2_gemm", 6, 32, 3, 288) == UNSUPPORTED                           # N % 4
    assert pack("capf_op_pack_f32h2_gemm", 32, 32, 3, 64) == UNSUPPORTED                           # K != ks * ks * Cin


def test_integration_stub_struct_matches_the_header_and_the_binding():
    """INTEGRATION.md's ctypes stub, include/capf.h's capf_config and capf.lib.CapfConfig must list the same fields in the
    same order (round 1 shipped a stub one field short: the library would have read past the caller's struct)."""
    import ctypes, os, re
    from capf.lib import CapfConfig
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    bound = [n for n, _ in CapfConfig._fields_]
    header = open(os.path.join(root, "include", "capf.h")).read()
    body = header[header.index("typedef struct capf_config {"):header.index("} capf_config;")]
    decl = []
    for line in body.splitlines()[1:]:
        m = re.match(r"\s*int32_t\s+([^;]+);", line)
        if m:
            decl += [re.sub(r"\[\d+\]", "", v).strip() for v in m.group(1).split(",")]
    assert decl == bound
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    stub = doc[doc.index("class capf_config(ctypes.Structure)"):doc.index("class CA_PF(nn.Module):")]
    assert re.findall(r'\("(\w+)", ctypes\.c_int32', stub) == bound
    assert ctypes.sizeof(CapfConfig) == 4 * 24
    ctor = re.search(r"c = capf_config\(([^\n]*)\)\s+#", doc).group(1)
    assert len(re.sub(r"\([^)]*\)", "T", ctor).split(",")) == len(bound)


def test_hot_kernels_do_not_spill_registers():
    """Build guard: a spilling MFMA kernel still produces right answers, 5-8x slower (scratch traffic and slow dispatch) --
    the grouped bf16 kernel once went from 16600 to 2000 frames/s that way.  Compile the conv / GEMM sources to assembly for
    gfx950 and require vgpr_spill_count == 0 for every kernel.  (Not in the list: igemm_bf16_ws -- igemm_bf16_group_ws_kernel reports
    vgpr_count 256, vgpr_spill_count 17, 52 bytes of scratch with this toolchain; known, and to be fixed on its own.)"""
    import concurrent.futures, re, shutil, subprocess, tempfile
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
        return [(n, c) for n, c in zip(names, counts) if c]

    with concurrent.futures.ThreadPoolExecutor(4) as ex:
        bad = sum(ex.map(spills, ["igemm_bf16", "igemm_f32", "igemm_f32_pw", "igemm_f32_pwchain", "igemm_bf16_pwchain", "igemm_wino",
                                  "igemm_f32x3_ws", "igemm_f32h2_ws", "igemm_f32h2"]), [])
    assert not bad, f"kernels with register spills: {bad}"


def test_plan_flags_select_kernel_families_and_nothing_else_does(monkeypatch):
    """capf_config::plan_flags is the ONLY way to take a kernel family out of the plan: the A/B environment switches of
    earlier rounds are compiled out of the product library (kernels.h diag_env), unknown flag bits are rejected."""
    from capf import Engine
    from capf.lib import PLAN_F32X3_EXACT, PLAN_NO_F32H2_GEMM, PLAN_NO_F32X3, PLAN_NO_FUSED_LIFTER, PLAN_NO_WINOGRAD, CapfError
    from mvn.models import _native

    def kernels(flags, embed=128):
        cfg = _cfg("hrnet_32")
        cfg.model.poseformer.embed_dim_ratio = embed
        eng = Engine(_native.make_capf_config(cfg, 256, 256, plan_flags=flags), device=None)
        return [(n, k) for n, k, _ in eng.op_table(64)]

    base = kernels(0)
    assert any(k == "ctx_attn" for _, k in base) and any(k.startswith("igemm_f32h2_") for _, k in base) and any(k.startswith("igemm_f32h2g") for _, k in base)
    assert not any(k.startswith("igemm_f32x3") for _, k in base)
    exact = kernels(PLAN_F32X3_EXACT)                                       # round 4's tile for the 3x3 convs: the exact three-bf16-piece split
    assert [n for n, k in exact if k.startswith("igemm_f32x3")] == [n for n, k in base if k.startswith("igemm_f32h2_")]
    no_x3 = kernels(PLAN_NO_F32X3)                                          # 3x3 convs on the Winograd kernels at every batch
    assert any(k.startswith("igemm_wino") for _, k in no_x3) and not any(k.startswith(("igemm_f32x3", "igemm_f32h2_")) for _, k in no_x3)
    no_g = kernels(PLAN_NO_F32H2_GEMM)                                      # the other convs / linears on the fp32 matrix pipe
    assert not any(k.startswith("igemm_f32h2g") for _, k in no_g) and [n for n, k in no_g if k.startswith("igemm_f32h2_")] == [n for n, k in base if k.startswith("igemm_f32h2_")]
    r3 = kernels(PLAN_NO_F32X3 | PLAN_NO_F32H2_GEMM)                        # round 3's plan: everything on the fp32 pipe
    assert not any(k.startswith(("igemm_f32x3", "igemm_f32h2")) for _, k in r3)
    for var in ("CAPF_LIFTER_FUSED", "CAPF_WINO", "CAPF_BF16_RH", "CAPF_WINO_F43", "CAPF_F32X3_MIN_MFLOP"):
        monkeypatch.setenv(var, "0")
    assert kernels(0) == base                                               # the environment does not reach the product plan
    unfused = kernels(PLAN_NO_FUSED_LIFTER)
    assert not any(k in ("ctx_attn", "embed") for _, k in unfused) and any(k == "deform_sample" for _, k in unfused)
    assert not any(k.startswith(("igemm_wino", "igemm_f32x3", "igemm_f32h2_")) for _, k in kernels(PLAN_NO_WINOGRAD))
    with pytest.raises(CapfError):
        kernels(1 << 14)
    # embed_dim_ratio beyond the fused kernels' register / LDS budget: the plan falls back to one kernel per op
    wide = kernels(0, embed=288)
    assert not any(k in ("ctx_attn", "embed") for _, k in wide) and any(k == "deform_sample" for _, k in wide)


def test_first_bottleneck_plan_bf16_without_a_gpu():
    """bneck_bf16.hip in the plan (no device needed): layer1.0's four convs name one kernel at the baseline batches of the two bf16 configurations,
    CAPF_PLAN_NO_BNECK / fp32 / small batches keep the five launches, and the five tensors the kernel touches never share workspace."""
    from capf import Engine
    from capf.lib import PLAN_NO_BNECK
    from mvn.models import _native
    for backbone, H, W, B, blk in (("cpn", 384, 288, 128, "backbone.resnet.layer1.0"), ("hrnet_48", 256, 256, 256, "backbone.layer1.0")):
        eng = Engine(_native.make_capf_config(_cfg(backbone), H, W, compute_dtype="bf16"), device=None)
        mem = {n: k for n, k, _ in eng.op_table(B) if n.startswith(blk + ".")}
        assert len(mem) == 4 and set(mem.values()) == {"bneck0_bf16<8x8>"}, mem
        ident = {n: k for n, k, _ in eng.op_table(B) if ".layer1." in n and not n.startswith(blk + ".")}
        assert len(ident) in (6, 9) and set(ident.values()) == {"bneck1_bf16<8x8>"}, ident       # (the identity blocks: conv1, conv2, conv3 + x per launch)
        assert not any(k == "bneck0_bf16<8x8>" for _, k, _ in eng.op_table(2))
        off = Engine(_native.make_capf_config(_cfg(backbone), H, W, compute_dtype="bf16", plan_flags=PLAN_NO_BNECK), device=None)
        assert not any(k.startswith("bneck") for _, k, _ in off.op_table(B))
        f32 = Engine(_native.make_capf_config(_cfg(backbone), H, W), device=None)
        assert not any(k.startswith("bneck") for _, k, _ in f32.op_table(B))
        # the block's conv1 / conv2 / shortcut are checkpointed behind its conv3 (the layer-wise tests read them from the TAP kernel's stores)
        names = [n for n, _, _ in eng.op_table(B)]
        c3 = names.index(blk + ".conv3")
        for m in ("conv1", "conv2", "downsample.0"):
            assert eng.op_describe(names.index(f"{blk}.{m}")).checkpoint == c3 + 1


def test_executed_flops_of_winograd_ops_are_half_or_two_thirds_of_the_algorithmic_count():
    from capf import Engine
    from mvn.models import _native
    eng = Engine(_native.make_capf_config(_cfg("hrnet_32"), 256, 256), device=None)
    # batch 64: the branch convs run the split-fp32 tile -- three fp16 piece products per fp32 product (six bf16 ones under
    # CAPF_PLAN_F32X3_EXACT), counted on the 16-bit pipe
    t64, e64 = eng.op_table(64), eng.op_executed_flops(64)
    assert any(k.startswith("igemm_f32h2_") for _, k, _ in t64) and any(k.startswith("igemm_f32h2g") for _, k, _ in t64)
    assert all(abs(e / a - 3.0) < 1e-9 for (n, k, a), e in zip(t64, e64) if k.startswith("igemm_f32h2_"))
    assert all(3.0 - 1e-9 <= e / a <= 3.6 for (n, k, a), e in zip(t64, e64) if k.startswith("igemm_f32h2g"))        # (K padded to 32)
    from capf.lib import PLAN_NO_F32H2_GEMM, PLAN_NO_F32X3, PLAN_F32X3_EXACT
    eng_x = Engine(_native.make_capf_config(_cfg("hrnet_32"), 256, 256, plan_flags=PLAN_F32X3_EXACT), device=None)
    t64, e64 = eng_x.op_table(64), eng_x.op_executed_flops(64)
    assert any(k.startswith("igemm_f32x3") for _, k, _ in t64)
    assert all(abs(e / a - 6.0) < 1e-9 for (n, k, a), e in zip(t64, e64) if k.startswith("igemm_f32x3"))
    eng_w = Engine(_native.make_capf_config(_cfg("hrnet_32"), 256, 256, plan_flags=PLAN_NO_F32X3 | PLAN_NO_F32H2_GEMM), device=None)
    table, ex = eng_w.op_table(32), eng_w.op_executed_flops(32)
    seen = set()
    for (name, kern, alg), e in zip(table, ex):
        if kern.startswith("igemm_wino"):
            r = e / alg
            assert abs(r - 0.5) < 1e-9 or abs(r - 2.0 / 3.0) < 1e-9, (name, r)
            seen.add(round(r, 3))
        elif kern.startswith("igemm") and alg > 0:
            assert 1.0 - 1e-9 <= e / alg <= 1.2, (name, kern, e / alg)       # K padded to the chunk width only
    assert 0.5 in seen
    # below the Winograd batch threshold the same ops run the direct kernel: executed == algorithmic
    t1, e1 = eng.op_table(1), eng.op_executed_flops(1)
    assert all(abs(e / a - 1.0) < 0.2 for (n, k, a), e in zip(t1, e1) if k.startswith("igemm") and a > 0)


def test_sync_batchnorm_conversion_keeps_the_reference_state_dict():
    """train.py:317-318 on the host mirror (CPU part; the GPU box checks that the engine binds the converted tree)."""
    import contextlib, io
    import torch
    from mvn.models.conpose import CA_PF
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "schema_hrnet_32.json")))
    with contextlib.redirect_stdout(io.StringIO()):
        m = CA_PF(_cfg("hrnet_32"))
    m = torch.nn.SyncBatchNorm.convert_sync_batchnorm(m)
    assert {k: list(v.shape) for k, v in m.state_dict().items()} == want
    assert sum(isinstance(x, torch.nn.SyncBatchNorm) for x in m.modules()) == 292
    assert not any(p.requires_grad for p in m.backbone.parameters())


def test_depth_is_a_plan_parameter_of_the_variant_without_context_blocks():
    """capf_config.depth (ContextPose_mpi/model/pose_dformer.py:199): blocks per group of the MPI-INF-3DHP lifter.  0 = levels;
    the H36M model and the training path are built for depth == levels only and say so."""
    from capf import Engine
    from capf.lib import CapfError
    from mvn.models import _native

    def plan(depth, context_blocks, training=0):
        c = _native.make_capf_config(_cfg("hrnet_32"), 256, 192, context_blocks=context_blocks)
        c.depth, c.training = depth, training
        eng = Engine(c, device=None)
        names = [n for n, _, _ in eng.op_table(2)]
        chain_flops.append(sum(f for n, _, f in eng.op_table(2) if n == "res.chain"))
        schema = [s[0] for s in eng.schema()]
        eng.close()
        return names, schema

    chain_flops = []
    for depth, want in ((0, 4), (4, 4), (2, 2), (6, 6)):
        names, schema = plan(depth, False)
        # (round 6: the res blocks of any depth are ONE launch, lifter_chain.hip -- its FLOPs count the blocks)
        assert names.count("res.chain") == 1 and chain_flops[-1] > 0 and abs(chain_flops[-1] / want - chain_flops[0] / 4) < 1e-6 * chain_flops[0]
        assert sum(n.endswith(".qkv") and n.startswith("joint") for n in names) == want
        assert sum(s.endswith("attn.qkv.weight") for s in schema) == 2 * want
    for bad in ((2, True, 0), (2, False, 1), (9, False, 0), (-1, False, 0)):
        with pytest.raises(CapfError):
            plan(*bad)


def test_a_lifter_row_wider_than_the_layernorm_kernels_hold_is_refused_at_creation():
    """Engine::build (csrc/plan.cpp): embed_dim_ratio * (levels + 1) <= 1536 -- the LayerNorm and head launchers (lifter.hip, train_kernels.hip)
    hold a joint row in 24 values per lane and return a bare HIP error for a wider one, so 320 is refused when the plan is made, for
    inference and training plans alike, with the reason in capf_last_error(NULL); 288 is the widest plan.  No forward runs here."""
    from capf import Engine
    from capf.lib import CapfError, load_library
    from mvn.models import _native

    def config(embed, training):
        cfg = _cfg("hrnet_32")
        cfg.model.poseformer.embed_dim_ratio = embed
        c = _native.make_capf_config(cfg, 128, 96)
        c.training = training
        return c

    for training in (0, 1):
        with pytest.raises(CapfError, match=r"must not exceed 1536.*LayerNorm and head kernels.*24 values per lane"):
            Engine(config(320, training), device=None)
        assert b"24 values per lane" in load_library().capf_last_error(None)
        eng = Engine(config(288, training), device=None)
        assert dict((n, s) for n, s, _ in eng.schema())["volume_net.Spatial_pos_embed"][-1] == 288
        assert eng.workspace_bytes(2) > 0
        eng.close()


@pytest.mark.parametrize("backbone", ["hrnet_32", "hrnet_48", "cpn"])
def test_two_piece_table_of_a_training_plan_follows_the_restated_rule_at_every_width(backbone):
    """capf_train_h2_matrices of a plan-only engine == the rule tests/test_gpu_train_widths.py restates from t_h2_plan (csrc/train.cpp), at
    every embed_dim_ratio % 32 == 0 up to 288; none under bf16."""
    from capf import Engine
    from mvn.models import _native
    from test_gpu_train_widths import MAP_CHANNELS, WIDTHS, h2_table
    for dtype in ("fp32", "bf16"):
        for embed in WIDTHS:
            cfg = _cfg(backbone)
            cfg.model.poseformer.embed_dim_ratio = embed
            eng = Engine(_native.make_capf_config(cfg, 128, 96, compute_dtype=dtype), device=None)
            want = h2_table(embed, MAP_CHANNELS[backbone], dtype)
            assert eng.lib.capf_train_h2_matrices(eng.h) == len(want), (dtype, embed)
            assert (len(want) == 0) == (dtype == "bf16")
            eng.close()


# ---- the binding's prototype table, struct mirrors and constants against include/capf.h ------------------------------------------------
def parse_header(text):
    """include/capf.h -> (functions {name: (return type, [parameter type])} in declaration order,
                          structs {name: [(field, type, array extents)]},
                          constants {name: value} of every CAPF_* enumerator and #define).
    A type is (base type without const, pointer depth); an array parameter counts as a pointer to its element."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    consts = {m.group(1): int(m.group(2), 0) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(CAPF_\w+)[ \t]+(-?\w+)[ \t]*$", text, flags=re.M)}
    text = re.sub(r"^[ \t]*#[^\n]*$", ";", text, flags=re.M)          # a directive ends a statement: it cannot run into the next declaration
    text = re.sub(r'extern\s+"C"\s*\{', ";", text)

    def typ(decl):
        """'const float* const feat[4]' -> ('feat', ('float', 1), [4])"""
        extents = [int(v) for v in re.findall(r"\[(\d+)\]", decl)]
        words = re.sub(r"\[\d+\]", " ", decl).replace("*", " * ").split()
        depth = words.count("*")
        words = [w for w in words if w not in ("*", "const", "struct")]
        return words[-1], (" ".join(words[:-1]), depth), extents

    depth, stmt, stmts = 0, "", []
    for ch in text:                                                   # statements: split at the semicolons outside braces
        if ch == "}" and depth == 0:
            continue                                                  # (the brace that closes extern "C")
        depth += (ch == "{") - (ch == "}")
        if ch == ";" and depth == 0:
            stmts.append(" ".join(stmt.split()))
            stmt = ""
        else:
            stmt += ch
    funcs, structs = {}, {}
    for s in stmts:
        m = re.fullmatch(r"enum \w+ \{(.*)\}", s)
        if m:
            nxt = 0
            for item in filter(None, (v.strip() for v in m.group(1).split(","))):
                name, _, val = (v.strip() for v in item.partition("="))
                consts[name] = nxt = int(val, 0) if val else nxt
                nxt += 1
            continue
        m = re.fullmatch(r"typedef struct (capf_\w+) \{(.*)\} \1", s)
        if m:
            fields = structs[m.group(1)] = []
            for decl in filter(None, (v.strip() for v in m.group(2).split(";"))):
                first, *more = (v.strip() for v in decl.split(","))
                fields.append(typ(first))
                fields += [typ(fields[-1][1][0] + " " + v) for v in more]        # "int32_t height, width": one base type, several names
            continue
        m = re.fullmatch(r"(.*?)\b(capf_\w+) ?\((.*)\)", s)
        if m and not s.startswith("typedef"):
            params = [] if m.group(3).strip() == "void" else [typ(p) for p in m.group(3).split(",")]
            funcs[m.group(2)] = (typ(m.group(1) + " _")[1], [(base, d + len(ext)) for _, (base, d), ext in params])
    return funcs, structs, consts


_HEADER = []


def _header():
    if not _HEADER:
        _HEADER.append(parse_header(open(os.path.join(ROOT, "include", "capf.h")).read()))
    return _HEADER[0]


def _mirrors():
    """{header struct name: ctypes.Structure of capf.lib}: CapfConfig -> capf_config, OpDesc -> capf_op_desc, ..."""
    from capf import lib as capf_lib
    snake = lambda n: "capf_" + re.sub(r"(?<!^)([A-Z])", r"_\1", n[4:] if n.startswith("Capf") else n).lower()
    return {snake(n): c for n, c in vars(capf_lib).items()
            if isinstance(c, type) and issubclass(c, ctypes.Structure) and c.__module__ == capf_lib.__name__}


def _scalar(base):
    return {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "size_t": ctypes.c_size_t, "float": ctypes.c_float,
            "double": ctypes.c_double, "int16_t": ctypes.c_int16, "uint16_t": ctypes.c_uint16, "uint8_t": ctypes.c_uint8}.get(base)


def _type_fault(bound, base, depth, mirrors):
    """None when the ctypes type `bound` may stand for the header type (base, depth), else what is wrong with it"""
    if depth == 0:
        want = None if base == "void" else _scalar(base)
        return None if bound is want else f"{base} bound as {getattr(bound, '__name__', bound)}"
    if bound is ctypes.c_void_p:                                       # a device pointer, a void*, an opaque handle; any address
        return None
    if bound is ctypes.c_char_p:                                       # a string or bytes
        return None if depth == 1 and base in ("char", "uint8_t") else f"{base}{'*' * depth} bound as c_char_p"
    if isinstance(bound, type) and issubclass(bound, ctypes._Pointer):
        pointee = bound._type_
        if depth > 1:
            return _type_fault(pointee, base, depth - 1, mirrors)
        if pointee is (mirrors.get(base) or _scalar(base)):
            return None
        return f"{base}* bound as POINTER({pointee.__name__})"
    return f"{base}{'*' * depth} bound as {getattr(bound, '__name__', bound)}, which is no pointer"


def prototype_faults(table, funcs, mirrors):
    """[(function, what is wrong)] of a prototype table against the header's functions: return type, argument count, kind per position,
    pointee of every POINTER(T)"""
    faults = [(n, "not in the header") for n in table if n not in funcs]
    for name, (ret, params) in funcs.items():
        if name not in table:
            faults.append((name, "no row"))
            continue
        (restype, argtypes) = table[name]
        bad = _type_fault(restype, *ret, mirrors)
        if ret == ("char", 1) and restype is not ctypes.c_char_p:      # a string result is read, not passed on: c_void_p will not do
            bad = f"char* returned as {getattr(restype, '__name__', restype)}"
        if bad:
            faults.append((name, "result: " + bad))
        if len(argtypes) != len(params):
            faults.append((name, f"{len(params)} parameters, {len(argtypes)} argtypes"))
            continue
        faults += [(name, f"argument {i}: {bad}") for i, (t, p) in enumerate(zip(argtypes, params)) for bad in [_type_fault(t, *p, mirrors)] if bad]
    return faults


def test_prototype_table_follows_the_header():
    from capf.lib import EXPORTS, PROTOTYPES
    funcs, _, _ = _header()
    assert len(funcs) > 100
    assert list(PROTOTYPES) == list(funcs) == EXPORTS                  # one row per declaration, in the header's order
    assert all(isinstance(a, list) for _, a in PROTOTYPES.values())
    assert prototype_faults(PROTOTYPES, funcs, _mirrors()) == []


def _mutate(name, index, new):
    """the binding's table with argument `index` of one row replaced ("last": dropped; "result": its restype replaced)"""
    from capf.lib import PROTOTYPES
    table = dict(PROTOTYPES)
    (restype, argtypes) = table[name]
    if index == "result":
        table[name] = (new, argtypes)
    elif index == "last":
        table[name] = (restype, argtypes[:-1])
    else:
        table[name] = (restype, argtypes[:index] + [new] + argtypes[index + 1:])
    return table


@pytest.mark.parametrize("name,index,new,header", [
    ("capf_optim_ctrl_init", 2, "c_int", ("int64_t", 0)),              # an int64_t argument bound as c_int
    ("capf_set_workspace", "last", None, ("size_t", 0)),               # a missing last argument
    ("capf_workspace_bytes", "result", "c_int", ("size_t", 0)),        # a size_t result on c_int
    ("capf_preprocess", 5, "pI32", ("float", 1)),                      # POINTER(c_int32) where the header has float*
], ids=["int64-as-int", "missing-last-argument", "size_t-result-as-int", "float-pointer-as-int32-pointer"])
def test_prototype_comparison_reports_a_planted_fault_and_nothing_else(name, index, new, header):
    funcs, _, _ = _header()
    ret, params = funcs[name]
    assert (ret if index == "result" else params[-1 if index == "last" else index]) == header      # the row is what the case says it is
    new = {"c_int": ctypes.c_int, "pI32": ctypes.POINTER(ctypes.c_int32), None: None}[new]
    faults = prototype_faults(_mutate(name, index, new), funcs, _mirrors())
    assert faults and {n for n, _ in faults} == {name}, faults


def test_loaded_library_carries_exactly_the_table():
    import capf
    from capf.lib import PROTOTYPES
    lib = capf.load_library()
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(lib, name)
        assert fn.restype is restype, name
        assert fn.argtypes is not None and len(fn.argtypes) == len(argtypes) and all(a is b for a, b in zip(fn.argtypes, argtypes)), name


def test_struct_mirrors_follow_the_header():
    _, structs, _ = _header()
    mirrors = _mirrors()
    assert set(mirrors) == set(structs) and len(structs) == 5         # every header struct has a mirror and the reverse (capf_handle is opaque)

    def ctype(base, depth, extents):
        t = ctypes.c_void_p if depth else _scalar(base)
        for n in reversed(extents):
            t = t * n
        return t

    def same(a, b):
        if isinstance(a, type) and issubclass(a, ctypes.Array):
            return isinstance(b, type) and issubclass(b, ctypes.Array) and a._length_ == b._length_ and same(a._type_, b._type_)
        return a is b

    for name, fields in structs.items():
        bound = mirrors[name]._fields_
        assert [f[0] for f in bound] == [f[0] for f in fields], name
        for (field, t), (_, (base, depth), extents) in zip(bound, fields):
            assert same(t, ctype(base, depth, extents)), (name, field, t)


def test_constants_follow_the_header():
    from capf import lib as capf_lib
    _, _, consts = _header()
    named = {n: v for n, v in vars(capf_lib).items() if "CAPF_" + n in consts}
    assert {"HRNET", "CPN50", "F32", "BF16", "F16", "ABI_VERSION", "OPTIM_MAX_SEGMENTS"} <= set(named)
    assert {n for n in named if n.startswith("PLAN_")} == {n[5:] for n in consts if n.startswith("CAPF_PLAN_")}
    for n, v in named.items():
        assert v == consts["CAPF_" + n], n
    assert capf_lib.PARAM_KINDS == {v: n[len("CAPF_P_"):].lower() for n, v in consts.items() if n.startswith("CAPF_P_")}
