"""CPU: the engine's launch routes -- the kernel capf_op_info names for every op, its algorithmic FLOPs, capf_op_bytes and
capf_op_executed_flops -- equal tests/golden/op_routes.npz exactly, for every plan and batch of tools/dump_op_routes.py's matrix
(HRNet-32 / HRNet-48 / CPN, fp32 and bf16, the plan flags that move routes, batches 1 .. 512), and tests/golden/op_routes_small.npz
for its small-map matrix (HRNet-32 fp32 at 64 x 64 and 96 x 96: levels that mix the F(4,3) and F(2,3) Winograd kernels and the
two-piece GEMM, and the batches at which the split-fp32 tile takes over), and tests/golden/op_routes_16bit.npz for its 16-bit
matrix (HRNet-32 bf16 / fp16 / bf16 with an fp32 stream, HRNet-48 and CPN bf16, HRNet-32 bf16 at 128 x 128; every batch 1 .. 64,
128 .. 512, and each plan's batches around the 2 GB limit of the 2-D halo tile: where that tile takes a conv and where it lets go).
The fixtures come from this engine at the commit they name (`base_commit`), not from the reference.

A change that moves a route on purpose regenerates the fixture and says in its description which rows moved:

    python -c "import __graft_entry__ as g; g.build()" && python tools/dump_op_routes.py
"""
import importlib.util
import os

import numpy as np

from conftest import ROOT, load_golden


def _tool():
    spec = importlib.util.spec_from_file_location("dump_op_routes", os.path.join(ROOT, "tools", "dump_op_routes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_op_routes_match_fixture():
    tool = _tool()
    _compare(load_golden("op_routes"), tool.to_arrays(tool.collect()))


def test_small_map_op_routes_match_fixture():
    tool = _tool()
    want = load_golden("op_routes_small")
    assert 79 in want["batches"] and 80 in want["batches"]      # 64 x 64: the tile's first batch
    _compare(want, tool.to_arrays(tool.collect(tool.small_cases(), tool.SMALL_BATCHES), tool.SMALL_BATCHES))


def test_16bit_op_routes_match_fixture():
    tool = _tool()
    want = load_golden("op_routes_16bit")
    batches = tool.route16_batches()
    for key, b in batches.items():                               # where the tile takes over, and the plan's pair around its 2 GB limit
        assert {23, 24, 52, 53} <= set(b) and b[-1] == b[-2] + 1 and b[-2] > 512, key
    res = tool.collect(tool.route16_cases(), batches)
    assert tool.tile_batch_holes(res, batches) == []             # a conv's tile batches are ONE range (Engine::build finds its two ends)
    _compare(want, tool.to_arrays(res, batches))


def _compare(want, got):
    assert list(want["batches"]) == list(got["batches"])
    ws, gs = want["strings"], got["strings"]
    keys = sorted(k for k in got if "." in k)
    assert keys == sorted(k for k in want.files if "." in k)
    for k in keys:
        w, g = want[k], got[k]
        assert w.shape == g.shape, k
        if k.endswith(".op") or k.endswith(".kernel"):
            bad = np.argwhere(ws[w] != gs[g])
            assert bad.size == 0, f"{k}: {len(bad)} rows differ, first {tuple(bad[0])}: {ws[w][tuple(bad[0])]!r} -> {gs[g][tuple(bad[0])]!r}"
        else:
            bad = np.argwhere(w != g)
            assert bad.size == 0, f"{k}: {len(bad)} values differ, first {tuple(bad[0])}: {w[tuple(bad[0])]!r} -> {g[tuple(bad[0])]!r}"
