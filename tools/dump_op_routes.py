"""Record this engine's launch routes (which kernel runs each op, and what that op is counted as) for a matrix of plans.

Plans engines with Engine(cfg, device=None) -- no GPU -- and stores, per (geometry, dtype, plan flags) and batch, what
capf_op_info (kernel name, algorithmic FLOPs), capf_op_bytes and capf_op_executed_flops report for every op.  The output is
tests/golden/op_routes.npz and, for the small-map matrix (SMALL_*), tests/golden/op_routes_small.npz, which
tests/test_op_routes.py compares against exactly.  They come from this engine's own plan (the C ABI of libcapf.so), not from
the reference model.  A third matrix (ROUTE16_*) scans the 16-bit plans batch by batch -- every batch 1 .. 64, where the 2-D halo
tile of the bf16 / fp16 3x3 convs takes over, and each plan's two batches around the tile's 2 GB addressing limit -- into
tests/golden/op_routes_16bit.npz; its batch list differs per plan and is stored per plan (`<plan>.batches`).

    python tools/dump_op_routes.py [--which all|main|small|16bit] [--find-caps]

--find-caps prints, per plan of the third matrix, the batch at which its first conv leaves the 2-D halo tile for the limit (what
ROUTE16_PLANS holds).  Every run reports, per plan of the third matrix, the ops whose tile batches in the scan have a hole (none may:
a conv's tile batches are one range, Engine::build finds its two ends).

Kernel and op names are stored once, as indices into the string list `strings`; `base_commit` names the commit the file was
made at.
"""
import argparse
import copy
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "contextaware-poseformer_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

BATCHES = (1, 2, 4, 5, 8, 16, 23, 24, 48, 64, 128, 256, 512)   # straddle H2G_MIN_BATCH, wino_min_batch and the bneck 64 Ki-pixel rule
GEOMETRIES = (("hrnet_32", 256, 256, ("fp32", "bf16")), ("hrnet_32", 256, 192, ("fp32", "bf16")),
              ("hrnet_48", 256, 256, ("bf16",)), ("cpn", 384, 288, ("bf16",)))
# Small maps (HRNet-32 branches of 16 x 16 .. 2 x 2 and 24 x 24 .. 3 x 3 pixels), a matrix and a file of their own: the split-fp32 tile takes
# them late (64 x 64: from batch 79, 96 x 96: from batch 36) and the Winograd kernels run them from batch 24 -- levels that mix an F(4,3)
# group with a lone F(2,3) conv (W = 2) and, at 96 x 96, with the two-piece GEMM as well (W = 3 is odd)
SMALL_BATCHES = (1, 4, 5, 16, 23, 24, 35, 36, 48, 64, 78, 79, 80, 128, 512)
SMALL_GEOMETRIES = (("hrnet_32", 64, 64, ("fp32",)), ("hrnet_32", 96, 96, ("fp32",)))
SMALL_FLAGS = {"fp32": ("0", "F32X3_EXACT", "NO_F32X3")}
FLAGS = {
    "fp32": ("0", "NO_F32X3|NO_F32H2_GEMM", "F32X3_EXACT", "NO_PWCHAIN", "H2_PLANES", "NO_WINOGRAD", "WINOGRAD_F23_ONLY"),
    "bf16": ("0", "NO_BNECK", "NO_WS", "NO_ROW_HALO", "NO_PWCHAIN", "NO_UPADD", "LIFTER_FP32"),
}
# The 16-bit plans, batch by batch: the 2-D halo tile (igemm_bf16_ws.hip) takes a 3x3 stride-1 conv from 1 GFLOP and batch 24 (23 | 24; the
# 128 x 128 branch convs cross 1 GFLOP at 52 | 53) up to its 2 GB limit.  Last: the batch at which the plan's first conv leaves the tile for
# that limit (--find-caps) and the one before.  In the 256 x 256 HRNet plans that conv is transition1's 256 -> 32 one (a 16-bit input of
# 64 x 64 x 256 per frame, in the fp32-stream plan too); 3814 | 3815 is where the fp32-stream plan's branch-0 BasicBlock convs leave (fp32
# residual rows: half the bf16 plan's 7629), recorded for the bf16 plan as well, where they stay
ROUTE16_COMMON = tuple(range(1, 65)) + (128, 256, 512)
ROUTE16_PLANS = (("hrnet_32", 256, 256, "bf16", "0", (953, 954, 3814, 3815)), ("hrnet_32", 256, 256, "fp16", "0", (953, 954)),
                 ("hrnet_32", 256, 256, "bf16", "BF16_F32_STREAM", (953, 954, 3814, 3815)), ("hrnet_48", 256, 256, "bf16", "0", (953, 954)),
                 ("cpn", 384, 288, "bf16", "0", (4521, 4522)), ("hrnet_32", 128, 128, "bf16", "0", (3814, 3815)))
TILE_KERNEL = re.compile(r"^igemm_\w+_ws<")


def _flag_bits(spec):
    from capf import lib
    return 0 if spec == "0" else sum(getattr(lib, "PLAN_" + f) for f in spec.split("|"))


def cases(geometries=GEOMETRIES, flags=FLAGS):
    """[(case key, backbone, height, width, dtype, plan flags spec)]"""
    out = []
    for bb, h, w, dtypes in geometries:
        for dt in dtypes:
            for fl in flags[dt]:
                out.append((f"{bb}_{h}x{w}_{dt}_{fl}", bb, h, w, dt, fl))
    return out


def small_cases():
    return cases(SMALL_GEOMETRIES, SMALL_FLAGS)


def route16_cases():
    return [(f"{bb}_{h}x{w}_{dt}_{fl}", bb, h, w, dt, fl) for bb, h, w, dt, fl, _ in ROUTE16_PLANS]


def route16_batches():
    """{case key: its batches} -- the common scan and the plan's batches around the 2 GB limit"""
    return {f"{bb}_{h}x{w}_{dt}_{fl}": ROUTE16_COMMON + caps for bb, h, w, dt, fl, caps in ROUTE16_PLANS}


def _engine(bb, h, w, dt, fl):
    from capf.lib import Engine
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    return Engine(_native.make_capf_config(backbone_preset(copy.deepcopy(config), bb), h, w, compute_dtype=dt, plan_flags=_flag_bits(fl)), device=None)


def find_caps():
    """per plan of the third matrix: the first batch above 512 at which fewer convs run the 2-D halo tile than at 512 (bisection: above
    512 every conv the size rule admits is in, and a conv that left for the 2 GB limit stays out)"""
    out = {}
    for key, bb, h, w, dt, fl in route16_cases():
        eng = _engine(bb, h, w, dt, fl)
        count = lambda b: sum(bool(TILE_KERNEL.match(t[1])) for t in eng.op_table(b))
        lo, hi, full = 512, 100000, count(512)
        assert full > 0 and count(hi) < full, key
        while hi - lo > 1:
            mid = (lo + hi) // 2
            lo, hi = (mid, hi) if count(mid) == full else (lo, mid)
        out[key] = hi
        eng.close()
    return out


def tile_batch_holes(res, batches):
    """[(case key, op name)] whose batches on the 2-D halo tile, among the scanned ones in ascending order, are not consecutive"""
    bad = []
    for key, (ops, kern, *_rest) in res.items():
        order = np.argsort(batches[key] if isinstance(batches, dict) else batches)
        for i, op in enumerate(ops):
            on = [bool(TILE_KERNEL.match(kern[b][i])) for b in order]
            if any(on) and not all(on[on.index(True):len(on) - on[::-1].index(True)]):
                bad.append((key, op))
    return bad


def collect(case_list=None, batches=BATCHES):
    """{case key: (op names, kernel names [batch][op], flops, bytes, executed flops)} for every case of the matrix; batches: one list, or
    {case key: list}"""
    res = {}
    for key, bb, h, w, dt, fl in cases() if case_list is None else case_list:
        eng = _engine(bb, h, w, dt, fl)
        ops, kern, flops, nbytes, execf = None, [], [], [], []
        for b in batches[key] if isinstance(batches, dict) else batches:
            tab = eng.op_table(b)
            if ops is None:
                ops = [t[0] for t in tab]
            kern.append([t[1] for t in tab])
            flops.append([t[2] for t in tab])
            nbytes.append(eng.op_bytes(b))
            execf.append(eng.op_executed_flops(b))
        eng.close()
        res[key] = (ops, kern, flops, nbytes, execf)
    return res


def to_arrays(res, batches=BATCHES):
    strings, index = [], {}

    def idx(s):
        if s not in index:
            index[s] = len(strings)
            strings.append(s)
        return index[s]

    arrs = {}
    for key, (ops, kern, flops, nbytes, execf) in res.items():
        arrs[key + ".op"] = np.array([idx(s) for s in ops], dtype=np.int32)
        arrs[key + ".kernel"] = np.array([[idx(s) for s in row] for row in kern], dtype=np.int32)
        arrs[key + ".flops"] = np.array(flops, dtype=np.float64)
        arrs[key + ".bytes"] = np.array(nbytes, dtype=np.float64)
        arrs[key + ".executed_flops"] = np.array(execf, dtype=np.float64)
        if isinstance(batches, dict):
            arrs[key + ".batches"] = np.array(batches[key], dtype=np.int32)
    arrs["strings"] = np.array(strings)
    arrs["batches"] = np.array(ROUTE16_COMMON if isinstance(batches, dict) else batches, dtype=np.int32)
    return arrs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "op_routes.npz"))
    ap.add_argument("--out-small", default=os.path.join(ROOT, "tests", "golden", "op_routes_small.npz"))
    ap.add_argument("--out-16bit", default=os.path.join(ROOT, "tests", "golden", "op_routes_16bit.npz"))
    ap.add_argument("--which", choices=("all", "main", "small", "16bit"), default="all")
    ap.add_argument("--find-caps", action="store_true")
    args = ap.parse_args()
    if args.find_caps:
        for key, cap in find_caps().items():
            print(f"{key}: first conv leaves the 2-D halo tile at batch {cap}")
        return
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    for which, out, case_list, batches in (("main", args.out, cases(), BATCHES), ("small", args.out_small, small_cases(), SMALL_BATCHES),
                                           ("16bit", args.out_16bit, route16_cases(), route16_batches())):
        if args.which not in ("all", which):
            continue
        res = collect(case_list, batches)
        arrs = to_arrays(res, batches)
        arrs["base_commit"] = np.array(commit or "unknown")
        np.savez_compressed(out, **arrs)
        nb = len(next(iter(batches.values()))) if isinstance(batches, dict) else len(batches)
        print(f"{out}: {len(case_list)} plans x {nb} batches, {len(arrs['strings'])} strings, base {commit[:12]}")
        if which == "16bit":
            holes = tile_batch_holes(res, batches)
            print(f"ops whose 2-D halo tile batches have a hole: {holes or 'none'}")


if __name__ == "__main__":
    main()
