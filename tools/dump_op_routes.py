"""Record this engine's launch routes (which kernel runs each op, and what that op is counted as) for a matrix of plans.

Plans engines with Engine(cfg, device=None) -- no GPU -- and stores, per (geometry, dtype, plan flags) and batch, what
capf_op_info (kernel name, algorithmic FLOPs), capf_op_bytes and capf_op_executed_flops report for every op.  The output is
tests/golden/op_routes.npz and, for the small-map matrix (SMALL_*), tests/golden/op_routes_small.npz, which
tests/test_op_routes.py compares against exactly.  They come from this engine's own plan (the C ABI of libcapf.so), not from
the reference model.

    python tools/dump_op_routes.py [--out tests/golden/op_routes.npz] [--out-small tests/golden/op_routes_small.npz]

Kernel and op names are stored once, as indices into the string list `strings`; `base_commit` names the commit the file was
made at.
"""
import argparse
import copy
import os
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


def collect(case_list=None, batches=BATCHES):
    """{case key: (op names, kernel names [batch][op], flops, bytes, executed flops)} for every case of the matrix"""
    from capf.lib import Engine
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    res = {}
    for key, bb, h, w, dt, fl in cases() if case_list is None else case_list:
        c = _native.make_capf_config(backbone_preset(copy.deepcopy(config), bb), h, w, compute_dtype=dt, plan_flags=_flag_bits(fl))
        eng = Engine(c, device=None)
        ops, kern, flops, nbytes, execf = None, [], [], [], []
        for b in batches:
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
    arrs["strings"] = np.array(strings)
    arrs["batches"] = np.array(batches, dtype=np.int32)
    return arrs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "op_routes.npz"))
    ap.add_argument("--out-small", default=os.path.join(ROOT, "tests", "golden", "op_routes_small.npz"))
    args = ap.parse_args()
    commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "HEAD"], capture_output=True, text=True).stdout.strip()
    for out, case_list, batches in ((args.out, cases(), BATCHES), (args.out_small, small_cases(), SMALL_BATCHES)):
        arrs = to_arrays(collect(case_list, batches), batches)
        arrs["base_commit"] = np.array(commit or "unknown")
        np.savez_compressed(out, **arrs)
        print(f"{out}: {len(case_list)} plans x {len(batches)} batches, {len(arrs['strings'])} strings, base {commit[:12]}")


if __name__ == "__main__":
    main()
