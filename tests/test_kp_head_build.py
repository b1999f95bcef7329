"""CPU build guard for csrc/kp_head.hip: every kernel of the keypoint head -- the single forward, its flip-test PAIR instantiations (two logit
passes per tile and the swap table in the kernel arguments) and the backward -- compiles for gfx950 without spilling vector registers.
The recipe of tests/test_abi.py::test_hot_kernels_do_not_spill_registers, whose list does not include this file."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_keypoint_head_kernels_do_not_spill_registers():
    hipcc = shutil.which("hipcc")
    if hipcc is None:
        pytest.skip("hipcc not on PATH")
    csrc = os.path.join(ROOT, "contextaware-poseformer_amd", "csrc")
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "kp_head.s")
        subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                        "-S", "--cuda-device-only", os.path.join(csrc, "kp_head.hip"), "-o", out],
                       check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        text = open(out).read()
    names = re.findall(r"^\s+\.name:\s+(\S+)", text, flags=re.M)
    counts = [int(v) for v in re.findall(r"^\s+\.vgpr_spill_count:\s+(\d+)", text, flags=re.M)]
    assert len(names) == len(counts) and counts
    # the pair forms are in the object: slab + combine x two decodes x three map dtypes, beside as many single forms
    assert sum("kp_fwd_slab_kernel" in n for n in names) == 12 and sum("kp_fwd_combine_kernel" in n for n in names) == 12
    bad = [(n, c) for n, c in zip(names, counts) if c]
    assert not bad, f"kernels with register spills: {bad}"
