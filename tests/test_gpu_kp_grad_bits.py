"""GPU: the gradients of the 2-D keypoint head, bit for bit what the recorded commit's library wrote (tests/golden/kp_grad_bits.json, made by
tools/make_kp_grad_bits.py; the cases and why these shapes: tests/kp_grad_bits_cases.py).  The two entries share one gradient kernel body and
one reduce; their summation orders are part of include/capf.h, and a change of either shows here as a digest that moved."""
import functools
import json
import os

import pytest

import kp_grad_bits_cases as G

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(os.path.join(ROOT, "tests", "golden", "kp_grad_bits.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("group", ["backward", "loss"])
def test_gradient_bits_are_the_parent_s(group):
    """every output of every case is finite (kp_grad_bits_cases.digest asserts it) and has the recorded digest"""
    rec = _recorded()
    want = {k: v for k, v in rec["digests"].items() if k.startswith(group + "/")}
    cases = list(G.backward_cases() if group == "backward" else G.loss_cases())
    assert sorted(want) == sorted(c[0] for c in cases)                 # the fixture holds exactly the cases of the list
    run = G.run_backward if group == "backward" else G.run_loss
    differ = []
    for key, *case in cases:
        got = {k: G.digest(v) for k, v in run(*case).items()}
        assert sorted(got) == sorted(want[key]), key                    # the same outputs, none missing
        differ += [f"{key}: {k}" for k in sorted(got) if got[k] != want[key][k]]
    print(f"{group}: {len(cases)} cases, {len(differ)} outputs differ from commit {rec['commit']}")
    assert not differ, differ
