"""The cases whose gradient BITS are pinned (tests/golden/kp_grad_bits.json): capf_kp_head_backward and capf_kp_heatmap_loss at the smallest
shapes at which their shared gradient kernel and reduce can go wrong.  tools/make_kp_grad_bits.py records sha256 digests of the outputs with
the library of the commit named in the file; tests/test_gpu_kp_grad_bits.py asserts them on the library under test.  The existing gradient
tests hold these entries to float64 within bounds, which does not show that a refactor left a summation order alone; equal digests do.

Inputs are the seeded ones of the existing suites: kp_head_cases.make_case and test_gpu_kp_head's cotangents for the decode backward,
test_gpu_kp_heatmap_loss's _case (with its NaN ground-truth item and its zero target weights, whose outputs are exact zeros) for the loss.
Everything below needs the GPU; the modules it takes its inputs from are imported on first use."""
import hashlib

import numpy as np

# ---- capf_kp_head_backward: (B, H, W, C, J) ---------------------------------------------------------------------------------------------
BACKWARD_SHAPES = (
    (1, 1, 1, 32, 17),        # one pixel: a tile of n = 1
    (2, 16, 16, 32, 17),      # exactly one full tile
    (3, 17, 16, 48, 17),      # a second tile of 16 pixels; C no power of two in o / C
    (2, 47, 45, 32, 17),      # 2115 pixels = 9 tiles: 2 tiles a block, 5 blocks a frame, the last with one tile of 67 pixels
    (2, 8, 8, 32, 1),         # J at both ends (kp_logits' copy of joint J - 1)
    (2, 8, 8, 32, 32),
    (1, 24, 18, 256, 17),     # J C = 4352 outputs over 256 threads, 272 reduce blocks
)
BACKWARD_WHICH = ("dkcrop", "dk2d", "both")
BACKWARD_BETAS = (1.0, 25.0)
BACKWARD_OUTPUTS = ("dW", "dbias", "dmap")

# ---- capf_kp_heatmap_loss ---------------------------------------------------------------------------------------------------------------
LOSS_BJC = ((1, 1, 4), (3, 17, 32), (3, 32, 48))
LOSS_HW = ((1, 1), (16, 16), (17, 16), (47, 45))
LOSS_REDUCTIONS = ("mean", "ohkm")     # OHKM at topk 8: with J = 17 and 32 some joints are unselected and take the exact-zero path
LOSS_TOPK = 8
LOSS_DTYPES = ("fp32", "bf16", "fp16")  # 16-bit maps: no dmap, the partials read the map one element at a time
LOSS_OUTPUTS = ("loss", "joint_loss", "dweight", "dbias", "dmap")


def backward_cases():
    """(key, shape, which, beta, accumulate)"""
    for shape in BACKWARD_SHAPES:
        for which in BACKWARD_WHICH:
            for beta in BACKWARD_BETAS:
                for accumulate in (0, 1):
                    yield f"backward/{'x'.join(map(str, shape))}/{which}/beta{beta:g}/acc{accumulate}", shape, which, beta, accumulate


def loss_cases():
    """(key, (B, J, C, H, W), reduction, dtype, accumulate); a 16-bit map has no dmap to accumulate into"""
    for B, J, C in LOSS_BJC:
        for H, W in LOSS_HW:
            for reduction in LOSS_REDUCTIONS:
                for dtype in LOSS_DTYPES:
                    for accumulate in ((0, 1) if dtype == "fp32" else (0,)):
                        yield f"loss/B{B}-J{J}-C{C}/{H}x{W}/{reduction}/{dtype}/acc{accumulate}", (B, J, C, H, W), reduction, dtype, accumulate


def digest(a):
    """sha256 of an output's bytes; every digested output is finite"""
    a = np.ascontiguousarray(a)
    assert np.isfinite(a).all()
    return hashlib.sha256(a.tobytes()).hexdigest()


def run_backward(shape, which, beta, accumulate):
    import kp_head_cases as K
    import test_gpu_kp_head as T
    X, Wt, bias = K.make_case(shape, 0)
    gc, gk = T._cotangents(shape)
    prior = T._dev(np.random.default_rng(3).standard_normal(X.shape).astype(np.float32)) if accumulate else None
    out = T._bwd({"X": X, "Wt": Wt, "bias": bias}, beta, T.DECODE, K.sample_to_image(shape[0]), gc if which != "dk2d" else None,
                 gk if which != "dkcrop" else None, dmap=prior)
    return dict(zip(BACKWARD_OUTPUTS, out))


def run_loss(bjchw, reduction, dtype, accumulate):
    import torch
    import test_gpu_kp_heatmap_loss as T
    d = T._case(*bjchw, dtype={"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[dtype])
    kw = {}
    if accumulate:
        kw["dmap_accumulate_into"] = torch.from_numpy(np.random.default_rng(9).standard_normal(tuple(d["x"].shape)).astype(np.float32)).to(T.DEV)
    got = T._run(d, reduction, LOSS_TOPK, **kw)
    assert (got["dmap"] is None) == (dtype != "fp32")
    return {k: v.cpu().numpy() for k, v in got.items() if v is not None}


def compute(group):
    """{case key: {output: digest}} of one group ("backward" / "loss") on the library capf.lib loads"""
    if group == "backward":
        return {key: {k: digest(v) for k, v in run_backward(*case).items()} for key, *case in backward_cases()}
    return {key: {k: digest(v) for k, v in run_loss(*case).items()} for key, *case in loss_cases()}
