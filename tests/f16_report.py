"""Shared by the fp16 tests: the fp16 evaluation of the CPU oracle, and the fp16 form of the layer-wise comparison.

compute_dtype = 'fp16' is the bf16 plan with IEEE fp16 as its 16-bit element, so its yardstick is the bf16 one with another
rounding: every storage and operand rounding of capf_oracle / op_oracle goes through the module attribute
capf_oracle.bf16_round, and fp16_emulation() swaps that attribute for the fp16 rounding while it is open.  Inside it
oracle.ca_pf_forward(..., emulate_bf16=True) IS the fp16-emulating oracle "E" of bf16_report.bf16_stage_report, whose SLACK, floors
and cap apply unchanged (they are statements about a 16-bit evaluation next to its emulation, not about bf16).

The emulation rounds with torch's conversion: round to nearest even, subnormals kept, overflow to Inf.  The kernels saturate at
+-65504 instead (capf.h "fp16 storage"); the two differ only where a value has left fp16's range, which no tensor of these
networks does (activations and folded weights are O(1e-3 .. 1e2)) and which tests/test_gpu_f16_ops.py checks on its own."""
import contextlib

import torch

import capf_oracle as oracle
import op_oracle
from bf16_report import BUDGET_CAP, FLOOR_JOINTS, FLOOR_MAPS, FLOOR_TOKENS, SLACK, bf16_stage_report, check_bf16_report  # noqa: F401  (re-exported)

_COMPARE = op_oracle.compare   # (layerwise_in_fp16 puts compare_f16 in the module attribute's place: fp32 tensors still go to the original)
F16_MIN_ULP = 2.0 ** -24       # spacing of the fp16 subnormals (and of the normals below 2^-13)


def f16_round(x):
    """fp32 -> fp16 (round to nearest even) -> fp32"""
    return x.to(torch.float16).to(torch.float32)


@contextlib.contextmanager
def fp16_emulation():
    """While open, every `bf16` rounding of capf_oracle / op_oracle is an fp16 rounding; restored on exit, whatever happens inside."""
    saved = oracle.bf16_round
    oracle.bf16_round = f16_round
    try:
        yield
    finally:
        oracle.bf16_round = saved


def compare_f16(got, want, f16, mass=None, term=None):
    """op_oracle.compare for fp16 storage (its ulp arithmetic is bf16's: 8 significand bits, no subnormal range in play).
    fp32 storage (f16 false): op_oracle.compare itself.
    fp16 storage: got and want must be the SAME or ADJACENT fp16 numbers -- spacing 2^(e - 10) at magnitude 2^e, never below the
    subnormal spacing 2^-24 -- once their fp32 pre-images are allowed the usual 2e-5 * mass of summation-order noise; at most 3 % of a
    tensor may be inexact at all.  A folded weight on an fp16 rounding boundary (op_oracle.compare's last paragraph) moves its channel's
    outputs by up to 2^-11 |x_k w_k| = term / 2048: accepted under the same confinement rule (at most two channels)."""
    if not f16:
        return _COMPARE(got, want, False, mass, term)
    got, want = got.float(), want.float()
    d = (got - want).abs()
    slack = 2e-5 * mass if mass is not None else 1e-5 * want.abs().max()
    mag = torch.maximum(got.abs(), want.abs())
    ulp = torch.pow(2.0, torch.floor(torch.log2(mag.clamp_min(1e-30))) - 10).clamp_min(F16_MIN_ULP)
    allowed = ulp + slack
    frac = (d > 0).float().mean().item()
    bad = d > allowed
    flips = 0
    if bool(bad.any()) and term is not None:
        chans = torch.nonzero(bad.reshape(-1, bad.shape[-1]).any(dim=0)).flatten().tolist()
        if len(chans) <= 2 and bool((d[bad] <= (allowed + term / 2048.0)[bad]).all()):
            flips = len(chans)
            bad = torch.zeros_like(bad)
    return {"max_err": (d / allowed).max().item(), "frac_inexact": frac, "ok": (not bool(bad.any())) and frac <= 0.03, "weight_flips": flips}


@contextlib.contextmanager
def layerwise_in_fp16():
    """Lets the helpers of tests/test_gpu_layerwise.py (written when 2 was the only 16-bit dtype code) check an fp16 engine: the fp16
    emulation, compare_f16 in op_oracle.compare's place, and capf.lib.Engine translating between the helpers' code 2 ("the 16-bit tensors
    of this handle") and the fp16 handle's truthful code 3 -- op_describe reports 3 as 2, op_tensor reads 2 as 3.  Only for engines whose
    compute_dtype is fp16; everything is restored on exit.  lifter_layerwise builds its model as "bf16" by name: inside this context that
    name builds the fp16 model (its LayerNorm / attention / projection launches are then the fp16 writers and readers)."""
    import test_gpu_layerwise as lw
    from capf import lib as capf_lib
    eng = capf_lib.Engine
    saved = (op_oracle.compare, eng.op_describe, eng.op_tensor, lw._model)

    def model16(backbone, dtype, *args, **kwargs):
        return saved[3](backbone, "fp16" if dtype == "bf16" else dtype, *args, **kwargs)

    def op_describe(self, index):
        d = saved[1](self, index)
        assert self.cfg.compute_dtype == capf_lib.F16 and 2 not in (d.in_dtype, d.out_dtype)      # an fp16 handle stores no bf16
        d.in_dtype = 2 if d.in_dtype == 3 else d.in_dtype
        d.out_dtype = 2 if d.out_dtype == 3 else d.out_dtype
        return d

    def op_tensor(self, index, slot, shape, dtype_code):
        return saved[2](self, index, slot, shape, 3 if dtype_code == 2 else dtype_code)

    with fp16_emulation():
        op_oracle.compare, eng.op_describe, eng.op_tensor, lw._model = compare_f16, op_describe, op_tensor, model16
        try:
            yield
        finally:
            op_oracle.compare, eng.op_describe, eng.op_tensor, lw._model = saved


def joint_distances(got, want):
    """(max-abs, mean per-joint Euclidean distance) between two joint sets [B, 1, 17, 3] / [B, 17, 3], metres"""
    g, w = got.reshape(-1, 17, 3).float(), want.reshape(-1, 17, 3).float()
    return (g - w).abs().max().item(), (g - w).norm(dim=-1).mean().item()
