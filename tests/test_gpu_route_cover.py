"""GPU: the rows of tests/route_cover_cases.py -- one op per launch route of the production geometries that no whole-plan layer-wise walk
reaches -- recomputed from the engine's own operands with the suite's walkers and bounds (test_gpu_layerwise.layerwise,
test_gpu_bf16_f32_stream.stream_layerwise with only=; op_oracle.compare unchanged: fp32 to 2e-5 of each output's sum of |terms|, 16-bit to the
same or the adjacent number with at most 3 % inexact).  tests/test_route_cover.py holds the table complete on the CPU plan.

A kernel family that passes its stand-alone fuzz can still be wrong at one production shape and tile choice (a ragged last tile at batch 5, a
group launch that mixes tile widths at batch 24, split-K at batch 1 on the 256 x 192 maps); here that shows as one op off, in the row and under
the kernel name that has it."""
import contextlib

import pytest

import route_cover_cases as rc
import test_gpu_layerwise as lw
from f16_report import layerwise_in_fp16
from small_geometry_cases import flag_bits

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("row", rc.ROWS, ids=[rc.row_id(r) for r in rc.ROWS])
def test_route_cover_row(row):
    frames, only = list(row.frames_to_check), {name for name, _ in row.ops}
    if row.plan_flags == "BF16_F32_STREAM":
        from test_gpu_bf16_f32_stream import stream_layerwise as walker
        walker(row.backbone, row.batch, frames, H=row.H, W=row.W, only=only)
    else:
        walker = lw.layerwise
        with (layerwise_in_fp16() if row.dtype == "fp16" else contextlib.nullcontext()):
            walker(row.backbone, row.dtype, row.batch, row.H, row.W, frames, plan_flags=flag_bits(row.plan_flags), only=only)
    # the kernel the walk saw for every named op is the table's (or its split-K form, which only an engine with a device can name:
    # route_cover_cases.LIVE_ONLY): a route that moved cannot turn the row into a repeat of another.  With the workspace's pointers in place
    # capf_op_info may also name a pointwise pair as one chained launch (route_cover_cases' docstring); nothing else
    want = {name: rc.kernel_of(sig) for name, sig in row.ops}
    assert set(walker.kernel_of) == set(want) == set(walker.live_kernel_of)
    moved = {n: (k, want[n]) for n, k in walker.kernel_of.items() if not rc.same_route(want[n], k)}
    moved.update({n: (k, want[n]) for n, k in walker.live_kernel_of.items() if not rc.same_route(want[n], k) and "_pwchain<" not in k})
    assert not moved, moved
