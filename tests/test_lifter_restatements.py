"""CPU: the float64 single-op restatements of the inference lifter (oracle/op_oracle.py embed_rows, ctx_attn_rows, mlp_half_rows,
res_chain_rows, head_rows), chained through a whole lifter, ARE the oracle's lifter: in float64 they equal capf_oracle.lifter_forward to
roundoff, and evaluated in fp32 they reproduce the reference's own goldens at the tolerances of tests/test_oracle_golden.py.  This pins
the restatements before tests/test_gpu_lifter_ops.py judges any kernel by them."""
import numpy as np
import pytest
import torch

import capf_oracle as oracle
import op_oracle
from conftest import load_golden, make_model
from golden_cases import CASES, case_inputs
from test_oracle_golden import TOL, _mpi_model


def chain(P, k2d, ref, feats, context_blocks=True, depth=4):
    """the lifter as the engine's op sequence: embed, (ctx attention + MLP half) x 4, res blocks, joint blocks, head"""
    x, _, parts = op_oracle.embed_rows(P, k2d, ref, feats)
    taps = {"sampled": parts["sampled"]}
    if context_blocks:
        for i in range(len(feats)):
            pre = f"volume_net.context_blocks.{i}"
            x, _, _ = op_oracle.ctx_attn_rows(P, pre, x, ref, feats)
            x, _ = op_oracle.mlp_half_rows(P, pre, x)
    taps["tok_ctx"] = x
    x, _ = op_oracle.res_chain_rows(P, x, depth)
    taps["tok_res"] = x
    x, _ = op_oracle.res_chain_rows(P, x, depth, "joint_blocks")
    taps["tok_joint"] = x
    out, _ = op_oracle.head_rows(P, x)
    return out.unsqueeze(1), taps


def _case(name):
    case = CASES[name]
    img, k2d, kc = case_inputs(case)
    x = img.permute(0, 3, 1, 2).contiguous()
    if case.get("mpi"):
        _, sd = _mpi_model(case)
    else:
        _, sd = make_model(case["backbone"], wseed=case["wseed"], bn=case["bn"])
    with torch.no_grad():
        feats = oracle.cpn_forward(sd, x) if case["backbone"] == "cpn" else oracle.hrnet_forward(sd, x)
    ref = oracle.normalise_crop_keypoints_(kc)
    return case, sd, k2d, ref, feats


@pytest.mark.parametrize("name", list(CASES))
def test_lifter_restatements_chain_to_the_oracle_and_the_reference_goldens(name):
    case, sd, k2d, ref, feats = _case(name)
    ctx, depth, B = not case.get("mpi"), case.get("depth") or 4, case["B"]
    g = load_golden(name)
    with torch.no_grad():
        P64 = {k: v.double() for k, v in sd.items()}
        f64 = [f.double() for f in feats]
        out64, _ = chain(P64, k2d.double(), ref.double(), f64, ctx, depth)
        want64 = oracle.lifter_forward(P64, k2d.double(), ref.double(), f64, context_blocks=ctx, depth=depth)
        out32, taps = chain(sd, k2d, ref, feats, ctx, depth)
    d64 = (out64 - want64).abs().max().item()
    print(f"{name}: float64 chain vs lifter_forward {d64:.2e} (max |out| {want64.abs().max().item():.2f})")
    assert d64 <= 1e-10 * max(1.0, want64.abs().max().item())
    if case.get("mpi"):
        out = out32.view(B, 1, 17, 3, 1).permute(0, 3, 1, 2, 4)
        np.testing.assert_allclose(out.numpy(), g["out"], atol=TOL, rtol=0)
        return
    np.testing.assert_allclose(out32.numpy(), g["out"], atol=TOL, rtol=0)
    for l in range(4):
        np.testing.assert_allclose(taps["sampled"][l].numpy(), g[f"sampled{l}"], atol=TOL)
    np.testing.assert_allclose(taps["tok_ctx"].permute(0, 2, 1, 3).numpy(), g["tok_ctx"], atol=TOL)
    np.testing.assert_allclose(taps["tok_res"].numpy().reshape(B * 17, 5, -1), g["tok_res"], atol=TOL)
    np.testing.assert_allclose(taps["tok_joint"].numpy().reshape(B, 17, -1), g["tok_joint"], atol=5 * TOL)


def test_deform_restatement_in_given_cells_and_positions_is_the_free_one():
    """ctx_attn_rows with the cells / positions handed in (what the GPU test passes: the engine's cidx / cpos taps) equals the free
    evaluation when they are the float64 ones; the cells agree with ATen's index rule on the float64 positions."""
    case, sd, k2d, ref, feats = _case("w32_256x256_adv")
    with torch.no_grad():
        P = {k: v.double() for k, v in sd.items()}
        f64 = [f.double() for f in feats]
        x, _, _ = op_oracle.embed_rows(P, k2d.double(), ref.double(), f64)
        free, mass, parts = op_oracle.ctx_attn_rows(P, "volume_net.context_blocks.0", x, ref.double(), f64)
        pos = parts["pos"]
        cells = torch.stack([torch.stack(op_oracle._cells(pos[:, :, l], f.shape[2], f.shape[3], True), -1) for l, f in enumerate(f64)], 2)
        given, _, _ = op_oracle.ctx_attn_rows(P, "volume_net.context_blocks.0", x, ref.double(), f64, cells=cells, pos=pos)
    for l, f in enumerate(feats):
        c = oracle.bilinear_corners(pos[:, :, l].float().numpy(), f.shape[2], f.shape[3], "border")
        agree = (torch.from_numpy(c["ix0"]).long() == cells[:, :, l, :, 0]).float().mean().item()
        assert agree > 0.99                      # (fp32 vs float64 positions may straddle a cell boundary only by roundoff)
    assert (free - given).abs().max().item() <= 1e-12 * mass.max().item()
