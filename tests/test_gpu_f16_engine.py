"""GPU: compute_dtype = 'fp16' through the engine -- layer-wise on the engine's own operands, end to end against the fp16 evaluation of the
oracle, next to a bf16 engine on the same frames (the point of the feature), and the variant without context blocks.

The yardsticks are the bf16 plan's with the fp16 rounding in the oracle's place (tests/f16_report.py); bounds are bf16_report's, unchanged."""
import contextlib
import copy
import io

import numpy as np
import pytest
import torch

import capf_oracle as oracle
import test_gpu_layerwise as lw
from capf import synth
from f16_report import (BUDGET_CAP, FLOOR_JOINTS, SLACK, bf16_stage_report, check_bf16_report, fp16_emulation, joint_distances,
                        layerwise_in_fp16)
from test_gpu_fullsize import _model

pytestmark = pytest.mark.gpu


def test_layerwise_hrnet32_fp16_batch4():
    """every backbone launch of the fp16 plan at batch 4 (ring schedule, direct kernels, unfused layer1) recomputed from the engine's operands"""
    with layerwise_in_fp16():
        k = lw.layerwise("hrnet_32", "fp16", 4, 256, 256, [0, 3])
    assert any(x.startswith("igemm_f16<") for x in k) and any(x.startswith("igemm_f16_stem") for x in k)
    assert not any("bf16" in x for x in k)


def _smallest_batch_with(backbone, prefixes, limit=512):
    """the smallest batch at which capf_op_info names a kernel of every prefix (a plan-only fp16 handle: the routing rules, queried)"""
    from capf import Engine
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), backbone)
    cfg.model.backbone.fix_weights = True
    eng = Engine(_native.make_capf_config(cfg, 256, 256, compute_dtype="fp16"), device=None)
    for B in range(1, limit + 1):
        kernels = {k for _, k, _ in eng.op_table(B)}
        if all(any(k.startswith(p) for k in kernels) for p in prefixes):
            return B
    raise AssertionError(f"no batch up to {limit} reaches {prefixes}")


def test_layerwise_hrnet32_fp16_at_the_batch_that_reaches_the_halo_tile_and_the_fused_bottlenecks():
    B = _smallest_batch_with("hrnet_32", ("igemm_f16_ws<", "bneck0_f16<", "bneck1_f16<"))
    print(f"smallest batch with the fp16 halo tile and fused bottlenecks: {B}")
    assert B > 4
    with layerwise_in_fp16():
        k = lw.layerwise("hrnet_32", "fp16", B, 256, 256, [0, B - 1])
    assert "bneck0_f16<8x8>" in k and "bneck1_f16<8x8>" in k          # (checked conv by conv from the operands the kernel itself stored)
    assert any(x.startswith("igemm_f16_ws<") for x in k)
    assert not any("bf16" in x for x in k)


def test_chained_pointwise_pairs_fp16_under_no_bneck():
    """CAPF_PLAN_NO_BNECK from batch 32 (layer1's 64x64 maps reach the chain's 131072 rows): the fp16 plan chains layer1's pointwise pairs
    (igemm_bf16_pwchain.hip on fp16 elements) exactly where the bf16 plan does, CAPF_PLAN_NO_PWCHAIN takes the chain out again, and every
    backbone launch of the chained plan meets the layer-wise bound (a prefix that ends on a chain's second conv runs the chain: its result is
    checked from the first conv's stored output; the helper names launches from a table read before the workspace exists, so the names are
    asserted on the live engines above, not on its return value)."""
    from capf.lib import PLAN_NO_BNECK, PLAN_NO_PWCHAIN
    B = 32
    img, k2d, kc = (t.cuda() for t in synth.synth_inputs(B, 256, 256, seed=72, crop_range=(256, 256)))
    names = {}
    for dtype in ("fp16", "bf16"):
        for flags in (PLAN_NO_BNECK, PLAN_NO_BNECK | PLAN_NO_PWCHAIN):
            model, _ = _model("hrnet_32", dtype, 71, flags)
            with torch.no_grad():
                assert bool(torch.isfinite(model(img, k2d, kc.clone())).all())          # (the chain is decided on live pointers: after a forward)
            names[dtype, flags] = [k for _, k, _ in model.engine_for(img).op_table(B)]
    chained, plain = names["fp16", PLAN_NO_BNECK], names["fp16", PLAN_NO_BNECK | PLAN_NO_PWCHAIN]
    assert "igemm_f16_pwchain<64,256,64>" in chained and not any("pwchain" in k for k in plain) and not any(k.startswith("bneck") for k in chained)
    for flags in (PLAN_NO_BNECK, PLAN_NO_BNECK | PLAN_NO_PWCHAIN):                  # route for route the bf16 plan, on live engines
        assert names["fp16", flags] == [k.replace("bf16", "f16") for k in names["bf16", flags]]
    with layerwise_in_fp16():
        k = lw.layerwise("hrnet_32", "fp16", B, 256, 256, [0, B - 1], plan_flags=PLAN_NO_BNECK)
    assert not any("bf16" in x for x in k)


def test_lifter_layerwise_fp16():
    """the lifter half of the tight check on an fp16 engine: every LayerNorm (fp16 writer), attention (fp16 writer) and qkv / proj / fc1 + GELU /
    fc2 launch recomputed from the rows the engine produced (test_gpu_layerwise.lifter_layerwise under the fp16 context)"""
    with layerwise_in_fp16():
        c = lw.lifter_layerwise("hrnet_32", 4, 256, 256, [0, 3])
    assert c.get("qkv bf16") == 8 and c.get("proj bf16") == 8 and c.get("fc1+gelu bf16") == 12 and c.get("fc2 bf16") == 12       # ("bf16": the helper's word for code 2)
    assert c.get("layernorm") == 20 and c.get("attention") == 8


def _corners_bit_exact(eng, B, ref):
    """both sampling sites: the zeros-mode idx{l} (reference points) and the border-mode cidx{i} (deformable samples, from the kernel's own
    positions) == the oracle's integer corner arithmetic"""
    n = 0
    for l in range(4):
        f = eng.tensor(f"feat{l}")
        assert f.dtype == torch.float16
        H, W = f.shape[1], f.shape[2]
        want = oracle.bilinear_corners(ref.numpy(), H, W, "zeros")
        got = eng.tensor(f"idx{l}").cpu().numpy()
        np.testing.assert_array_equal(got[..., 0], want["ix0"])
        np.testing.assert_array_equal(got[..., 1], want["iy0"])
        for i in range(4):
            pos = eng.tensor(f"cpos{i}").cpu().view(B, 17, 4, 16, 2)
            idx = eng.tensor(f"cidx{i}").cpu().view(B, 17, 4, 16, 2).numpy()
            want = oracle.bilinear_corners(pos[:, :, l].numpy(), H, W, "border")
            np.testing.assert_array_equal(idx[:, :, l, :, 0], want["ix0"])
            np.testing.assert_array_equal(idx[:, :, l, :, 1], want["iy0"])
            n += want["ix0"].size
    assert n == 4 * 4 * B * 17 * 16


def test_end_to_end_hrnet32_fp16_against_its_emulation():
    """HRNet-32, 256x256, 4 frames: H = the fp16 engine, E = the oracle under the fp16 emulation, F = the fp32 oracle, stage by stage
    (bf16_report's rules: |H-F| <= 1.5 |E-F| + floor, the triangle, the cap), and both sampling sites' corner indices bit for bit."""
    B = 4
    model, sd = _model("hrnet_32", "fp16", 81)
    img, k2d, kc = synth.synth_inputs(B, 256, 256, seed=82, crop_range=(256, 256))
    taps_e, taps_f = {}, {}
    with torch.no_grad():
        with fp16_emulation():
            want_e = oracle.ca_pf_forward(sd, img, k2d, kc.clone(), backbone="hrnet_32", taps=taps_e, emulate_bf16=True)
        want_f = oracle.ca_pf_forward(sd, img, k2d, kc.clone(), backbone="hrnet_32", taps=taps_f)
        eng = model.engine_for(img.cuda())
        eng.set_debug(True)
        got = model(img.cuda(), k2d.cuda(), kc.clone().cuda()).cpu()
    assert bool(torch.isfinite(got).all())
    check_bf16_report(bf16_stage_report("hrnet_32 fp16 B=4 256x256", eng, got, None, taps_e, want_e, taps_f, want_f))
    _corners_bit_exact(eng, B, taps_f["ref"])


def test_fp16_engine_is_closer_to_fp32_than_the_bf16_engine():
    """The point of the feature.  Same weights, same frames (those of tests/test_f16_plan.py's emulation measurement: hrnet_32, 128x96, 2 frames,
    weights 61, frames 62) through a bf16 engine and an fp16 engine:  |fp16 - F| <= r |bf16 - F| on the joints, max and mean, with
    r = min(1, 1.5 x the EMULATIONS' own ratio on these frames) -- 1.5 is the slack the project gives a HIP path over its emulation
    (bf16_report.SLACK), the ratio is a CPU measurement (0.152 max, 0.146 mean: EXPERIMENTS), never a GPU figure.  The frames qualify
    because the emulations alone separate by more than 2x on them."""
    from test_f16_plan import emulation_distances
    emu, _, _ = emulation_distances()
    assert 2.0 * emu["fp16"][0] <= emu["bf16"][0] and 2.0 * emu["fp16"][1] <= emu["bf16"][1], emu
    r = [min(1.0, SLACK * emu["fp16"][i] / emu["bf16"][i]) for i in (0, 1)]
    img, k2d, kc = synth.synth_inputs(2, 128, 96, seed=62, crop_range=(96, 128))
    dist = {}
    with torch.no_grad():
        for dtype in ("bf16", "fp16"):
            model, sd = _model("hrnet_32", dtype, 61)
            if dtype == "bf16":
                want_f = oracle.ca_pf_forward(sd, img, k2d, kc.clone(), backbone="hrnet_32")
            dist[dtype] = joint_distances(model(img.cuda(), k2d.cuda(), kc.clone().cuda()).cpu(), want_f)
    print(f"joints vs the fp32 oracle (m): bf16 engine max {dist['bf16'][0]:.3e} mean {dist['bf16'][1]:.3e}   fp16 engine max {dist['fp16'][0]:.3e} "
          f"mean {dist['fp16'][1]:.3e}   allowed ratio max {r[0]:.3f} mean {r[1]:.3f}   (emulations: bf16 {emu['bf16'][0]:.3e} / {emu['bf16'][1]:.3e}, "
          f"fp16 {emu['fp16'][0]:.3e} / {emu['fp16'][1]:.3e})")
    assert dist["fp16"][0] <= r[0] * dist["bf16"][0], (dist, r)
    assert dist["fp16"][1] <= r[1] * dist["bf16"][1], (dist, r)


def test_variant_without_context_blocks_fp16_against_its_emulation():
    """VolumetricTriangulationNet(compute_dtype='fp16') at embed 64 over HRNet-32: one forward against the oracle under the fp16 emulation (E)
    and the fp32 oracle (F), the joints held to bf16_report's rules."""
    from model.conpose import VolumetricTriangulationNet, mpi_preset
    from mvn.utils.cfg import config
    cfg = mpi_preset(copy.deepcopy(config), "hrnet_32")
    assert cfg.model.poseformer.embed_dim_ratio == 64
    depth = int(cfg.model.poseformer.depth)
    with contextlib.redirect_stdout(io.StringIO()):
        m = VolumetricTriangulationNet(cfg, compute_dtype="fp16").eval()
    sd = synth.load_synthetic(m, seed=91, bn_mode="random")
    m = m.cuda()
    B = 2
    img, k2d, kc = synth.synth_inputs(B, 256, 256, seed=92, crop_range=(256, 256))

    def run(emulate):
        x = img.permute(0, 3, 1, 2).contiguous()
        ref = oracle.normalise_crop_keypoints_(kc.clone())
        feats = oracle.hrnet_forward(sd, x, nm=oracle.BF16 if emulate else oracle.FP32)
        return oracle.lifter_forward(sd, k2d, ref, feats, context_blocks=False, depth=depth, emulate_bf16=emulate)

    with torch.no_grad():
        with fp16_emulation():
            e = run(True)
        f = run(False)
        out, aux = m(img.cuda(), k2d.cuda(), kc.clone().cuda())
    assert aux is None and tuple(out.shape) == (B, 3, 1, 17, 1)
    h = out.permute(0, 2, 3, 4, 1).contiguous().view(B, 17, 3).cpu()
    he, hf, ef = joint_distances(h, e)[0], joint_distances(h, f)[0], joint_distances(e, f)[0]
    print(f"variant without context blocks, fp16, joints max-abs: |HIP - emu| {he:.3e}  |HIP - fp32| {hf:.3e}  |emu - fp32| {ef:.3e}")
    assert bool(torch.isfinite(h).all())
    assert hf <= SLACK * ef + FLOOR_JOINTS and he <= SLACK * (hf + ef) + FLOOR_JOINTS and hf <= BUDGET_CAP
    assert any(k.startswith("igemm_f16") for _, k, _ in m.engine_for(img.cuda()).op_table(B))
