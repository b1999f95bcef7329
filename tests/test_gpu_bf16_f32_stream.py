"""GPU: CAPF_PLAN_BF16_F32_STREAM -- bf16 HRNet with an fp32 activation stream (bf16 only as conv operands; capf_oracle.BF16_STREAM_FP32 is
the spec).  Layer by layer on the engine's own operands (fp32 tensors, bf16 operands, shadows bit for bit), end to end against the stream
emulation and against the reference's own bf16-operand evaluation, the accuracy it buys over the default bf16 plan, determinism, and a
training step held to the fp64 yardstick."""
import numpy as np
import pytest
import torch

import capf_oracle as oracle
import op_oracle
from bf16_report import bf16_stage_report, check_bf16_report
from capf import synth
from test_gpu_fullsize import _model

pytestmark = pytest.mark.gpu


def _flag():
    from capf.lib import PLAN_BF16_F32_STREAM
    return PLAN_BF16_F32_STREAM


def _nchw(x):
    return x.float().permute(0, 3, 1, 2).contiguous()


def _compare_f32(got, want, mass, term):
    """fp32 storage: |got - want| <= 2e-5 * mass, plus op_oracle.compare's allowance for a folded weight on a bf16 rounding boundary
    (outputs beyond it in at most two channels, each within term / 256)."""
    d = (got.float() - want.float()).abs()
    allowed = 2e-5 * mass
    bad = d > allowed
    flips = 0
    if bool(bad.any()):
        chans = torch.nonzero(bad.reshape(-1, bad.shape[-1]).any(dim=0)).flatten().tolist()
        if len(chans) <= 2 and bool((d[bad] <= (allowed + term / 256.0)[bad]).all()):
            flips, bad = len(chans), torch.zeros_like(bad)
    return {"max_err": (d / (allowed + 1e-30)).max().item(), "ok": not bool(bad.any()), "weight_flips": flips}


def stream_layerwise(backbone, B, rows, wseed=81, iseed=82, H=256, W=256, only=None):
    """only: the op names to walk (tests/test_gpu_route_cover.py), as in test_gpu_layerwise.layerwise; None: every conv and fuse sum."""
    model, sd = _model(backbone, "bf16", wseed, _flag())
    img, k2d, kc = synth.synth_inputs(B, H, W, seed=iseed, crop_range=(W, H))
    img_d = img.cuda()
    eng = model.engine_for(img_d)
    names = [n for n, _, _ in eng.schema()]
    n_ops = eng.lib.capf_num_ops(eng.h)
    descs = [eng.op_describe(i) for i in range(n_ops)]
    table = eng.op_table(B)
    todo = [i for i, d in enumerate(descs) if d.backbone and d.kind in (0, 1)]
    if only is not None:
        todo = [i for i in todo if table[i][0] in only]
    stream = torch.cuda.current_stream().cuda_stream
    kernel_of = {}
    kernels, n_checked, n_shadow, flips, worst = set(), 0, 0, 0, {}
    for cp in sorted(set(descs[i].checkpoint for i in todo)):
        eng.forward_prefix(img_d, cp, stream)
        torch.cuda.synchronize()
        for i in [i for i in todo if descs[i].checkpoint == cp]:
            d = descs[i]
            take = lambda slot, h, w, c, dt: eng.op_tensor(i, slot, (B, h, w, c), dt)[rows].cpu()
            got = take(5, d.Ho, d.Wo, d.Cout, d.out_dtype)
            with torch.no_grad():
                if d.kind == 0:
                    x = take(0, d.H, d.W, d.Cin, d.in_dtype)
                    res = take(4, d.Ho, d.Wo, d.Cout, 0) if d.has_residual else None          # (every residual of this plan is fp32)
                    conv, bn = names[d.p_weight][:-len(".weight")], names[d.p_bn_weight][:-len(".weight")]
                    want_b, mass, term = op_oracle.conv_bn_act(sd, conv, bn, x, res, d.ks, d.stride, d.pad, d.act, True)
                    if d.out_dtype == 0:
                        want = oracle._cbr(sd, conv, bn, _nchw(x), d.stride, d.pad, relu=(d.act == 1),
                                           res=_nchw(res) if res is not None else None, nm=oracle.BF16_STREAM_FP32)
                        r = _compare_f32(got, want.permute(0, 2, 3, 1), mass, term)
                    else:
                        r = op_oracle.compare(got, want_b, True, mass, term)
                else:
                    ins = [take(k, d.H >> d.shift[k], d.W >> d.shift[k], d.Cin, d.in_dtype) for k in range(d.n_in)]
                    assert d.in_dtype == 0 and d.out_dtype == 0
                    r = op_oracle.compare(got, op_oracle.fuse_sum(ins, [d.shift[k] for k in range(d.n_in)], d.relu, False), False)
            kern = table[i][1] or "fuse_sum"
            assert r["ok"], (table[i][0], kern, r)
            flips += r["weight_flips"]
            kernels.add(kern)
            kernel_of[table[i][0]] = kern
            worst[kern] = max(worst.get(kern, 0.0), r["max_err"])
            if d.out_dtype == 0:
                try:
                    sh = eng.op_tensor(i, 6, (B, d.Ho, d.Wo, d.Cout), 2)[rows].cpu()
                except Exception:
                    sh = None
                if sh is not None:
                    assert torch.equal(sh.view(torch.int16), oracle.bf16_round(got).to(torch.bfloat16).view(torch.int16)), table[i][0]
                    n_shadow += 1
            n_checked += 1
    print(f"{backbone} bf16 fp32-stream B={B}: {n_checked} backbone ops, {n_shadow} bf16 shadows bit-exact, {flips} weight flips")
    for k, e in sorted(worst.items()):
        print(f"    {k:38s} worst error {e:9.2e} of the allowance")
    # (fp32 storage shows every folded-weight rounding flip that bf16 storage rounds away -- test_gpu_layerwise.py allows 4 there; measured 11
    # for both backbones here, each confined to <= 2 channels of one op and within term / 256 by _compare_f32)
    assert n_checked == len(todo) and flips <= 16
    assert (n_checked > 85 and n_shadow > 20) if only is None else (set(kernel_of) == set(only) and n_checked == len(set(only)))
    stream_layerwise.kernel_of = kernel_of
    stream_layerwise.live_kernel_of = {n: k or kernel_of[n] for n, k, _ in eng.op_table(B) if n in kernel_of}
    return kernels


def test_stream_layerwise_hrnet48_batch256():
    k = stream_layerwise("hrnet_48", 256, [0, 85, 170, 255])
    assert any(x.startswith("igemm_bf16_ws") for x in k) and any(x.startswith("igemm_bf16<") for x in k) and "fuse_sum" in k


def test_stream_layerwise_hrnet32_batch4():
    k = stream_layerwise("hrnet_32", 4, [0, 3])
    assert any(x.startswith("igemm_bf16<") for x in k) and "fuse_sum" in k


def test_stream_end_to_end_vs_the_stream_emulation():
    """cfg2 geometry (HRNet-48, 256x256, B = 256), a 16-frame slice against ca_pf_forward(emulate_bf16="stream_fp32") and the fp32 oracle."""
    B, pick = 256, list(range(0, 256, 16))
    model, sd = _model("hrnet_48", "bf16", 91, _flag())
    img, k2d, kc = synth.synth_inputs(B, 256, 256, seed=92, crop_range=(256, 256))
    taps_e, taps_f = {}, {}
    torch.set_num_threads(min(16, torch.get_num_threads()))
    with torch.no_grad():
        want_e = oracle.ca_pf_forward(sd, img[pick], k2d[pick], kc[pick].clone(), backbone="hrnet_48", taps=taps_e, emulate_bf16="stream_fp32")
        want_f = oracle.ca_pf_forward(sd, img[pick], k2d[pick], kc[pick].clone(), backbone="hrnet_48", taps=taps_f)
        eng = model.engine_for(img.cuda())
        eng.set_debug(True)
        got = model(img.cuda(), k2d.cuda(), kc.clone().cuda()).cpu()
        for l in range(4):
            assert eng.tensor(f"feat{l}").dtype == torch.float32
        rep = bf16_stage_report("cfg2 geometry bf16 fp32-stream", eng, got, pick, taps_e, want_e, taps_f, want_f)
    check_bf16_report(rep)


def test_stream_on_the_golden_frame_sits_at_the_references_bf16_operand_evaluation():
    from bf16_report import reference_bf16_distances
    from conftest import load_golden
    from golden_cases import CASES, case_inputs
    name = "w48_256x256_b1"
    case, g = CASES[name], load_golden(name)
    from conftest import make_model
    model, _ = make_model(case["backbone"], device="cuda", wseed=case["wseed"], bn=case["bn"], compute_dtype="bf16", plan_flags=_flag())
    img, k2d, kc = case_inputs(case)
    with torch.no_grad():
        got = model(img.cuda(), k2d.cuda(), kc.clone().cuda()).cpu().numpy()
    mean = float(np.linalg.norm(got - g["out"], axis=-1).mean())
    opr = reference_bf16_distances(name)["opr"]["joints_mean_dist"]
    print(f"{name}: fp32-stream plan {mean:.3e} m mean from the reference's fp32 joints; reference with bf16 operands only {opr:.3e}")
    assert 0.4 * opr <= mean <= 2.0 * opr


def test_the_stream_plan_is_closer_to_fp32_than_the_default_bf16_plan():
    """The point of the flag: same weights, same 32 frames; distance of the joints to the engine's fp32 plan (parity 1e-6 to the oracle)."""
    B = 32
    img, k2d, kc = synth.synth_inputs(B, 256, 256, seed=95, crop_range=(256, 256))
    out = {}
    for tag, dt, fl in (("fp32", "fp32", 0), ("bf16", "bf16", 0), ("stream", "bf16", _flag())):
        model, _ = _model("hrnet_48", dt, 94, fl)
        with torch.no_grad():
            out[tag] = model(img.cuda(), k2d.cuda(), kc.clone().cuda()).cpu()
        del model
        torch.cuda.empty_cache()
    dist = {t: ((out[t] - out["fp32"]).norm(dim=-1).mean().item(), (out[t] - out["fp32"]).abs().max().item()) for t in ("bf16", "stream")}
    print(f"HRNet-48 256x256, {B} frames, joints vs the fp32 plan: default bf16 {dist['bf16'][0]:.3e} m mean / {dist['bf16'][1]:.3e} max;"
          f"  fp32 stream {dist['stream'][0]:.3e} / {dist['stream'][1]:.3e}")
    assert dist["stream"][0] < dist["bf16"][0] and dist["stream"][1] < dist["bf16"][1]


def test_stream_forward_is_deterministic():
    model, _ = _model("hrnet_48", "bf16", 96, _flag())
    img, k2d, kc = synth.synth_inputs(64, 256, 256, seed=97, crop_range=(256, 256))
    with torch.no_grad():
        a = model(img.cuda(), k2d.cuda(), kc.clone().cuda()).cpu()
        b = model(img.cuda(), k2d.cuda(), kc.clone().cuda()).cpu()
    assert torch.isfinite(a).all() and torch.equal(a, b)


def test_stream_training_step_vs_fp64_yardstick():
    """The hrnet_48-bf16 B = 9 row of test_gpu_train_matrix.py under the flag: frozen backbone, fp32 maps, lifter on the fp32 pipe."""
    from conftest import make_model
    from test_gpu_train_matrix import _hold_to_yardstick, _step
    from train_yardstick import check_cells_against_index_rule
    B = 9
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model, _ = make_model("hrnet_48", device="cuda", wseed=61 + B, bn="random", compute_dtype="bf16", plan_flags=_flag())
    model.train(); model.backbone.eval(); model.volume_net.train()
    model.drop_path_rate = 0.0
    img, k2d, kc, gt = synth.synth_inputs(B, 256, 256, seed=62 + B, crop_range=(256, 256), with_gt=True)
    eng = model.engine_for(img.cuda())
    eng.set_debug(True)
    pred, loss, ref = _step(model, img, k2d, kc, gt)
    for l in range(4):
        assert eng.tensor(f"feat{l}").dtype == torch.float32        # the maps the step read were fp32
    tag = f"hrnet_48 bf16 fp32-stream B={B}"
    check_cells_against_index_rule(eng, B, tag)
    (l2, mx), _ = _hold_to_yardstick(tag, model, eng, B, k2d, ref, gt, pred, loss)
    print(f"  {tag}: worst gradient {l2:.2e} relative L2, {mx:.2e} of max")
