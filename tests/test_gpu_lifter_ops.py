"""GPU: layer-wise ("teacher-forced") parity of EVERY op of the inference lifter, whatever its kind: the fused embedding and context
attention (lifter_fused.hip), the MLP-half and res-block chains (lifter_chain.hip), the unfused route (prep_embed, sample_ref,
deform_sample), LayerNorm, attention, the rows-mode GEMMs (LayerNorm folded or not) and the head.  Each op is recomputed in float64
(oracle/op_oracle.py, pinned to the reference goldens by tests/test_lifter_restatements.py) from the operands the ENGINE produced: the
token buffer is read after capf_forward_prefix(i), the op's result after capf_forward_prefix(i + 1).
  fp32 results: |got - want| <= 2e-5 x the output's sum of |terms|; bf16 results: the same or the adjacent bf16 number; the chains:
  2e-5 x the token buffer's largest magnitude (tests/test_gpu_lifter_chain.py).
  The context sampler's cells (cidx taps) are ATen's index rule on its own positions (cpos taps) bit for bit, the positions agree with
  the float64 ones within the bound, and the samples are recomputed in those cells (a position on a cell boundary by roundoff is no error).
Every point asserts the route its plan takes from op_table's kernel names, and that every lifter op of the schedule was checked."""
import numpy as np
import pytest
import torch

import capf_oracle as oracle
import op_oracle
from capf import synth
from capf.lib import PLAN_NO_F32H2_GEMM, PLAN_NO_FUSED_LIFTER
from lifter_models import lifter_model as _model

pytestmark = pytest.mark.gpu

V = "volume_net"


# ---- the template instance an op reaches (csrc/lifter.hip launch_attention / launch_layernorm / launch_head)
def attention_instance(N, d, out_bf16):
    ob = ",bf16" if out_bf16 else ""
    if 5 < N <= 17 and (3 * 17 * (d + 1) + 17 * 18) * 4 <= 64 * 1024:
        return f"attention_lds_kernel<17{ob}> d={d}"
    if d % 16 == 0 and N <= 17:
        return f"attention_split_kernel<{5 if N <= 5 else 17},4{ob}> d={d}"
    return f"attention_kernel<{5 if N <= 5 else 17}{ob}> d={d}"


def layernorm_instance(C, out_bf16):
    return f"layernorm_kernel<{2 if C <= 128 else 10 if C <= 640 else 24}{',bf16' if out_bf16 else ''}> C={C}"


def head_instance(C):
    return f"head_kernel<{10 if C <= 640 else 24}> D={C}"


def _compare(got, want, bf16, mass=None, inexact_cap=True):
    """op_oracle.compare + `max_err` as the worst fraction of the allowance (fp32 too: compare reports fp32 errors against the range).
    inexact_cap=False: bf16 results need not be 97 % exact, only each the same or the adjacent bf16 number after the fp32 allowance -- rows
    whose mean is 1e3 x their spread have fp32 pre-images known to ~1e-3 of the result, and those round either way often."""
    r = op_oracle.compare(got, want, bf16, mass)
    if bf16 and not inexact_cap:
        r["ok"] = r["max_err"] <= 1.0
    if not bf16:
        d = (got.double() - want.double()).abs()
        r["max_err"] = (d / (2e-5 * mass + 1e-30)).max().item()
    return r


def lifter_ops(model, sd, B, H, W, iseed=82, kcrop=None, inexact_cap=True):
    """Walk every non-backbone op of the inference schedule; returns {kernel instance: (count, worst error)}.  The joint count is the
    checkpoint's (Spatial_pos_embed [1, L1, J, C]), the Blocks' head count the model's configuration's."""
    J = sd[V + ".Spatial_pos_embed"].shape[2]
    heads = int(getattr(model._config.model.poseformer, "num_heads", 8))
    img, k2d, kc = synth.synth_inputs(B, H, W, seed=iseed, crop_range=(192, 256), joints=J)
    if kcrop is not None:
        kc = kcrop
    img_d, k2d_d, kc_d = img.cuda(), k2d.cuda(), kc.cuda()
    ref = oracle.normalise_crop_keypoints_(kc.clone())                        # (bit for bit what the embedding writes back: test_oracle_golden)
    out = torch.zeros(B, 1, J, 3, device="cuda")
    eng = model.engine_for(img_d)
    assert (eng.cfg.num_joints, eng.cfg.num_heads) == (J, heads)
    eng.set_debug(True)                                                       # (cpos / cidx taps of the context samplers)
    names = [n for n, _, _ in eng.schema()]
    n_ops = eng.lib.capf_num_ops(eng.h)
    descs = [eng.op_describe(i) for i in range(n_ops)]
    table = eng.op_table(B)
    stream = torch.cuda.current_stream().cuda_stream
    P = op_oracle.lifter_params64(sd)
    C = P[V + ".coord_embed.weight"].shape[0]
    L1 = P[V + ".Spatial_pos_embed"].shape[1]
    L, D = L1 - 1, L1 * C
    lifter = [i for i, d in enumerate(descs) if not d.backbone]
    copies = [i for i in lifter if table[i][0].startswith("copy.")]
    todo = [i for i in lifter if i not in copies]
    depth = sum(1 for n in names if n.startswith(V + ".res_blocks.") and n.endswith(".norm1.weight"))

    def prefix(n):
        eng.forward_prefix(img_d, n, stream, k2d_d, kc_d.clone(), out)       # (a fresh kcrop every time: the embedding normalises it in place)
        torch.cuda.synchronize()

    def tokens(i, slot):
        return eng.op_tensor(i, slot, (B, J, L1, C), 0).double().cpu()

    def feats():
        return [eng.tensor(f"feat{l}").double().permute(0, 3, 1, 2).contiguous().cpu() for l in range(L)]

    def rows_of(i, slot, k, width, dt):
        d = descs[i]
        G, S1, S2, off = (int(v) for v in d.maps[k])
        m = torch.arange(B * d.rows_per_frame)
        addr = (m // G) * S1 + (m % G) * S2 + off
        flat = eng.op_tensor(i, slot, (int(addr.max()) + width,), dt)
        return flat[(addr[:, None] + torch.arange(width)[None, :]).cuda()].double().cpu()

    def cells_and_positions(n, maps, pos64, pos_mass):
        """the context sampler's taps: cells == ATen's rule on its own positions bit for bit, positions == float64 ones within the bound"""
        cpos = eng.tensor(f"cpos{n}").cpu().view(B, J, L, 16, 2)
        cidx = eng.tensor(f"cidx{n}").cpu().view(B, J, L, 16, 2)
        for l, f in enumerate(maps):
            c = oracle.bilinear_corners(cpos[:, :, l].numpy(), f.shape[2], f.shape[3], "border")
            np.testing.assert_array_equal(cidx[:, :, l, :, 0].numpy(), c["ix0"])
            np.testing.assert_array_equal(cidx[:, :, l, :, 1].numpy(), c["iy0"])
        r = _compare(cpos, pos64, False, pos_mass)
        assert r["ok"], (f"cpos{n}", r)
        return cpos.double(), cidx.long(), r["max_err"]

    def check_idx(l, f):
        idx = eng.tensor(f"idx{l}").cpu().numpy()
        c = oracle.bilinear_corners(ref.numpy(), f.shape[2], f.shape[3], "zeros")
        np.testing.assert_array_equal(idx[..., 0], c["ix0"])
        np.testing.assert_array_equal(idx[..., 1], c["iy0"])

    results = []                    # (instance, op name, compare result)
    ref64, k2d64 = ref.double(), k2d.double()
    for i in todo:
        d, (name, kern, _) = descs[i], table[i]
        n0 = len(results)
        prefix(i)
        with torch.no_grad():
            if kern == "embed":
                prefix(i + 1)
                maps = feats()
                want, mass, parts = op_oracle.embed_rows(P, k2d64, ref64, maps)
                results.append((kern, name, _compare(tokens(i, 5), want, False, mass)))
                for l, f in enumerate(maps):
                    results.append((kern + " sampled", name, _compare(eng.tensor(f"sampled{l}").cpu(), parts["sampled"][l], False,
                                                                               parts["sampled_mass"][l])))
                    check_idx(l, f)
            elif kern == "prep_embed":
                prefix(i + 1)
                want, mass, parts = op_oracle.embed_rows(P, k2d64, ref64, feats())
                results.append((kern, name, _compare(tokens(i, 5)[:, :, 0], parts["token0"], False, parts["token0_mass"])))
            elif kern == "sample_ref":
                l = int(name.split(".")[1])
                prefix(i + 1)
                maps = feats()
                want, mass, parts = op_oracle.embed_rows(P, k2d64, ref64, maps)
                got = eng.op_tensor(i, 5, (B, J, maps[l].shape[1]), 0).cpu()
                results.append((kern, name, _compare(got, parts["sampled"][l], False, parts["sampled_mass"][l])))
                check_idx(l, maps[l])
            elif kern == "ctx_attn":
                n = int(name[3:].split(".")[0])
                x = tokens(i, 5)
                prefix(i + 1)
                maps = feats()
                _, _, parts = op_oracle.ctx_attn_rows(P, f"{V}.context_blocks.{n}", x, ref64, maps)
                cpos, cidx, perr = cells_and_positions(n, maps, parts["pos"], parts["pos_mass"])
                want, mass, _ = op_oracle.ctx_attn_rows(P, f"{V}.context_blocks.{n}", x, ref64, maps, cells=cidx, pos=cpos)
                results.append((kern, name, _compare(tokens(i, 5), want, False, mass)))
                results.append(("ctx_attn positions (cpos)", name, {"max_err": perr, "ok": True}))
            elif kern == "deform_sample":
                n = int(name[3:].split(".")[0])
                ao = rows_of(i - 1, 5, 1, 3 * 16, 0).view(B, J, L, 48)            # (the attn_off GEMM in front of it: its output rows)
                prefix(i + 1)
                maps = feats()
                U, Um, pos64, pos_mass = op_oracle.deform_rows(ao, ref64, maps)
                cpos, cidx, perr = cells_and_positions(n, maps, pos64, pos_mass)
                U, Um, _, _ = op_oracle.deform_rows(ao, ref64, maps, cells=cidx, pos=cpos)
                for l in range(L):
                    assert table[i + 1 + l][0] == f"ctx{n}.embed_proj.{l}"
                    got = eng.op_tensor(i + 1 + l, 0, (B, J, 4, maps[l].shape[1]), 0).cpu()
                    results.append((kern, name, _compare(got, U[l], False, Um[l])))
                results.append(("deform_sample positions (cpos)", name, {"max_err": perr, "ok": True}))
            elif kern == "mlp_chain":
                x = tokens(i, 5)
                prefix(i + 1)
                want, mass = op_oracle.mlp_half_rows(P, f"{V}.context_blocks.{int(name[3:].split('.')[0])}", x)
                results.append((kern, name, _compare(tokens(i, 5), want, False, mass)))
            elif kern == "res_chain":
                x = tokens(i, 5)
                prefix(i + 1)
                want, mass = op_oracle.res_chain_rows(P, x, depth, heads=heads)
                results.append((kern, name, _compare(tokens(i, 5), want, False, mass)))
            elif kern == "head":
                x = tokens(i, 0)
                prefix(i + 1)
                want, mass = op_oracle.head_rows(P, x)
                results.append((head_instance(D), name, _compare(out.cpu().view(B, J, 3), want, False, mass)))
            elif d.kind in (0, 4, 5):
                assert d.kind != 0 or not d.conv
                a = rows_of(i, 0, 0, d.Cin, d.in_dtype)
                res = None
                if d.has_residual and name.startswith("feat_embed."):        # (the pos-embed parameter as residual, capf_op_desc has no slot for it)
                    l = int(name.split(".")[1])
                    res = P[V + ".Spatial_pos_embed"][0, 1 + l].repeat(B, 1)
                elif d.has_residual:
                    res = rows_of(i, 4, 2, d.Cout if d.kind == 0 else d.Cin, 0)
                prefix(i + 1)
                got = rows_of(i, 5, 1, d.Cout, d.out_dtype)
                out_bf = d.out_dtype == 2
                if d.kind == 0:
                    if d.p_weight >= 0:
                        w, b = sd[names[d.p_weight]].double(), sd[names[d.p_bias]].double()
                    else:                                                         # [attention_weights | sampling_offsets] as one pack
                        assert name.endswith(".attn_off")
                        pre = f"{V}.context_blocks.{int(name[3:].split('.')[0])}"
                        w = torch.cat([P[pre + ".attention_weights.weight"], P[pre + ".sampling_offsets.weight"]])
                        b = torch.cat([P[pre + ".attention_weights.bias"], P[pre + ".sampling_offsets.bias"]])
                    if d.in_dtype == 2:
                        w = oracle.bf16_round(w.float()).double()
                    am = a.abs()
                    inst = kern
                    if d.p_ln_weight >= 0:                                        # LayerNorm folded into the GEMM's prologue
                        a, am = op_oracle.layernorm_rows64(a, None, sd[names[d.p_ln_weight]].double(), sd[names[d.p_ln_bias]].double(), float(d.eps))
                        inst = f"{kern} + LayerNorm prologue (eps {d.eps:.0e}) K={d.Cin}"
                    want, mass = op_oracle.linear_rows64(a, am, w, b, res, d.act == 2)
                elif d.kind == 4:
                    want, mass = op_oracle.layernorm_rows64(a, res, sd[names[d.p_ln_weight]].double(), sd[names[d.p_ln_bias]].double(), float(d.eps))
                    inst = layernorm_instance(d.Cin, out_bf) + f" eps {d.eps:.0e}"
                else:
                    g, t, h, hd = (int(v) for v in d.attn)
                    assert h == heads and t in (L1, J)
                    want, mass = op_oracle.attention_rows64(a, g * B, t, h, hd)
                    inst = attention_instance(t, hd, out_bf)
                if out_bf:
                    want = oracle.bf16_round(want.float())
                results.append((inst, name, _compare(got, want, out_bf, mass, inexact_cap)))
            else:
                raise AssertionError(f"lifter op {name} ({kern}, kind {d.kind}) has no restatement")
        assert len(results) > n0 and all(r[2]["ok"] for r in results[n0:]), (name, [r for r in results[n0:] if not r[2]["ok"]])
    checked = {r[1] for r in results}
    assert checked == {table[i][0] for i in todo} and len(todo) == len(lifter) - len(copies)
    assert [table[i][0] for i in copies] == ["copy.tok_ctx", "copy.tok_res", "copy.tok_joint"]
    worst = {}
    for inst, name, r in results:
        c, e, nm = worst.get(inst, (0, -1.0, ""))
        worst[inst] = (c + 1, max(e, r["max_err"]), name if r["max_err"] > e else nm)
    print(f"B={B}: {len(todo)} lifter ops recomputed in float64 from the engine's own operands")
    for k in sorted(worst):
        c, e, nm = worst[k]
        print(f"    {k:64s} x {c:3d}   worst error {e:9.2e} of the allowance   ({nm})")
    lifter_ops.kernels = {table[i][1] for i in todo}
    return worst


def _has(worst, prefix):
    return any(k.startswith(prefix) for k in worst)


@pytest.mark.parametrize("B", [1, 7, 64])
def test_lifter_ops_default_fp32_plan(B):
    """embed, ctx_attn, the MLP halves and the res blocks as chains (batch 1 / 7 / 64: ragged last row tiles), the joint blocks on the
    two-piece GEMMs (batch 1: the fp32 split-K kernel) with LayerNorm at C = 640, attention at d = 80, head_kernel<10> at D = 640"""
    model, sd = _model("hrnet_32")
    w = lifter_ops(model, sd, B, 256, 192)
    k = lifter_ops.kernels
    assert {"embed", "ctx_attn", "mlp_chain", "res_chain", "head"} <= k and not k & {"prep_embed", "sample_ref", "deform_sample"}
    assert _has(w, "igemm_f32_rows_splitk" if B == 1 else "igemm_f32h2g") and _has(w, "layernorm_kernel<10> C=640") and _has(w, "attention_lds_kernel<17> d=80") and "head_kernel<10> D=640" in w


def test_lifter_ops_unfused_route():
    """CAPF_PLAN_NO_FUSED_LIFTER: prep_embed, sample_ref, the feat_embed / attn_off / embed_proj GEMMs, deform_sample, per-op LayerNorm and
    attention (attention_split_kernel over the 5 level tokens at d = 16)"""
    model, sd = _model("hrnet_32", plan_flags=PLAN_NO_FUSED_LIFTER)
    w = lifter_ops(model, sd, 7, 256, 192)
    assert {"prep_embed", "sample_ref", "deform_sample"} <= lifter_ops.kernels and not lifter_ops.kernels & {"embed", "ctx_attn", "mlp_chain", "res_chain"}
    assert _has(w, "attention_split_kernel<5,4> d=16") and _has(w, "layernorm_kernel<2> C=128")


def test_lifter_ops_fp32_matrix_pipe_with_layernorm_folded():
    """CAPF_PLAN_NO_F32H2_GEMM: the lifter GEMMs on the fp32 matrix pipe, LayerNorm folded into their prologue at K = 128 (igemm_f32 LNA)"""
    model, sd = _model("hrnet_32", plan_flags=PLAN_NO_F32H2_GEMM)
    w = lifter_ops(model, sd, 3, 256, 192)
    assert not any(k.startswith("igemm_f32h2g") for k in lifter_ops.kernels) and "res_chain" not in lifter_ops.kernels
    assert _has(w, "igemm_f32<") and any(k.startswith("igemm_f32<") and "LayerNorm prologue (eps 1e-05) K=128" in k for k in w)
    assert any(k.startswith("igemm_f32<") and "LayerNorm prologue (eps 1e-06) K=128" in k for k in w)


@pytest.mark.parametrize("B", [1, 5])
def test_lifter_ops_embed_256(B):
    """embed_dim_ratio 256 (D = 1280): ctx_attn at its largest C, LayerNorm folded at K = 256, layernorm_kernel<24>, attention_lds_kernel at
    d = 160, head_kernel<24>"""
    model, sd = _model("hrnet_32", embed=256)
    w = lifter_ops(model, sd, B, 256, 192)
    assert {"embed", "ctx_attn"} <= lifter_ops.kernels
    assert any("LayerNorm prologue" in k and k.endswith("K=256") for k in w)
    assert _has(w, "layernorm_kernel<24> C=1280") and _has(w, "attention_lds_kernel<17> d=160") and "head_kernel<24> D=1280" in w


def test_lifter_ops_embed_288_wide_fallback():
    """embed_dim_ratio 288: the unfused kernels, the generic attention_kernel<5> at d = 36, ragged head lanes at D = 1440"""
    model, sd = _model("hrnet_32", embed=288)
    w = lifter_ops(model, sd, 2, 256, 192)
    assert {"prep_embed", "sample_ref", "deform_sample"} <= lifter_ops.kernels
    assert _has(w, "attention_kernel<5> d=36") and _has(w, "layernorm_kernel<24> C=1440") and "head_kernel<24> D=1440" in w


@pytest.mark.parametrize("backbone,embed", [("hrnet_32", 64), ("hrnet_48", 96)])
def test_lifter_ops_mpi_variant(backbone, embed):
    """the MPI-INF-3DHP variant (no context blocks), depth 2: LayerNorm folded at K = 64 / 96, attention_kernel<5> at d = 8 / 12, ragged
    D = 320 / 480"""
    model, sd = _model(backbone, mpi=True, depth=2)
    w = lifter_ops(model, sd, 3, 256, 192)
    D = 5 * embed
    assert not lifter_ops.kernels & {"ctx_attn", "deform_sample", "mlp_chain"} and "embed" in lifter_ops.kernels
    assert any("LayerNorm prologue" in k and k.endswith(f"K={embed}") for k in w)
    assert _has(w, f"attention_kernel<5> d={embed // 8}") and _has(w, f"layernorm_kernel<10> C={D}") and f"head_kernel<10> D={D}" in w


@pytest.mark.parametrize("backbone,B,H,W", [("hrnet_48", 2, 256, 256), ("cpn", 3, 384, 288)])
def test_lifter_ops_bf16_plan(backbone, B, H, W):
    """compute_dtype = bf16: embed / ctx_attn on bf16 maps, bf16 LayerNorm / attention writers and bf16 GEMMs, the head"""
    model, sd = _model(backbone, dtype="bf16")
    w = lifter_ops(model, sd, B, H, W)
    assert {"embed", "ctx_attn", "head"} <= lifter_ops.kernels
    assert _has(w, "layernorm_kernel<2,bf16>") and _has(w, "attention_lds_kernel<17,bf16>") and _has(w, "attention_split_kernel<5,4,bf16>")


# ---- edges, as data: one seeded adversarial case per kind, on the default fp32 plan and on the bf16 plan
def _ln_cancellation(sd):
    """every token row = 2 + a spread of ~1.2e-3 (mean ~1.7e3 x the standard deviation, variance below the LayerNorms' eps): the residual
    stream's writers scaled by 2e-3, Spatial_pos_embed a constant"""
    for k in list(sd):
        if k.startswith(V + ".") and any(t in k for t in (".coord_embed.", ".feat_embed.", ".embed_proj.", ".attn.proj.", ".mlp.fc2.")):
            sd[k] = sd[k] * 2e-3
    sd[V + ".Spatial_pos_embed"] = torch.full_like(sd[V + ".Spatial_pos_embed"], 2.0)


def _saturated_softmax(sd):
    """qkv x 11 and attention_weights x 60: logits of ~100 and more, beyond exp's fp32 range without the max subtraction"""
    for k in list(sd):
        if k.startswith(V + ".") and (".attn.qkv." in k):
            sd[k] = sd[k] * 11.0
        if k.startswith(V + ".") and (".attention_weights." in k):
            sd[k] = sd[k] * 60.0


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("case", ["borders", "layernorm_cancellation", "saturated_softmax"])
def test_lifter_ops_adversarial(case, dtype):
    B = 2
    tweak = {"layernorm_cancellation": _ln_cancellation, "saturated_softmax": _saturated_softmax}.get(case)
    model, sd = _model("hrnet_32", dtype=dtype, tweak=tweak)
    kc = synth.adversarial_crop_keypoints(B, seed=83) if case == "borders" else None      # (on / next to cell edges, on and beyond +-1)
    lifter_ops(model, sd, B, 256, 192, kcrop=kc, inexact_cap=case != "layernorm_cancellation")
    assert {"embed", "ctx_attn", "head"} <= lifter_ops.kernels
