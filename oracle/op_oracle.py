"""Single-op CPU restatements for the layer-wise ("teacher-forced") parity tests.

TEST INFRASTRUCTURE — NOT PRODUCT CODE (same rules as capf_oracle.py: only tests/ may import it).

Why it exists: a deep bf16 network is chaotic at the rounding level — two correct implementations that differ only in fp32
summation order decorrelate to the full bf16 noise floor within a few dozen layers — so the end-to-end distance between the
HIP path and ANY CPU evaluation (fp32 or bf16-emulating) cannot be bounded tighter than that floor.  One op at a time it can:
each function here recomputes ONE op of the engine's plan (csrc/plan.cpp) from the operands the ENGINE itself produced
(capf_op_tensor), with the same storage roundings (capf_oracle.Numerics), so the outputs agree to fp32 summation order — in
bf16 storage: bit for bit except for the rare value whose fp32 pre-image straddles a rounding boundary (one bf16 ulp).
The ops follow the reference's modules exactly as capf_oracle does:
    conv + eval BatchNorm (+ residual) (+ ReLU)   pose_hrnet.py:66-136, 238-275, 321-327, 383-407; networks/resnet.py:58-93, 137-139;
                                                  globalNet.py:29-45; refineNet.py:3-45
    fuse sum (nearest upsample + add + ReLU)      pose_hrnet.py:294-301
    max-pool 3x3 s2 p1                            networks/resnet.py:140
    bilinear resize, align_corners=True           globalNet.py:40, refineNet.py:61
    nn.Linear (+ residual) (+ GELU), LayerNorm,
    multi-head self-attention of the lifter       pose_dformer.py:15-79 (Mlp :15-31, Attention :34-59, Block :62-79)
"""
import torch
import torch.nn.functional as F

import capf_oracle as oracle


def _nchw(x):
    return x.float().permute(0, 3, 1, 2).contiguous()


def _nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def conv_bn_act(P, conv, bn, x_nhwc, residual_nhwc, ks, stride, pad, act, bf16, up_nhwc=None):
    """x / residual: the engine's own NHWC operands (fp32 or bf16 tensors) -> (NHWC fp32 holding what the engine must store,
    NHWC fp32 `mass` = sum_k |x_k| |w_k| + |bias| + |residual| per output: the scale fp32 summation-order noise is relative to —
    an output that is the small remainder of large cancelling terms cannot be reproduced to a fraction of ITS magnitude)."""
    nm = oracle.BF16 if bf16 else oracle.FP32
    x = nm.r(_nchw(x_nhwc))                                  # (the stem rounds the fp32 image on its way into LDS)
    res = _nchw(residual_nhwc) if residual_nhwc is not None else None
    assert act in (0, 1)
    if up_nhwc is None:
        y = oracle._cbr(P, conv, bn, x, stride, pad, relu=(act == 1), res=res, nm=nm)
    else:
        # + bilinear_upsample(up) BEHIND the activation, in fp32, one storage rounding at the end (capf_op_desc.up_H: CPN's lateral conv with
        # the upsampled path added in its epilogue, globalNet.py:66; csrc/plan.cpp build_cpn)
        y = oracle._cbr(P, conv, bn, x, stride, pad, relu=(act == 1), res=res, nm=(oracle._NOROUND if bf16 else nm))
        y = nm.r(y + F.interpolate(_nchw(up_nhwc), size=y.shape[-2:], mode="bilinear", align_corners=True))
    sc = P[bn + ".weight"] / torch.sqrt(P[bn + ".running_var"] + oracle.BN_EPS)
    w = (P[conv + ".weight"] * sc.view(-1, 1, 1, 1)).abs()
    mass = F.conv2d(x.abs(), w, (P[bn + ".bias"] - P[bn + ".running_mean"] * sc).abs(), stride, pad)
    if res is not None:
        mass = mass + res.abs()
    if up_nhwc is not None:
        mass = mass + F.interpolate(_nchw(up_nhwc).abs(), size=mass.shape[-2:], mode="bilinear", align_corners=True)
    # largest single term |x_k w_k| an output can contain (bound: largest |x| in its window times the channel's largest |w|):
    # the scale of ONE folded weight landing on the other side of a bf16 rounding boundary (see compare)
    xmax = F.max_pool2d(x.abs().amax(dim=1, keepdim=True), ks, stride, pad)
    term = xmax * w.amax(dim=(1, 2, 3)).view(1, -1, 1, 1)
    return _nhwc(y), _nhwc(mass), _nhwc(term)


def fuse_sum(inputs_nhwc, shifts, relu, bf16):
    nm = oracle.BF16 if bf16 else oracle.FP32
    acc = None
    for t, s in zip(inputs_nhwc, shifts):
        t = _nchw(t)
        if s:
            t = F.interpolate(t, scale_factor=2 ** s, mode="nearest")
        acc = t if acc is None else acc + t
    if relu:
        acc = F.relu(acc)
    return _nhwc(nm.r(acc))


def maxpool(x_nhwc):
    return _nhwc(F.max_pool2d(_nchw(x_nhwc), 3, 2, 1))


def resize(x_nhwc, Ho, Wo, bf16, add_nhwc=None):
    """bilinear, align_corners=True (+ a map of the output's shape added in fp32 before the one storage rounding: the engine's
    globalNet runs the 1x1 conv of an `upsamples` branch BEFORE the interpolation and adds the lateral here)"""
    nm = oracle.BF16 if bf16 else oracle.FP32
    y = F.interpolate(_nchw(x_nhwc), size=(Ho, Wo), mode="bilinear", align_corners=True)
    if add_nhwc is not None:
        y = y + _nchw(add_nhwc)
    return _nhwc(nm.r(y))


def linear_rows(a_rows, w, b, res_rows, gelu, bf16_operands, out_bf16):
    """One nn.Linear of the lifter on the engine's own rows: a_rows [M, K] (bf16 rows if the op runs on the bf16 MFMA path), w [N, K],
    b [N], optional fp32 residual rows -> (what the engine must store, mass = sum |a| |w| + |b| + |residual|)."""
    a = a_rows.float()
    w = oracle.bf16_round(w) if bf16_operands else w
    y = a @ w.t() + b
    mass = a.abs() @ w.abs().t() + b.abs()
    if res_rows is not None:
        y = y + res_rows.float()
        mass = mass + res_rows.float().abs()
    if gelu:
        y = F.gelu(y)                                        # exact erf form (pose_dformer.py:17 nn.GELU)
        mass = mass * 1.2                                    # |gelu'| <= 1.13
    return (oracle.bf16_round(y) if out_bf16 else y), mass


def layernorm_rows(x_rows, add_rows, g, b, eps, out_bf16):
    x = x_rows.float() if add_rows is None else x_rows.float() + add_rows.float()
    y = F.layer_norm(x, (x.shape[-1],), g, b, eps)
    return oracle.bf16_round(y) if out_bf16 else y


def attention_rows(qkv_rows, groups, tokens, heads, hd, out_bf16):
    """qkv rows [groups * tokens, 3 * heads * hd] ordered (q | k | v) x heads x hd (pose_dformer.py:49) -> [groups * tokens, heads * hd]"""
    qkv = qkv_rows.float().view(groups, tokens, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    att = torch.softmax((q @ k.transpose(-2, -1)) * hd ** -0.5, dim=-1)
    y = (att @ v).transpose(1, 2).reshape(groups * tokens, heads * hd)
    return oracle.bf16_round(y) if out_bf16 else y


def compare(got, want, bf16, mass=None, term=None):
    """-> dict(max_err, frac_inexact, ok, weight_flips).  `mass` (conv ops): per-output sum of |terms|; fp32 summation in another
    order moves an output by ~1e-6 of it (K <= 3456 terms, eps 6e-8, random-walk growth), bounded here by 2e-5 * mass (Winograd
    F(4,3) amplifies roundoff by its 1/24 .. 8 transform constants: measured 1e-5 of the range per conv).
    fp32 storage: |got - want| <= 2e-5 * mass (no mass: 1e-5 of the tensor's range).
    bf16 storage: got and want must be the SAME or ADJACENT bf16 numbers (one rounding flip), after allowing the fp32 pre-images
    the same 2e-5 * mass; at most 3 % of a tensor may be inexact at all.  One more thing can legitimately differ: the BatchNorm
    fold w * gamma / sqrt(var + eps) is evaluated once by the GPU and once by the CPU, and a folded weight whose fp32 value sits
    on a bf16 rounding boundary may round the other way (probability ~2^-16 per weight).  Such a weight moves every output of ITS
    channel by up to 2^-8 |x_k w_k|: outputs outside the allowance are accepted iff they are within that much (`term`) AND all lie
    in at most two output channels (a kernel bug does not confine itself to one channel's worth of one tap)."""
    got, want = got.float(), want.float()
    d = (got - want).abs()
    slack = 2e-5 * mass if mass is not None else 1e-5 * want.abs().max()
    if not bf16:
        worst = (d / (slack + 1e-30)).max().item()
        return {"max_err": (d.max() / want.abs().max().clamp_min(1e-30)).item(), "frac_inexact": (d > 0).float().mean().item(),
                "ok": worst <= 1.0, "weight_flips": 0}
    mag = torch.maximum(got.abs(), want.abs())
    ulp = torch.pow(2.0, torch.floor(torch.log2(mag.clamp_min(1e-30))) - 7)        # spacing of bf16 numbers at that magnitude
    allowed = ulp + slack
    frac = (d > 0).float().mean().item()
    bad = d > allowed
    flips = 0
    if bool(bad.any()) and term is not None:
        chans = torch.nonzero(bad.reshape(-1, bad.shape[-1]).any(dim=0)).flatten().tolist()
        if len(chans) <= 2 and bool((d[bad] <= (allowed + term / 256.0)[bad]).all()):
            flips = len(chans)
            bad = torch.zeros_like(bad)
    return {"max_err": (d / allowed).max().item(), "frac_inexact": frac, "ok": (not bool(bad.any())) and frac <= 0.03,
            "weight_flips": flips}


# ----------------------------------------------------------------------------------------------
# the inference lifter op by op, in float64 (tests/test_gpu_lifter_ops.py).  Token tensors are in the engine's layout
# [B, J, L1, C] ("b p l c", csrc/plan.cpp build_lifter); P holds float64 tensors (lifter_params64).  Every function returns
# (want, mass): mass = per-output sum of |terms| (op_oracle.compare's allowance is 2e-5 of it), built from the same lines as
# capf_oracle.lifter_forward (pose_dformer.py:115-141, 210-241) out of its own pieces.
#   * A bilinear sample moves with its position: an fp32 unnormalisation ((g + 1) / 2 * (size - 1)) is ~1e-5 pixel off the
#     float64 one at 128 pixels, and the sample by that times the differences of its corners.  Its mass is therefore the
#     sum of |corner| over the four corners of its cell, whatever their weights.
#   * A softmax weight is known to a relative few u * (sum of |terms| of its logit, a dot product of up to 64 terms): masses
#     behind a softmax carry the factor (1 + SOFTMAX_SLACK * logit mass), SOFTMAX_SLACK = 8 * 2^-24 / 2e-5 rounded up.
#   * LayerNorm y = g (x - mean) / std + b: mass = |g| (|x - mean| + LN_MEAN_TERM |mean|) / std + |b|.  The computed mean of
#     a row is at most (24 serial + 6 tree additions) u |mean| off, 1.8e-6 |mean|, inside 2e-5 LN_MEAN_TERM |mean|; a row whose
#     mean is 1e3 x its spread gets an allowance that much wider, which a two-pass kernel needs and a one-pass kernel
#     (E[x^2] - E[x]^2: the variance known to u mean^2) exceeds.
# ----------------------------------------------------------------------------------------------
SOFTMAX_SLACK = 0.03
LN_MEAN_TERM = 0.125


def lifter_params64(P, pre="volume_net"):
    return {k: v.double() for k, v in P.items() if k.startswith(pre + ".")}


def _lin64(P, name, x, x_mass):
    w, b = P[name + ".weight"], P[name + ".bias"]
    return oracle._linear(P, name, x), x_mass @ w.abs().t() + b.abs()


def _ln64(P, name, x, eps):
    return oracle._ln(P, name, x, eps), _ln_mass(x, P[name + ".weight"], P[name + ".bias"], eps)


def _ln_mass(x, g, b, eps):
    mu = x.mean(dim=-1, keepdim=True)
    xc = x - mu
    rstd = 1.0 / torch.sqrt((xc * xc).mean(dim=-1, keepdim=True) + eps)
    return (xc.abs() + LN_MEAN_TERM * mu.abs()) * rstd * g.abs() + b.abs()


def _cells(grid, H, W, border):
    """NW corners of ATen's bilinear index rule (align_corners=True) for float64 positions grid [..., 2]."""
    ix, iy = ((grid[..., 0] + 1) / 2) * (W - 1), ((grid[..., 1] + 1) / 2) * (H - 1)
    if border:
        ix, iy = ix.clamp(0, W - 1), iy.clamp(0, H - 1)
    return torch.floor(ix).long(), torch.floor(iy).long()


def _corner_abs(feat, ix0, iy0):
    """sum over the four corners of the cell (ix0, iy0) of |feat| (zero outside the map): [B, C, *ix0.shape[1:]]"""
    B, C, H, W = feat.shape
    flat = feat.abs().reshape(B, C, H * W)
    out = 0
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        xx, yy = ix0 + dx, iy0 + dy
        inside = ((xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)).to(feat.dtype)
        idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).reshape(B, 1, -1).expand(B, C, -1)
        out = out + torch.gather(flat, 2, idx).reshape(B, C, *ix0.shape[1:]) * inside.unsqueeze(1)
    return out


def embed_rows(P, k2d, ref, feats, pre="volume_net"):
    """OP_EMBED (lifter_fused.hip embed_kernel + embed_feat_kernel; pose_dformer.py:214-225): coord_embed(k2d), grid_sample of every
    level at the reference points (padding zeros), feat_embed.l, + Spatial_pos_embed.  k2d / ref [B, J, 2], feats NCHW float64.
    -> (tokens [B, J, L1, C], mass, parts); parts: sampled / sampled_mass [B, J, C_l] per level (OP_SAMPLE_REF of the unfused route), and
    token0 / token0_mass (OP_PREP_EMBED).  The feat_embed.l GEMMs of the unfused route are checked as rows ops on the engine's sampled rows."""
    pos = P[pre + ".Spatial_pos_embed"][0]                                   # [L1, J, C]
    x0, m0 = _lin64(P, pre + ".coord_embed", k2d, k2d.abs())                # :214
    toks, masses, sampled, smass = [x0], [m0], [], []
    g = ref.unsqueeze(-2)                                                    # [B, J, 1, 2]
    for l, f in enumerate(feats):                                           # :216-218
        s = F.grid_sample(f, g, mode="bilinear", padding_mode="zeros", align_corners=True).squeeze(-1).permute(0, 2, 1)
        ix0, iy0 = _cells(g, f.shape[2], f.shape[3], border=False)
        sm = _corner_abs(f, ix0, iy0).squeeze(-1).permute(0, 2, 1)
        sampled.append(s)
        smass.append(sm)
        t, m = _lin64(P, f"{pre}.feat_embed.{l}", s, sm)                    # :220-221
        toks.append(t)
        masses.append(m)
    x = torch.stack(toks, dim=2) + pos.permute(1, 0, 2)                      # :223-225, "b p l c"
    mass = torch.stack(masses, dim=2) + pos.permute(1, 0, 2).abs()
    parts = dict(sampled=sampled, sampled_mass=smass, token0=x[:, :, 0], token0_mass=mass[:, :, 0])
    return x, mass, parts


def deform_rows(ao, ref, feats, cells=None, pos=None, ao_mass=None, heads=4, samples=4):
    """OP_DEFORM (lifter.hip deform_sample_kernel; pose_dformer.py:122-133 up to the embed_proj): ao [B, J, L, 3 * heads * samples] =
    [attention_weights | sampling_offsets] rows of the L query tokens -> per level l (query token l samples map l):
    U_l [B, J, heads, C_l] = sum over the head's samples of softmax weight x border-padded bilinear sample.
    pos: the sampling positions [B, J, L, heads * samples, 2] to use (the engine's cpos taps); None = tanh(offsets) + ref.
    cells: NW corners [B, J, L, heads * samples, 2] (the engine's cidx taps); None = ATen's rule on pos.
    -> (U list, U mass list, pos64 [B, J, L, hs, 2] = float64 tanh(offsets) + ref, pos64 mass)."""
    B, J, L, _ = ao.shape
    hs = heads * samples
    logits = ao[..., :hs].reshape(B, J, L, heads, samples)
    w = torch.softmax(logits, dim=-1)                                        # :123-124
    pos64 = torch.tanh(ao[..., hs:].reshape(B, J, L, hs, 2)) + ref.view(B, J, 1, 1, 2)   # :125-127
    am = ao.abs() if ao_mass is None else ao_mass
    pos_mass = am[..., hs:].reshape(B, J, L, hs, 2) + ref.abs().view(B, J, 1, 1, 2)
    soft = 1 + SOFTMAX_SLACK * am[..., :hs].reshape(B, J, L, heads, samples).amax(dim=-1, keepdim=True)
    use = pos64 if pos is None else pos
    U, Um = [], []
    for l, f in enumerate(feats):
        H, W = f.shape[2], f.shape[3]
        if cells is None:
            ix0, iy0 = _cells(use[:, :, l], H, W, border=True)
        else:
            ix0, iy0 = cells[:, :, l, :, 0].long(), cells[:, :, l, :, 1].long()
        s = oracle.grid_sample_in_cells(f, use[:, :, l], ix0, iy0)         # [B, C_l, J, hs]   :128
        s = s.permute(0, 2, 3, 1).reshape(B, J, heads, samples, -1)
        sm = _corner_abs(f, ix0, iy0).permute(0, 2, 3, 1).reshape(B, J, heads, samples, -1)
        wl = w[:, :, l].unsqueeze(-1)
        U.append((wl * s).sum(dim=-2))
        Um.append((wl * sm).sum(dim=-2) * soft[:, :, l])
    return U, Um, pos64, pos_mass


def ctx_attn_rows(P, pre, x, ref, feats, cells=None, pos=None, heads=4, samples=4):
    """OP_CTX_ATTN (lifter_fused.hip ctx_attn_kernel + ctx_proj_kernel; pose_dformer.py:115-135), the attention half of context block
    `pre`: q = LayerNorm(x_l + x_0) (eps 1e-5), [attention_weights | sampling_offsets](q), deform_rows, embed_proj.l, residual add into
    tokens 1..L.  x [B, J, L1, C] -> (x after the op, mass, parts: ao / ao_mass = the query rows' projections [B, J, L, 48] (the unfused
    attn_off GEMM), q / q_mass (ctx*.norm1), U / U_mass (the unfused deform), pos / pos_mass = float64 positions)."""
    x0, xr = x[:, :, :1], x[:, :, 1:]
    L = xr.shape[2]
    q, qm = _ln64(P, pre + ".norm1", xr + x0, 1e-5)                          # :120
    aw, awm = _lin64(P, pre + ".attention_weights", q, qm.abs())            # :123
    so, som = _lin64(P, pre + ".sampling_offsets", q, qm.abs())             # :125
    ao, aom = torch.cat([aw, so], -1), torch.cat([awm, som], -1)
    U, Um, pos64, pos_mass = deform_rows(ao, ref, feats, cells, pos, aom, heads, samples)
    outs, masses = [], []
    for l in range(L):                                                        # :130-135
        y, m = _lin64(P, f"{pre}.embed_proj.{l}", U[l], Um[l])              # [B, J, heads, C / heads]
        outs.append(xr[:, :, l] + y.flatten(2))
        masses.append(xr[:, :, l].abs() + m.flatten(2))
    want = torch.cat([x0, torch.stack(outs, 2)], 2)
    mass = torch.cat([x0.abs(), torch.stack(masses, 2)], 2)
    return want, mass, dict(q=q, q_mass=qm, ao=ao, ao_mass=aom, U=U, U_mass=Um, pos=pos64, pos_mass=pos_mass)


def _chain_mass(want, x, logit_mass=0.0):
    """the chains' allowance: 2e-5 of the token buffer's largest magnitude (tests/test_gpu_lifter_chain.py), as a mass; attention whose
    logits carry a mass beyond 1 / SOFTMAX_SLACK (saturated softmax) widens it by SOFTMAX_SLACK x that mass"""
    scale = max(want.abs().max().item(), x.abs().max().item())
    return torch.full_like(want, scale * max(1.0, SOFTMAX_SLACK * logit_mass))


def mlp_half_rows(P, pre, x):
    """OP_MLP_CHAIN (lifter_chain.hip, ATTN = false; pose_dformer.py:137-138): tokens 1..L += fc2(GELU(fc1(LayerNorm(tokens, eps 1e-5)))),
    token 0 unchanged.  x [B, J, L1, C] -> (want, mass = max |x| everywhere: the chains are held to 2e-5 of the buffer's range)."""
    xr = x[:, :, 1:]
    h = oracle._mlp(P, pre + ".mlp", oracle._ln(P, pre + ".norm2", xr, 1e-5))
    want = torch.cat([x[:, :, :1], xr + h], 2)
    return want, _chain_mass(want, x)


def res_chain_rows(P, x, depth, group="res_blocks", pre="volume_net", heads=8):
    """OP_RES_CHAIN (lifter_chain.hip; pose_dformer.py:62-79, 231-238): `depth` Blocks (LayerNorm eps 1e-6) composed.  group res_blocks:
    attention over the L1 level tokens of each joint; joint_blocks: over the J joints, a joint's tokens concatenated (D = L1 * C wide).
    x [B, J, L1, C] -> (want, mass as mlp_half_rows)."""
    B, J, L1, C = x.shape
    y = x.reshape(B * J, L1, C) if group == "res_blocks" else x.reshape(B, J, L1 * C)
    zm = 0.0
    for i in range(depth):
        blk = f"{pre}.{group}.{i}"
        qkv = oracle._linear(P, blk + ".attn.qkv", oracle._ln(P, blk + ".norm1", y, 1e-6)).unflatten(-1, (3, heads, -1)).abs()
        zm = max(zm, (torch.einsum("gnhd,gmhd->ghnm", qkv[..., 0, :, :], qkv[..., 1, :, :]) * qkv.shape[-1] ** -0.5).max().item())
        y = oracle._attn_block(P, blk, y, heads)
    want = y.reshape(B, J, L1, C)
    return want, _chain_mass(want, x, zm)


def head_rows(P, x, pre="volume_net"):
    """OP_HEAD (lifter.hip head_kernel; pose_dformer.py:240): head.1(LayerNorm(x, eps 1e-5)) over a joint's D = L1 * C values.
    x [B, J, L1, C] -> ([B, J, 3], mass)."""
    B, J, L1, C = x.shape
    h, hm = _ln64(P, pre + ".head.0", x.reshape(B, J, L1 * C), 1e-5)
    return _lin64(P, pre + ".head.1", h, hm)


def layernorm_rows64(x_rows, add_rows, g, b, eps):
    """OP_LAYERNORM (and the LayerNorm prologue of a folded GEMM) in float64 -> (y, mass)"""
    x = x_rows if add_rows is None else x_rows + add_rows
    return F.layer_norm(x, (x.shape[-1],), g, b, eps), _ln_mass(x, g, b, eps)


def linear_rows64(a_rows, a_mass, w, b, res_rows, gelu):
    """a rows-mode GEMM in float64 on given A rows (and the mass they carry) -> (y, mass)"""
    y = a_rows @ w.t() + b
    mass = a_mass @ w.abs().t() + b.abs()
    if res_rows is not None:
        y = y + res_rows
        mass = mass + res_rows.abs()
    if gelu:
        y = F.gelu(y)
        mass = mass * 1.2                                    # |gelu'| <= 1.13
    return y, mass


def attention_rows64(qkv_rows, groups, tokens, heads, hd):
    """OP_ATTENTION in float64 -> (y, mass): mass = sum_j a_j |v_j| (1 + SOFTMAX_SLACK x the largest logit mass of the row)"""
    qkv = qkv_rows.view(groups, tokens, 3, heads, hd).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    att = torch.softmax((q @ k.transpose(-2, -1)) * hd ** -0.5, dim=-1)
    zm = (q.abs() @ k.abs().transpose(-2, -1)) * hd ** -0.5
    y = (att @ v).transpose(1, 2).reshape(groups * tokens, heads * hd)
    m = ((att @ v.abs()) * (1 + SOFTMAX_SLACK * zm.amax(dim=-1, keepdim=True))).transpose(1, 2).reshape(groups * tokens, heads * hd)
    return y, m
