"""GPU: the fp16 instantiations of the 16-bit kernels, one op at a time, against float64 on the SAME fp16-rounded operands.

Products of two fp16 numbers are exact in fp32 and the accumulation is fp32, so a result differs from the float64 one by an fp32
accumulation's error and, where it is stored as fp16, one rounding:
    |got - want| <= 2.5e-6 * mass  (+ 2^-11 |want| + 2^-25 for an fp16 result)
mass = sum of |terms| (+ |bias| + |residual|) per output -- capf.h's statement for an fp32 accumulation (2.5e-6 of the sum of |terms|,
K <= 3456), half an fp16 ulp (11 significand bits), and half the spacing of the fp16 subnormals.  Nothing here comes from a run."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ACC = 2.5e-6                 # fp32 accumulation, of the sum of |terms| (include/capf.h)
HALF_ULP = 2.0 ** -11        # fp16: 11 significand bits
HALF_SUB = 2.0 ** -25        # half the spacing of the fp16 subnormals
F16_MAX = 65504.0


def _bound(want, mass, f16_out):
    return ACC * mass + ((HALF_ULP * want.abs() + HALF_SUB) if f16_out else 0.0)


def _bn(co, g):
    return (torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g) * 0.1, torch.randn(co, generator=g) * 0.1, torch.rand(co, generator=g) * 0.4 + 0.8)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _fold(wp, co, ci, ks):
    """the fp16 weights the kernel multiplies, from the layout-0 pack [Cout, Kpad] (K order kh, kw, ci) -> float64 OIHW"""
    return wp[:, :ks * ks * ci].double().cpu().view(co, ks, ks, ci).permute(0, 3, 1, 2).contiguous()


def _conv64(x, w_fold, bias, stride, ks, res, act):
    """x NCHW fp16, w_fold float64, bias fp32 [Cout], res NCHW fp16 or None -> (want, mass) float64 NCHW"""
    xd = x.double()
    want = F.conv2d(xd, w_fold, bias.double(), stride, ks // 2)
    mass = F.conv2d(xd.abs(), w_fold.abs(), bias.double().abs(), stride, ks // 2)
    if res is not None:
        want, mass = want + res.double(), mass + res.double().abs()
    return (F.relu(want) if act == 1 else want), mass


def _check(got_nhwc, want, mass, what, f16_out=True):
    got = got_nhwc.double().cpu().permute(0, 3, 1, 2) if got_nhwc.dim() == 4 else got_nhwc.double().cpu()
    assert got.shape == want.shape and bool(torch.isfinite(got).all()), what
    worst = ((got - want).abs() / _bound(want, mass, f16_out)).max().item()
    print(f"{what}: worst error {worst:.3f} of the bound")
    assert worst <= 1.0, (what, worst)


# Cin / Cout 32 and 48 (48: the padding of the 64-deep K chunks and of the 32 / 64-column tiles), 16x16 and 8x8 maps, two frames
@pytest.mark.parametrize("ci,co", [(32, 32), (48, 48), (32, 48), (48, 32)])
@pytest.mark.parametrize("ks,st,H,W", [(3, 1, 16, 16), (3, 2, 16, 16), (1, 1, 8, 8), (3, 1, 8, 8)])
def test_conv_f16_against_fp64_on_fp16_rounded_operands(ci, co, ks, st, H, W):
    from capf import lib as capf
    g = torch.Generator().manual_seed(ci * 7 + co * 3 + ks + st + H)
    x = torch.randn(2, ci, H, W, generator=g).half()
    w = torch.randn(co, ci, ks, ks, generator=g) / (ci * ks * ks) ** 0.5
    wp, bias = capf.pack_conv_16(w.cuda(), tuple(t.cuda() for t in _bn(co, g)))
    assert wp.dtype == torch.float16
    res = torch.randn(2, co, (H - 1) // st + 1, (W - 1) // st + 1, generator=g).half()
    want, mass = _conv64(x, _fold(wp, co, ci, ks), bias.cpu(), st, ks, res, 1)
    got = capf.conv_nhwc_16(_nhwc(x).cuda(), wp, bias, ks, st, 1, _nhwc(res).cuda())
    assert got.dtype == torch.float16
    _check(got, want, mass, f"conv {ks}x{ks}/{st} {ci}->{co} {H}x{W}")
    # the bf16 instantiation of the same entry is the existing bf16 kernel, bit for bit
    xb, rb = _nhwc(x.float().bfloat16()).cuda(), _nhwc(res.float().bfloat16()).cuda()
    bn = tuple(t.cuda() for t in _bn(co, torch.Generator().manual_seed(1)))
    wpb, bb = capf.pack_conv_bf16(w.cuda(), bn)
    wp16, b16 = capf.pack_conv_16(w.cuda(), bn, dtype=capf.BF16)
    assert torch.equal(wpb, wp16) and torch.equal(bb, b16)
    assert torch.equal(capf.conv_nhwc_bf16(xb, wpb, bb, ks, st, 1, rb), capf.conv_nhwc_16(xb, wp16, b16, ks, st, 1, rb, dtype=capf.BF16))


def test_pack_f16_rounds_the_folded_weight_once_to_nearest_even():
    """all three layouts hold fp16(w * gamma / sqrt(var + eps)) -- the same values, permuted -- and the fp32 bias of the bf16 packs"""
    from capf import lib as capf
    g = torch.Generator().manual_seed(3)
    co, ci = 48, 32
    w = torch.randn(co, ci, 3, 3, generator=g) / 17.0
    bn = _bn(co, g)
    packs = [capf.pack_conv_16(w.cuda(), tuple(t.cuda() for t in bn), layout=l) for l in (0, 1, 2)]
    sc = bn[0] / torch.sqrt(bn[3] + 1e-5)
    fold = w * sc.view(-1, 1, 1, 1)
    w0 = packs[0][0][:, :9 * ci].cpu().view(co, 3, 3, ci).permute(0, 3, 1, 2)
    lo, hi = (fold.double() * (1 - 2e-7)).half(), (fold.double() * (1 + 2e-7)).half()          # (the fold itself is an fp32 product: 1 ulp of freedom)
    assert bool(((w0 == lo) | (w0 == hi)).all())
    for wp, _ in packs[1:]:
        assert wp.dtype == torch.float16
        v = wp.flatten().float().cpu()
        assert torch.equal(torch.sort(v[v != 0]).values, torch.sort(w0.flatten().float()[w0.flatten() != 0]).values)
    _, b_bf = capf.pack_conv_bf16(w.cuda(), tuple(t.cuda() for t in bn))
    for _, b in packs:
        assert torch.equal(b, b_bf)


def test_halo_tile_f16_group_of_three_widths_in_one_launch():
    """The 2-D halo tile through its group entry at small geometries: 32-, 64- and 96-channel tiles (the 96 one is the instantiation that
    requests its residual behind the K loop), 8x8 maps with several frames per tile and a partly filled last tile, 16x16 and a ragged
    12x20; residual + ReLU, one problem without either."""
    from capf import lib as capf
    g = torch.Generator().manual_seed(11)
    shapes = [(16, 32, 2, 8, 8, 1, True), (32, 64, 5, 8, 8, 1, True), (48, 96, 3, 16, 16, 1, True), (48, 48, 2, 12, 20, 0, False)]
    probs, refs = [], []
    for ci, co, B, H, W, act, res in shapes:
        x = torch.randn(B, ci, H, W, generator=g).half()
        w = torch.randn(co, ci, 3, 3, generator=g) / (9 * ci) ** 0.5
        bn = tuple(t.cuda() for t in _bn(co, g))
        wp, bias = capf.pack_conv_16(w.cuda(), bn, layout=2)
        w0, _ = capf.pack_conv_16(w.cuda(), bn, layout=0)
        r = torch.randn(B, co, H, W, generator=g).half() if res else None
        probs.append((_nhwc(x).cuda(), wp, bias, act, _nhwc(r).cuda() if res else None, co))
        refs.append(_conv64(x, _fold(w0, co, ci, 3), bias.cpu(), 1, 3, r, act))
    outs = capf.conv_nhwc_16_ws_group(probs)
    for (ci, co, B, H, W, _, _), y, (want, mass) in zip(shapes, outs, refs):
        assert y.dtype == torch.float16
        _check(y, want, mass, f"halo tile {ci}->{co} B{B} {H}x{W}")
    for p, y in zip(probs, outs):                                         # a problem's bits do not depend on what shares its launch
        assert torch.equal(capf.conv_nhwc_16_ws_group([p])[0], y)


def test_grouped_f16_launch_with_row_halo_tiles():
    """The grouped kernel's ping-pong schedule with row-halo tiles (CAPF_PLAN_NO_WS plans, and launches the halo tile does not want): from
    2048 tiles per launch, so 65 frames of 64x64 -- the reference is computed on the first and the last frame only.  A 32-channel 3x3
    (row-halo, chunk width 32), a 48-channel one (chunk width 48) and a 1x1 that stays on the direct tile, in one grid."""
    from capf import lib as capf
    g = torch.Generator().manual_seed(29)
    B, H, W = 65, 64, 64
    probs, refs = [], []
    for ci, co, ks in ((32, 32, 3), (48, 48, 3), (32, 64, 1)):
        x = torch.randn(B, ci, H, W, generator=g).half()
        w = torch.randn(co, ci, ks, ks, generator=g) / (ci * ks * ks) ** 0.5
        bn = tuple(t.cuda() for t in _bn(co, g))
        wp, bias = capf.pack_conv_16(w.cuda(), bn)
        wrh = capf.pack_conv_16(w.cuda(), bn, layout=1)[0] if ks == 3 else None
        r = torch.randn(B, co, H, W, generator=g).half()
        probs.append((_nhwc(x).cuda(), wp, bias, ks, 1, 1, _nhwc(r).cuda(), wrh))
        refs.append(_conv64(x[[0, B - 1]], _fold(wp, co, ci, ks), bias.cpu(), 1, ks, r[[0, B - 1]], 1))
    outs, variant = capf.conv_nhwc_16_group(probs)
    assert variant == 2                                    # igemm_bf16_group_rh_kernel<F16Fmt>
    for (x, wp, *_), y, (want, mass) in zip(probs, outs, refs):
        _check(y[[0, B - 1]], want, mass, f"grouped row-halo launch {x.shape[3]}->{wp.shape[0]}")
        assert bool(torch.isfinite(y.float()).all())


@pytest.mark.parametrize("M,N,K,gelu,res", [(34, 1920, 640, False, False), (34, 640, 640, False, True), (85, 132, 256, False, True), (34, 1280, 640, True, False),
                                            (1088, 1920, 640, False, False)])
def test_linear_f16_against_fp64(M, N, K, gelu, res):
    """the lifter's projections: fp16 operands, fp32 accumulation, fp32 result (+ fp32 residual) or GELU and one fp16 rounding; M = 34 is
    two frames' rows, 85 a ragged row count with N no multiple of the tile, 1088 the 128 x 128 tiles"""
    from capf import lib as capf
    g = torch.Generator().manual_seed(M * 3 + N + K)
    x = torch.randn(M, K, generator=g).half()
    w = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    b = torch.randn(N, generator=g)
    r = torch.randn(M, N, generator=g) if res else None
    want = x.double() @ w.double().t() + b.double()
    mass = x.double().abs() @ w.double().abs().t() + b.double().abs()
    if res:
        want, mass = want + r.double(), mass + r.double().abs()
    if gelu:
        want, mass = F.gelu(want), mass * 1.2                 # |gelu'| <= 1.13
    got = capf.linear_16(x.cuda(), w.cuda(), b.cuda(), r.cuda() if res else None, gelu=gelu)
    assert got.dtype == (torch.float16 if gelu else torch.float32)
    _check(got, want, mass, f"linear M{M} N{N} K{K} gelu={gelu}", f16_out=gelu)


@pytest.mark.parametrize("first", [True, False])
def test_fused_bottleneck_f16_at_its_smallest_tile(first):
    """bneck_bf16.hip on fp16 elements at one 8 x 8 tile per frame (the smallest map its entry accepts), 3 frames: every conv of the
    bottleneck against fp64 on the operands the KERNEL stored (tap), and the product kernel (no taps) bit for bit equal to it."""
    from capf import lib as capf
    g = torch.Generator().manual_seed(5 + first)
    B, H, W, cin = 3, 8, 8, 64 if first else 256
    x = (torch.randn(B, cin, H, W, generator=g).abs() if not first else torch.randn(B, cin, H, W, generator=g)).half()      # (an identity bottleneck's input is a ReLU's output)
    geo = [(cin, 64, 1), (64, 64, 3), (64, 256, 1)] + ([(64, 256, 1)] if first else [])
    packs = []
    for ci, co, ks in geo:
        w = torch.randn(co, ci, ks, ks, generator=g) / (ci * ks * ks) ** 0.5
        packs.append(capf.pack_conv_16(w.cuda(), tuple(t.cuda() for t in _bn(co, g))))
    xd = _nhwc(x).cuda()
    y, t1, t2, sc = capf.bneck_16(xd, packs, tap=True)
    y0 = capf.bneck_16(xd, packs, tap=False)[0]
    assert y.dtype == torch.float16 and torch.equal(y, y0)
    nchw = lambda t: t.cpu().permute(0, 3, 1, 2)
    fold = [_fold(wp, co, ci, ks) for (wp, _), (ci, co, ks) in zip(packs, geo)]
    _check(t1, *_conv64(x, fold[0], packs[0][1].cpu(), 1, 1, None, 1), "bottleneck conv1")
    _check(t2, *_conv64(nchw(t1), fold[1], packs[1][1].cpu(), 1, 3, None, 1), "bottleneck conv2")
    if first:
        _check(sc, *_conv64(x, fold[3], packs[3][1].cpu(), 1, 1, None, 0), "bottleneck downsample")
    _check(y, *_conv64(nchw(t2), fold[2], packs[2][1].cpu(), 1, 1, nchw(sc) if first else x, 1), "bottleneck conv3 + shortcut")


def test_results_beyond_the_fp16_range_saturate():
    """Inputs chosen so that results reach +-7e4: the store clamps them to +-65504 -- no Inf, no NaN -- and leaves the others alone.
    Direct conv, halo tile and the GELU linear (the three fp16 epilogues); a NaN input still gives NaN."""
    from capf import lib as capf
    g = torch.Generator().manual_seed(17)
    ci = co = 32
    x = torch.full((2, ci, 8, 8), 700.0) * (torch.rand(2, ci, 8, 8, generator=g) * 0.2 + 0.9)       # |x| ~ 700: fp16 holds it
    x = x.half()
    w = torch.ones(co, ci, 3, 3) / 2.88 * torch.linspace(-1.0, 1.0, co).view(-1, 1, 1, 1)            # interior outputs: 700 * 288 / 2.88 * s = 7e4 * s
    w0, bias = capf.pack_conv_16(w.cuda())
    w2, _ = capf.pack_conv_16(w.cuda(), layout=2)
    want, mass = _conv64(x, _fold(w0, co, ci, 3), bias.cpu(), 1, 3, None, 0)
    assert want.abs().max().item() > 6.9e4 and (want.abs() < 6e4).any()
    for what, got in (("direct", capf.conv_nhwc_16(_nhwc(x).cuda(), w0, bias, 3, 1, 0)), ("halo tile", capf.conv_nhwc_16_ws_group([(_nhwc(x).cuda(), w2, bias, 0, None, co)])[0])):
        got = got.double().cpu().permute(0, 3, 1, 2)
        assert bool(torch.isfinite(got).all()), what
        sat = want.abs() >= 65520.0 * (1 + 1e-5)                # beyond the last rounding boundary (with the accumulation's slack): clamped
        below = want.abs() <= 65520.0 * (1 - 1e-5)
        assert sat.any() and torch.equal(got[sat], torch.sign(want[sat]) * F16_MAX), what
        assert bool(((got - want).abs()[below] <= _bound(want, mass, True)[below]).all()), what
        assert got.abs().max().item() == F16_MAX
    xl = torch.full((34, 64), 300.0).half()
    wl = (torch.ones(128, 64) * torch.linspace(-4.0, 4.0, 128).view(-1, 1)).half()                  # rows reach +-7.7e4 before GELU
    got = capf.linear_16(xl.cuda(), wl.cuda(), torch.zeros(128).cuda(), None, gelu=True).float().cpu()
    want = F.gelu(xl.double() @ wl.double().t())
    assert bool(torch.isfinite(got).all()) and got.max().item() == F16_MAX and bool((got[want > 65600.0] == F16_MAX).all())
    xn = _nhwc(x).clone()
    xn[0, 3, 3, 5] = float("nan")
    got = capf.conv_nhwc_16(xn.cuda(), w0, bias, 3, 1, 0).float().cpu()
    assert bool(torch.isnan(got[0, 3, 3]).all()) and bool(torch.isfinite(got[1]).all())               # NaN stays NaN, and stays local


# the stem kernels (Cin = 3: fp32 image and fp32 pack in, both rounded to fp16 on their way into LDS): HRNet's 3x3 / 2 into 64 channels (the
# streaming stem), the same into 96 (the tiled stem), CPN's 7x7 / 2 shape, and a 5x5, which no run-based stem takes (the element-wise gather)
@pytest.mark.parametrize("ks,st,co,H,W,big", [(3, 2, 64, 32, 24, False), (3, 2, 64, 32, 24, True), (3, 2, 96, 16, 16, False), (7, 2, 64, 32, 24, True),
                                               (5, 1, 32, 12, 10, True)])
def test_stem_f16_rounds_and_clamps_its_fp32_input(ks, st, co, H, W, big):
    """big: some pixels of the fp32 image are +-7e4, beyond fp16 -- the only place an out-of-range INPUT can enter an fp16 plan.  The staging
    clamps them to +-65504 (no Inf operand, no Inf or NaN out); the reference multiplies the clamped, fp16-rounded image, and -- a few such
    pixels under one 3x3 or 5x5 window can carry a sum past fp16's range -- clamps its results as the store does."""
    from capf import lib as capf
    g = torch.Generator().manual_seed(ks * 11 + co + H)
    x = torch.randn(2, 3, H, W, generator=g) * 2.0
    if big:
        hot = torch.rand(2, 3, H, W, generator=g) < 0.02
        x = torch.where(hot, torch.sign(x) * 7e4, x)
        assert int(hot.sum()) > 10
    w = torch.randn(co, 3, ks, ks, generator=g) / (3 * ks * ks) ** 0.5
    wp, bias = capf.pack_conv(w.cuda(), tuple(t.cuda() for t in _bn(co, g)))
    assert wp.dtype == torch.float32
    x16 = x.clamp(-F16_MAX, F16_MAX).half()
    assert bool(torch.isfinite(x16).all())
    w16 = wp[:, :ks * ks * 3].cpu().half().double().view(co, ks, ks, 3).permute(0, 3, 1, 2).contiguous()
    want, mass = _conv64(x16, w16, bias.cpu(), st, ks, None, 1)
    got = capf.conv_nhwc_16(_nhwc(x).cuda(), wp, bias, ks, st, 1)
    assert got.dtype == torch.float16
    _check(got, want.clamp(-F16_MAX, F16_MAX), mass, f"stem {ks}x{ks}/{st} 3->{co} {H}x{W} big={big}")
    if big:
        assert want.abs().max().item() > 1e3            # (the clamped pixels are in the sums)


def test_subnormal_fp16_operands_are_multiplied_as_values():
    """Activations of 1e-6 are fp16 subnormals (below 6.1e-5).  The matrix pipe multiplies them as the values they are and the results --
    subnormal themselves -- are stored to the subnormal spacing: the usual bound.  A flush to zero anywhere would leave zeros where the
    reference holds ~1e-6, thirty times the bound."""
    from capf import lib as capf
    g = torch.Generator().manual_seed(23)
    ci = co = 48
    x = (torch.randn(2, ci, 8, 8, generator=g) * 1e-6).half()
    assert 0 < x.abs().max().item() < 6.1e-5 and (x != 0).float().mean().item() > 0.9
    w = torch.randn(co, ci, 3, 3, generator=g) / (9 * ci) ** 0.5 * 4.0
    w0, bias = capf.pack_conv_16(w.cuda())
    w2, _ = capf.pack_conv_16(w.cuda(), layout=2)
    want, mass = _conv64(x, _fold(w0, co, ci, 3), bias.cpu(), 1, 3, None, 0)
    assert want.abs().max().item() > 30 * HALF_SUB
    _check(capf.conv_nhwc_16(_nhwc(x).cuda(), w0, bias, 3, 1, 0), want, mass, "direct conv, subnormal operands")
    _check(capf.conv_nhwc_16_ws_group([(_nhwc(x).cuda(), w2, bias, 0, None, co)])[0], want, mass, "halo tile, subnormal operands")
    # subnormal WEIGHTS against normal activations, fp32 out: nothing but the accumulation's error
    xl = torch.randn(34, 64, generator=g).half()
    wl = (torch.randn(128, 64, generator=g) * 1e-6).half()
    got = capf.linear_16(xl.cuda(), wl.cuda(), torch.zeros(128).cuda())
    _check(got, xl.double() @ wl.double().t(), xl.double().abs() @ wl.double().abs().t(), "linear, subnormal weights", f16_out=False)
