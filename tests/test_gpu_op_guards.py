"""GPU: where the stand-alone kernels write and what they read past their operands (tests/workspace_guard.py).

capf/lib.py's wrappers allocate every output with torch.empty, which rounds allocations up: a ragged last tile that stores a few elements
past y is invisible to test_gpu_ops.py / test_gpu_f16_ops.py, and so is a fetch past an operand's end whose neighbour happens to be finite.
Here every wrapper runs inside guarded_allocations() -- its outputs are interiors of banded allocations pre-filled with 0xFF (NaN) -- with
every input a flush copy (the first byte behind its last element is band), TWICE: band byte 0x00 and band byte 0xFF behind the inputs.  The
two results must have the same bits and no band may change.  No oracle: values are those files' business, and their seeded problem
generators are imported, not copied.  Problems with more than 2 M output elements are left out.

Packed weights and the bias are guarded outputs too, and come back fully written: no 0xFF element inside the documented extent (Kpad
columns, rows up to a channel slice, inverse scales).  A pack then goes to its kernel as a flush copy like every other input.

Shapes added to the generators': linear M in {1, 31, 85, 257}, N in {4, 36, 100} (and an odd N for the fp32 linear), conv maps 1 x 1, 1 x 2,
5 x 3 and 9 x 7, stride 2 on odd maps, Cout in {8, 18, 36}, B * Ho * Wo no multiple of 256.  K in {36, 100, 132} (K % 32 != 0): the
linear entry points refuse such a K (asserted here), so it runs where the library accepts it -- as the Cin of 1 x 1 convs on the same GEMM
kernels, and as N / K of the weight gradient."""
import pytest
import torch

import test_gpu_ops as ops
import workspace_guard as wg
from capf import lib as capf

pytestmark = pytest.mark.gpu

MAX_OUT = 2 << 20
BANDS = (0x00, 0xFF)


def _nhwc(t):
    return None if t is None else t.permute(0, 2, 3, 1).contiguous()


def _written(t, what):
    """a guarded output (pre-filled with 0xFF) holds no element that is still all ones"""
    if t is None:
        return
    bits = t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)
    left = int((bits == -1).sum())
    assert left == 0, f"{what}: {left} of {bits.numel()} elements were never written (first at {int((bits.flatten() == -1).nonzero()[0, 0])})"


def _twice(tag, body):
    """body(put) -> outputs (tensors; None entries allowed).  put(t) hands a host / device tensor over as a flush device copy whose band is
    the run's band byte.  Runs under both band bytes inside guarded_allocations; every band checked; the outputs bit-identical."""
    runs = []
    for band in BANDS:
        flushed = []

        def put(t):
            if t is None:
                return None
            flushed.append(wg.flush(t if t.is_cuda else t.cuda(), band))
            return flushed[-1]

        with wg.guarded_allocations():
            outs = [o for o in body(put) if o is not None]
            torch.cuda.synchronize()
        wg.check_all(flushed, f"{tag}: input (band 0x{band:02X})")
        for i, o in enumerate(outs):
            _written(o, f"{tag}: output {i} (band 0x{band:02X})")
        runs.append([o.clone() for o in outs])
    assert len(runs[0]) == len(runs[1]) > 0
    for i, (a, b) in enumerate(zip(*runs)):
        same = a.view(torch.uint8) == b.view(torch.uint8)
        assert bool(same.all()), (f"{tag}: output {i} depends on the bytes behind an input: {int((~same).sum())} bytes differ between band 0x00 and "
                                  f"band 0xFF, first at byte {int((~same).flatten().nonzero()[0, 0])} of {same.numel()}")


def _packed(put, pack, w, bn, what, **kw):
    """pack inside the guarded context: weights and bias fully written; -> flush copies of (wp, bias[, extra])"""
    out = pack(put(w), tuple(put(t) for t in bn) if bn is not None else None, **kw)
    torch.cuda.synchronize()
    for t in out[:2]:
        if torch.is_tensor(t):
            _written(t, f"{what} pack")
    return tuple(put(t) if torch.is_tensor(t) else t for t in out)


def _bn(co, g):
    return (torch.rand(co, generator=g) + 0.5, torch.randn(co, generator=g) * 0.1, torch.randn(co, generator=g) * 0.1, torch.rand(co, generator=g) * 0.4 + 0.8)


def _out_elems(B, H, W, co, ks=3, st=1):
    Ho, Wo = capf._out_hw(H, W, ks, st)
    return B * Ho * Wo * co


# the shapes the generators do not produce: (ci, co, ks, stride, H, W, B): maps 1 x 1, 1 x 2, 5 x 3, 9 x 7; stride 2 on odd maps; Cout 8, 18, 36;
# B * Ho * Wo % 256 != 0 throughout (257 rows: 1 x 1 at B = 257); Cin 36, 100, 132: K % 32 != 0 on the GEMM kernels
EXTRA_CONVS = [(32, 8, 3, 1, 1, 1, 3), (64, 36, 3, 1, 1, 2, 5), (36, 18, 1, 1, 5, 3, 7), (100, 36, 1, 1, 9, 7, 3), (132, 8, 1, 1, 1, 1, 257),
               (32, 36, 3, 2, 5, 3, 4), (64, 18, 3, 2, 9, 7, 5), (36, 36, 3, 2, 9, 7, 2), (100, 8, 3, 1, 5, 3, 31), (16, 18, 5, 2, 9, 7, 3),
               (132, 36, 3, 1, 9, 7, 5), (48, 8, 1, 2, 5, 3, 85)]
assert all((B * capf._out_hw(H, W, ks, st)[0] * capf._out_hw(H, W, ks, st)[1]) % 256 for _, _, ks, st, H, W, B in EXTRA_CONVS)


def _extra_conv_problems(seed, ok=lambda ci, co, ks, st: True):
    g = torch.Generator().manual_seed(seed)
    for case, (ci, co, ks, st, H, W, B) in enumerate(EXTRA_CONVS):
        if not ok(ci, co, ks, st):
            continue
        x = torch.randn(B, ci, H, W, generator=g)
        w = torch.randn(co, ci, ks, ks, generator=g) / (ci * ks * ks) ** 0.5
        Ho, Wo = capf._out_hw(H, W, ks, st)
        yield 100 + case, ci, co, ks, st, H, W, B, case % 2, bool(case % 3), x, w, _bn(co, g), torch.randn(B, co, Ho, Wo, generator=g)


# ---- fp32 MFMA convs and linears ----------------------------------------------------------------------------------------------------------------
def test_conv_f32_fuzz_guarded():
    """capf_op_pack_conv / capf_op_conv on test_conv_fuzz_against_torch's 36 problems and the extra shapes; the Cout % 4 == 0 ones again as
    grouped launches of up to 8"""
    g = torch.Generator().manual_seed(1)
    probs = []
    for case, ci, co, ks, st, H, W, B, act, res, x, w, bn in ops.conv_fuzz_problems():
        Ho, Wo = capf._out_hw(H, W, ks, st)
        probs.append((case, co, ks, st, act, x, w, bn, torch.randn(B, co, Ho, Wo, generator=g) if res else None))
    for case, ci, co, ks, st, H, W, B, act, res, x, w, bn, r in _extra_conv_problems(2):
        probs.append((case, co, ks, st, act, x, w, bn, r if res else None))
    probs = [p for p in probs if _out_elems(p[5].shape[0], p[5].shape[2], p[5].shape[3], p[1], p[2], p[3]) <= MAX_OUT]
    assert len(probs) == 36 + len(EXTRA_CONVS)
    for case, co, ks, st, act, x, w, bn, r in probs:
        def one(put):
            wp, bias = _packed(put, capf.pack_conv, w, bn, f"conv case {case}")
            return [capf.conv_nhwc(put(_nhwc(x)), wp, bias, ks, st, act, put(_nhwc(r)))]
        _twice(f"conv case {case} ({tuple(x.shape)} -> {co}, k{ks} s{st})", one)
    groupable = [p for p in probs if p[1] % 4 == 0]
    for i in range(0, len(groupable), 8):
        def group(put):
            ps = []
            for case, co, ks, st, act, x, w, bn, r in groupable[i:i + 8]:
                wp, bias = _packed(put, capf.pack_conv, w, bn, f"conv case {case}")
                ps.append((put(_nhwc(x)), wp, bias, ks, st, act, put(_nhwc(r))))
            return capf.conv_nhwc_group(ps)
        _twice(f"grouped fp32 convs {i}..", group)


# (M, N, K, act, residual, bias): M in {1, 31, 85, 257}, N in {4, 36, 100} and odd N
EXTRA_LINEARS = [(1, 4, 32, 0, False, True), (31, 36, 64, 2, True, True), (85, 100, 96, 1, False, False), (257, 33, 128, 0, True, True),
                 (1, 101, 160, 2, True, False), (257, 4, 32, 1, True, True), (31, 100, 640, 0, False, True), (85, 7, 32, 0, True, False)]


def _extra_linear_problems(seed, cases):
    g = torch.Generator().manual_seed(seed)
    for case, (M, N, K, act, res, has_b) in enumerate(cases):
        yield (100 + case, M, N, K, act, res, has_b, torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5,
               torch.randn(N, generator=g) if has_b else None, torch.randn(M, N, generator=g) if res else None)


def test_linear_f32_fuzz_guarded():
    """capf_op_linear on test_linear_fuzz_against_torch's 24 problems and the extra shapes (odd N, M = 1)"""
    n = 0
    for case, M, N, K, act, res, has_b, x, w, b, r in list(ops.linear_fuzz_problems()) + list(_extra_linear_problems(3, EXTRA_LINEARS)):
        _twice(f"linear case {case} M{M} N{N} K{K}", lambda put: [capf.linear(put(x), put(w), put(b), act=act, residual=put(r))])
        n += 1
    assert n == 24 + len(EXTRA_LINEARS)


def test_linear_entries_refuse_a_k_that_is_no_multiple_of_32():
    """K in {36, 100, 132}: refused by every stand-alone linear (so those K run as 1 x 1 convs and weight gradients here)"""
    x = torch.zeros(8, 132, device="cuda")
    for K in (36, 100, 132):
        w = torch.zeros(8, K, device="cuda")
        with pytest.raises(capf.CapfError):
            capf.linear(x[:, :K].contiguous(), w)
        with pytest.raises(capf.CapfError):
            capf.linear_f32h2g(x[:, :K].contiguous(), w, None, 8)
        with pytest.raises(capf.CapfError):
            capf.linear_ln_f32h2g(x[:, :K].contiguous(), w[0], w[0], 1e-5, w, None, 8)
        with pytest.raises(capf.CapfError):
            capf.linear_bf16(x[:, :K].contiguous().bfloat16(), w.bfloat16())


# ---- Winograd --------------------------------------------------------------------------------------------------------------------------------
WINO23 = [c for c in ops.WINO_CASES if c[4] * c[2] * c[3] * c[1] <= MAX_OUT] + [(32, 8, 1, 2, 5, 1, True), (64, 36, 5, 2, 3, 0, True), (32, 36, 9, 6, 2, 1, False)]
WINO43 = [(64, 64, 32, 32, 2, 1, True), (32, 32, 16, 64, 3, 1, False), (128, 128, 8, 8, 5, 0, True), (96, 96, 6, 12, 2, 1, True), (256, 64, 4, 4, 3, 1, False),
          (64, 160, 12, 8, 2, 1, True), (32, 8, 5, 4, 3, 1, True), (64, 36, 9, 8, 1, 0, False)]


@pytest.mark.parametrize("variant,cases", [(23, WINO23), (43, WINO43)], ids=["F(2,3)", "F(4,3)"])
def test_winograd_guarded(variant, cases):
    """capf_op_pack_conv_wino / capf_op_conv_wino on the cases of test_winograd_conv_matches_torch / test_winograd_f43_conv_matches_torch
    plus small and odd maps, and the first four of each again as one grouped launch"""
    g = torch.Generator().manual_seed(variant)
    made = []
    for ci, co, H, W, B, act, res in cases:
        x, w = torch.randn(B, H, W, ci, generator=g), torch.randn(co, ci, 3, 3, generator=g) / (9 * ci) ** 0.5
        bn, r = _bn(co, g), (torch.randn(B, H, W, co, generator=g) if res else None)
        made.append((x, w, bn, act, r))

        def one(put):
            wp, bias = _packed(put, capf.pack_conv_wino, w, bn, f"wino{variant}", variant=variant)
            return [capf.conv_nhwc_wino(put(x), wp, bias, act, put(r))]
        _twice(f"Winograd {variant} {ci}->{co} {H}x{W} B{B}", one)

    def group(put):
        ps = []
        for x, w, bn, act, r in made[:4]:
            wp, bias = _packed(put, capf.pack_conv_wino, w, bn, f"wino{variant}", variant=variant)
            ps.append((put(x), wp, bias, act, put(r)))
        return capf.conv_nhwc_wino_group(ps)
    _twice(f"grouped Winograd {variant}", group)


# ---- the 16-bit kernels ------------------------------------------------------------------------------------------------------------------------
def test_row_halo_fuzz_guarded():
    """capf_op_pack_conv_bf16_rh / capf_op_conv_bf16_rh on test_row_halo_fuzz_against_torch's 24 problems"""
    g = torch.Generator().manual_seed(4)
    for case, ci, co, H, W, B, act, res, x, w, bnp in ops.row_halo_fuzz_problems():
        r = torch.randn(B, co, H, W, generator=g).bfloat16() if res else None

        def one(put):
            wp, bias, cw = _packed(put, capf.pack_conv_bf16_rh, w, bnp, f"row-halo case {case}")
            return [capf.conv_nhwc_bf16_rh(put(_nhwc(x)), wp, bias, act, put(_nhwc(r)))]
        _twice(f"row-halo case {case}: Cin {ci} Cout {co} {H}x{W} B{B}", one)


@pytest.mark.parametrize("dtype", [capf.BF16, capf.F16], ids=["bf16", "fp16"])
def test_ws_fuzz_guarded(dtype):
    """the 2-D halo tile on test_ws_fuzz_against_torch's 28 problems, in both 16-bit formats (capf_op_pack_conv_16 layout 2 /
    capf_op_conv_16_ws_group; bf16 also through capf_op_pack_conv_bf16_ws / capf_op_conv_bf16_ws_group), the first three as one group"""
    t16 = torch.bfloat16 if dtype == capf.BF16 else torch.float16
    g = torch.Generator().manual_seed(5)
    kept = []
    for case, ci, co, H, W, B, act, res, x, w, bnp in ops.ws_fuzz_problems():
        if _out_elems(B, H, W, co) > MAX_OUT:
            continue
        x = x.float().to(t16)
        r = torch.randn(B, co, H, W, generator=g).to(t16) if res else None
        kept.append((co, act, x, w, bnp, r))

        def one(put):
            wp, bias = _packed(put, capf.pack_conv_16, w, bnp, f"halo-tile case {case}", layout=2, dtype=dtype)
            outs = capf.conv_nhwc_16_ws_group([(put(_nhwc(x)), wp, bias, act, put(_nhwc(r)), co)], dtype=dtype)
            if dtype == capf.BF16:
                wq, bq = _packed(put, capf.pack_conv_bf16_ws, w, bnp, f"halo-tile case {case} (bf16 entry)")
                outs += capf.conv_nhwc_bf16_ws_group([(put(_nhwc(x)), wq, bq, act, put(_nhwc(r)), co)])
            return outs
        _twice(f"halo-tile case {case}: Cin {ci} Cout {co} {H}x{W} B{B}", one)
    assert len(kept) >= 24

    def group(put):
        ps = []
        for co, act, x, w, bnp, r in kept[:3]:
            wp, bias = _packed(put, capf.pack_conv_16, w, bnp, "halo-tile group", layout=2, dtype=dtype)
            ps.append((put(_nhwc(x)), wp, bias, act, put(_nhwc(r)), co))
        return capf.conv_nhwc_16_ws_group(ps, dtype=dtype)
    _twice("grouped halo tile", group)


BF16_EXTRA = [(32, 8, 3, 1, 1, 1, 3), (64, 36, 3, 1, 1, 2, 5), (32, 20, 1, 1, 5, 3, 7), (96, 36, 3, 2, 9, 7, 3), (64, 8, 3, 2, 5, 3, 31), (128, 20, 1, 2, 9, 7, 2)]


@pytest.mark.parametrize("dtype", [capf.BF16, capf.F16], ids=["bf16", "fp16"])
def test_conv_16_guarded(dtype):
    """capf_op_pack_conv_16 layout 0 / capf_op_conv_16 on test_gpu_ops.BF16_CASES (up to 2 M outputs) and small / odd maps, stride 2 on odd
    maps, Cout 8 / 20 / 36 (the 16-bit kernels take Cout % 4 == 0); the four-conv grouped launch (capf_op_conv_16_group, row-halo packs alongside)"""
    t16 = torch.bfloat16 if dtype == capf.BF16 else torch.float16
    g = torch.Generator().manual_seed(6)
    cases = [c[:7] for c in ops.BF16_CASES if _out_elems(c[6], c[4], c[5], c[1], c[2], c[3]) <= MAX_OUT] + BF16_EXTRA
    for n, (ci, co, ks, st, H, W, B) in enumerate(cases):
        x, w, bn = torch.randn(B, H, W, ci, generator=g).to(t16), torch.randn(co, ci, ks, ks, generator=g) / (ci * ks * ks) ** 0.5, _bn(co, g)
        Ho, Wo = capf._out_hw(H, W, ks, st)
        r = torch.randn(B, Ho, Wo, co, generator=g).to(t16) if n % 2 else None

        def one(put):
            wp, bias = _packed(put, capf.pack_conv_16, w, bn, f"16-bit conv {n}", layout=0, dtype=dtype)
            return [capf.conv_nhwc_16(put(x), wp, bias, ks, st, n % 3 == 0, put(r), dtype=dtype)]
        _twice(f"16-bit conv {ci}->{co} k{ks} s{st} {H}x{W} B{B}", one)

    branch = [(torch.randn(5, hw, hw, c, generator=g).to(t16), torch.randn(c, c, 3, 3, generator=g) / (9 * c) ** 0.5, _bn(c, g),
               torch.randn(5, hw, hw, c, generator=g).to(t16)) for c, hw in ((32, 16), (64, 8), (128, 4), (256, 2))]

    def group(put):
        ps = []
        for x, w, bn, r in branch:
            wp, bias = _packed(put, capf.pack_conv_16, w, bn, "16-bit group", layout=0, dtype=dtype)
            wr, _ = _packed(put, capf.pack_conv_16, w, bn, "16-bit group (row-halo)", layout=1, dtype=dtype)
            ps.append((put(x), wp, bias, 3, 1, 1, put(r), wr))
        return capf.conv_nhwc_16_group(ps, dtype=dtype)[0]
    _twice("grouped 16-bit convs", group)


# (M, N, K, gelu, residual): K % 64 == 0 is the entry's condition
LINEAR16 = [(1, 4, 64, False, False), (31, 36, 128, True, False), (85, 100, 64, False, True), (257, 132, 192, True, False), (17, 640, 640, False, True),
            (300, 132, 64, False, False), (1, 100, 256, True, False), (257, 4, 64, False, True)]


@pytest.mark.parametrize("dtype", [capf.BF16, capf.F16], ids=["bf16", "fp16"])
def test_linear_16_guarded(dtype):
    """capf_op_linear_16 in both formats, capf_op_linear_bf16 for bf16: M 1 / 31 / 85 / 257, N 4 / 36 / 100, fp32 and 16-bit GELU outputs"""
    t16 = torch.bfloat16 if dtype == capf.BF16 else torch.float16
    g = torch.Generator().manual_seed(7)
    for M, N, K, gelu, res in LINEAR16:
        x, w, b = torch.randn(M, K, generator=g).to(t16), (torch.randn(N, K, generator=g) / K ** 0.5).to(t16), torch.randn(N, generator=g)
        r = torch.randn(M, N, generator=g) if res else None

        def one(put):
            outs = [capf.linear_16(put(x), put(w), put(b), put(r), gelu=gelu, dtype=dtype)]
            if dtype == capf.BF16:
                outs.append(capf.linear_bf16(put(x), put(w), put(b), put(r), gelu=gelu))
            return outs
        _twice(f"16-bit linear M{M} N{N} K{K} gelu={gelu}", one)


@pytest.mark.parametrize("first", [True, False], ids=["first", "identity"])
@pytest.mark.parametrize("dtype", [capf.BF16, capf.F16], ids=["bf16", "fp16"])
def test_bneck_16_guarded(dtype, first):
    """capf_op_bneck_16 at its smallest tile (8 x 8) on 3 frames, and at 16 x 24 on 5: with taps (t1, t2, shortcut are outputs) and without"""
    t16 = torch.bfloat16 if dtype == capf.BF16 else torch.float16
    g = torch.Generator().manual_seed(8 + first)
    cin = 64 if first else 256
    geo = [(cin, 64, 1), (64, 64, 3), (64, 256, 1)] + ([(64, 256, 1)] if first else [])
    ws = [(torch.randn(co, ci, ks, ks, generator=g) / (ci * ks * ks) ** 0.5, _bn(co, g)) for ci, co, ks in geo]
    for B, H, W in ((3, 8, 8), (5, 16, 24)):
        x = torch.randn(B, H, W, cin, generator=g).abs().to(t16)

        def one(put):
            packs = [_packed(put, capf.pack_conv_16, w, bn, "bottleneck", layout=0, dtype=dtype) for w, bn in ws]
            xd = put(x)
            y, t1, t2, sc = capf.bneck_16(xd, packs, tap=True, dtype=dtype)
            y0 = capf.bneck_16(xd, packs, tap=False, dtype=dtype)[0]
            return [y, t1, t2, sc, y0]
        _twice(f"bottleneck first={first} {H}x{W} B{B}", one)


# ---- the split-fp32 tiles -------------------------------------------------------------------------------------------------------------------------
def _tile_problems():
    kept = [p for p in ops.f32x3_fuzz_problems() if _out_elems(p[5], p[3], p[4], p[2]) <= MAX_OUT]
    g = torch.Generator().manual_seed(9)
    for n, (ci, co, H, W, B) in enumerate([(16, 8, 1, 1, 3), (32, 36, 1, 2, 5), (48, 8, 5, 3, 7), (64, 36, 9, 7, 3), (16, 36, 5, 3, 31)]):
        kept.append((100 + n, ci, co, H, W, B, n % 2, True, torch.randn(B, ci, H, W, generator=g), torch.randn(co, ci, 3, 3, generator=g) / (9 * ci) ** 0.5,
                     _bn(co, g), torch.randn(B, co, H, W, generator=g)))
    return kept


@pytest.mark.parametrize("which", ["f32x3", "f32h2"])
def test_split_fp32_tile_fuzz_guarded(which):
    """the 30 seeded problems test_f32x3_fuzz_against_torch and test_f32h2_fuzz_against_torch share, plus maps 1 x 1, 1 x 2, 5 x 3, 9 x 7 with
    Cout 8 / 36, through capf_op_pack_conv_f32x3 / _f32h2 and the tiles' grouped entry; the first four as ONE launch"""
    pack, run = {"f32x3": (capf.pack_conv_f32x3, capf.conv_nhwc_f32x3_group), "f32h2": (capf.pack_conv_f32h2, capf.conv_nhwc_f32h2_group)}[which]
    probs = _tile_problems()
    assert len(probs) >= 33
    for case, ci, co, H, W, B, act, res, x, w, bnp, r in probs:
        def one(put):
            wp, bias = _packed(put, pack, w, bnp, f"{which} case {case}")
            return run([(put(_nhwc(x)), wp, bias, act, put(_nhwc(r)) if res else None, co)])
        _twice(f"{which} tile case {case}: Cin {ci} Cout {co} {H}x{W} B{B}", one)

    def group(put):
        ps = []
        for case, ci, co, H, W, B, act, res, x, w, bnp, r in probs[:4]:
            wp, bias = _packed(put, pack, w, bnp, f"{which} group")
            ps.append((put(_nhwc(x)), wp, bias, act, put(_nhwc(r)) if res else None, co))
        return run(ps)
    _twice(f"grouped {which} tile", group)


def test_f32h2_planes_guarded():
    """a BasicBlock's conv1 -> conv2 on the two-fp16-piece tile with the planes tensor and its exponent table between them"""
    g = torch.Generator().manual_seed(10)
    for ci, H, W, B in ((128, 16, 16, 3), (256, 8, 8, 9), (128, 12, 9, 5), (64, 24, 18, 2)):        # (geometries of test_f32h2_planes_between_two_convs)
        x, r = torch.randn(B, H, W, ci, generator=g), torch.randn(B, H, W, ci, generator=g)
        w1, w2 = (torch.randn(ci, ci, 3, 3, generator=g) / (9 * ci) ** 0.5 for _ in range(2))
        b1, b2 = _bn(ci, g), _bn(ci, g)

        def one(put):
            p1, c1 = _packed(put, capf.pack_conv_f32h2, w1, b1, "planes conv1")
            p2, c2 = _packed(put, capf.pack_conv_f32h2, w2, b2, "planes conv2")
            planes, exps = capf.conv_nhwc_f32h2_planes(put(x), p1, c1, 1, None, ci, planes_out=True)
            y = capf.conv_nhwc_f32h2_planes(put(planes), p2, c2, 1, put(r), ci, exps_in=put(exps))
            return [planes, exps, y]
        _twice(f"planes {ci} {H}x{W} B{B}", one)


# ---- the two-fp16-piece GEMM --------------------------------------------------------------------------------------------------------------------
def test_f32h2g_conv_fuzz_guarded():
    """capf_op_pack_f32h2_gemm / capf_op_conv_f32h2g on test_f32h2g_conv_fuzz_against_torch's 24 problems and the extra shapes with
    Cout % 4 == 0 (Cin 36 / 100 / 132 among them: K % 32 != 0 under a Kpad of 32s); eight of them as one grouped launch"""
    probs = [p for p in ops.f32h2g_conv_fuzz_problems()]
    probs += [(c, ks, st, ci, co, H, W, B, act, res, x, w, bn, r if res else None)
              for c, ci, co, ks, st, H, W, B, act, res, x, w, bn, r in _extra_conv_problems(11, lambda ci, co, ks, st: co % 4 == 0)]
    probs = [p for p in probs if _out_elems(p[7], p[5], p[6], p[4], p[1], p[2]) <= MAX_OUT]
    assert len(probs) >= 24 + 7
    for case, ks, st, ci, co, H, W, B, act, res, x, w, bnp, r in probs:
        def one(put):
            wp, bias = _packed(put, capf.pack_f32h2_gemm, w, bnp, f"h2g conv case {case}")
            return [capf.conv_nhwc_f32h2g(put(_nhwc(x)), wp, bias, ks, st, act, put(_nhwc(r)), co)]
        _twice(f"h2g conv case {case}: {ci}->{co} k{ks} s{st} {H}x{W} B{B}", one)

    def group(put):
        ps = []
        for case, ks, st, ci, co, H, W, B, act, res, x, w, bnp, r in probs[-8:]:
            wp, bias = _packed(put, capf.pack_f32h2_gemm, w, bnp, "h2g group")
            ps.append((put(_nhwc(x)), wp, bias, ks, st, act, put(_nhwc(r)), co))
        return capf.conv_nhwc_f32h2g_group(ps)
    _twice("grouped h2g convs", group)


# (M, N, K, act, residual): N % 4 == 0 and K % 32 == 0 are the entry's conditions; the LayerNorm fold takes K <= 256
H2G_LINEARS = [(1, 4, 32, 0, False), (31, 36, 64, 2, True), (85, 100, 96, 0, True), (257, 4, 128, 1, False), (1, 100, 256, 2, True), (257, 36, 160, 0, False),
               (37, 52, 96, 2, True), (85, 640, 640, 0, True), (31, 132, 32, 0, False)]


def test_f32h2g_linears_guarded():
    """capf_op_linear_f32h2g, and capf_op_linear_ln_f32h2g where K <= 256: M 1 / 31 / 85 / 257, N 4 / 36 / 100"""
    g = torch.Generator().manual_seed(12)
    for M, N, K, act, res in H2G_LINEARS:
        x, w, b = torch.randn(M, K, generator=g), torch.randn(N, K, generator=g) / K ** 0.5, torch.randn(N, generator=g) * 0.1
        r = torch.randn(M, N, generator=g) if res else None
        gamma, beta = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.2

        def one(put):
            wp, _ = _packed(put, capf.pack_f32h2_gemm, w, None, f"h2g linear N{N} K{K}")
            outs = [capf.linear_f32h2g(put(x), wp, put(b), N, act, put(r))]
            if K <= 256:
                outs.append(capf.linear_ln_f32h2g(put(x), put(gamma), put(beta), 1e-6, wp, put(b), N, act, put(r)))
            return outs
        _twice(f"h2g linear M{M} N{N} K{K}", one)


# ---- the weight gradient ----------------------------------------------------------------------------------------------------------------------------
# fp32 kernel: test_gpu_ops.WGRAD_F32_NK plus N / K in {36, 100, 132} (multiples of 4, not of 32); two-piece kernel: its own list
WGRAD_EXTRA_NK = [(36, 100), (100, 132), (132, 36), (4, 36), (8, 100)]


@pytest.mark.parametrize("M", ops.WGRAD_M)
def test_wgrad_guarded(M):
    """capf_op_wgrad at test_gpu_ops.WGRAD_M rows, both kernels (up to 2 M output elements)"""
    g = torch.Generator().manual_seed(4000 + M)
    for two_piece, shapes in ((False, ops.WGRAD_F32_NK + WGRAD_EXTRA_NK), (True, ops.WGRAD_H2_NK)):
        for N, K in shapes:
            if N * K + N > MAX_OUT:
                continue
            dy, x = torch.randn(M, N, generator=g), torch.randn(M, K, generator=g)
            _twice(f"wgrad M{M} N{N} K{K} two_piece={two_piece}", lambda put: list(capf.wgrad(put(dy), put(x), two_piece)))


# ---- the loss, metric and preprocessing kernels (values: tests/test_gpu_metric_edges.py) --------------------------------------------------------
def test_pose_errors_and_segment_sums_guarded():
    """capf_pose_errors writes err[n, 4] and reads pose prev[i] and nothing behind the last pose; capf_segment_sums writes sums[S, 4] and
    counts[S, 2]: n around their blocks of 128 and 256, J from 3 to 32, a predecessor table and none, ids outside the segment table"""
    import numpy as np
    from mvn.datasets.human36m import previous_in_segment
    for n, J, S in ((1, 17, 1), (127, 3, 6), (129, 32, 7), (257, 17, 7), (1000, 16, 6)):
        rng = np.random.default_rng(n)
        pred, gt = torch.from_numpy(rng.standard_normal((n, J, 3)).astype(np.float32)), torch.from_numpy(rng.standard_normal((n, J, 3)).astype(np.float32))
        seg = rng.integers(-1, S + 1, n).astype(np.int32)
        prev = torch.from_numpy(previous_in_segment(seg))
        seg = torch.from_numpy(seg)

        def one(put):
            p, g, pv = put(pred), put(gt), put(prev)
            err, err0 = capf.pose_errors(p, g, pv), capf.pose_errors(p, g)
            sums, counts = capf.segment_sums(put(err), put(seg), pv, n_segments=S)
            sums0, counts0 = capf.segment_sums(put(err0))
            return [err, err0, sums, counts, sums0, counts0]
        _twice(f"pose_errors / segment_sums n{n} J{J} S{S}", one)


def test_mpjpe_entries_guarded():
    """capf_mpjpe and capf_mpjpe_nd (a thin ctypes call: mvn.models.loss.MPJPE is their only caller): one loss element, dpred[rows, D]"""
    import ctypes
    lib = capf.load_library()
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    g = torch.Generator().manual_seed(13)
    for rows, D in ((1, 3), (1023, 3), (1025, 3), (8705, 3), (1, 1), (1025, 2), (1023, 7), (2, 4)):
        pred, gt = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g)

        def one(put):
            p, t = put(pred), put(gt)
            stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            outs = []
            for entry in ("capf_mpjpe", "capf_mpjpe_nd") if D == 3 else ("capf_mpjpe_nd",):
                loss, dpred = torch.empty(1, device="cuda"), torch.empty(rows, D, device="cuda")
                dims = (rows,) if entry == "capf_mpjpe" else (rows, D)
                assert getattr(lib, entry)(stream, P(p), P(t), *dims, P(loss), P(dpred), 0.125) == 0
                outs += [loss, dpred]
            return outs
        _twice(f"mpjpe rows {rows} D {D}", one)


def test_keypoints_loss_guarded():
    """capf_keypoints_loss with its gradient in the three modes: rows around its block of 1024, D 1 to 4, validity [rows, 1]"""
    g = torch.Generator().manual_seed(14)
    for rows, D in ((1, 3), (17, 1), (1023, 2), (1025, 3), (3000, 4)):
        pred, gt, v = torch.randn(rows, D, generator=g), torch.randn(rows, D, generator=g), (torch.rand(rows, 1, generator=g) > 0.3).float()

        def one(put):
            p, t, w = put(pred), put(gt), put(v)
            return [o for mode in (0, 1, 2) for o in capf.keypoints_loss(mode, p, t, w, 0.5, want_grad=True)]
        _twice(f"keypoints_loss rows {rows} D {D}", one)


def test_preprocess_and_fliptest_fuse_guarded():
    """capf_preprocess (uint8 crops in, four outputs) at ragged image sizes in its three modes, with and without ground truth; the flip-test
    fusion at B 1 / 129 with the H36M table and a 32-joint caller table"""
    g = torch.Generator().manual_seed(15)
    for B, H, W in ((1, 8, 8), (5, 9, 7), (2, 256, 192)):
        img = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
        gt, k2d, kc = torch.randn(B, 1, 17, 3, generator=g), torch.rand(B, 17, 2, generator=g) * 2 - 1, torch.rand(B, 17, 2, generator=g) * 191
        for mode in (0, 1, 2):
            for backbone in ("hrnet_32", "cpn"):
                _twice(f"preprocess {B}x{H}x{W} mode {mode} {backbone}",
                       lambda put: list(capf.preprocess(put(img), put(gt) if mode != 2 or backbone == "cpn" else None, put(k2d), put(kc), backbone, mode)))
    swap32 = [j ^ 1 if j < 20 else j for j in range(32)]
    for B, J, swap in ((1, 17, None), (129, 17, None), (1, 32, swap32), (129, 32, swap32), (3, 1, [0])):
        p = torch.randn(2, B, 1, J, 3, generator=g)
        _twice(f"fliptest_fuse B{B} J{J}", lambda put: [capf.fliptest_fuse(put(p), swap)])


# ---- the JPEG decoders' scratch (its own contract: capf_jpeg_*_info's scratch_bytes) -----------------------------------------------------------
def test_jpeg_decoders_stay_inside_an_exact_poisoned_scratch():
    """capf_jpeg_decode and capf_jpeg_decode_batch on the eight goldens of tests/golden/jpeg_cases.npz: the wrappers allocate the scratch
    (exactly scratch_bytes), the outputs, the status and the coefficients with torch.empty -- here banded and pre-filled with 0x00, then with
    0xFF: every output equals its libjpeg golden under both fills, the coefficients are the same bits, no band changes"""
    import os
    import numpy as np
    from conftest import ROOT
    from test_gpu_jpeg_batch import CASES
    gold = np.load(os.path.join(ROOT, "tests", "golden", "jpeg_cases.npz"), allow_pickle=False)
    datas = [gold[n + ":jpeg"].tobytes() for n in CASES]
    kept = []
    for fill in BANDS:
        with wg.guarded_allocations(fill_byte=fill) as made:
            got = []
            for subseq in (0, 4):
                outs, status, coefs = capf.jpeg_decode_batch(datas, "cuda", subseq, True)
                torch.cuda.synchronize()
                assert not bool(status.any()), status
                got += [o.clone() for o in outs] + [c.clone() for cs in coefs for c in cs]
                for n, o in zip(CASES, outs):
                    assert np.array_equal(o.cpu().numpy(), gold[n + ":bgr"]), (n, subseq, fill)
            for n, d in zip(CASES, datas):
                one = capf.jpeg_decode(d, "cuda")
                torch.cuda.synchronize()
                assert np.array_equal(one.cpu().numpy(), gold[n + ":bgr"]), (n, fill)
            assert len(made) >= 2 * (len(CASES) + 2) + 2 * len(CASES)        # (outputs, status, scratch[, coefficients] per call)
        kept.append(got)
    assert all(torch.equal(a, b) for a, b in zip(*kept))
