"""GPU: the forward from uint8 crops -- normalisation, BGR flip and mirror in the stem conv's load (capf_forward_u8, capf_op_conv_u8).

Two kinds of check, neither with a tolerance of its own:
* against the byte formula of include/capf.h (one-hot taps): every output of a stem conv with one-hot weights IS one normalised input byte,
  so channel flip, mirror, frame mapping, zero padding and the handling of a misaligned base are pinned independently of capf_preprocess;
* against the float route (capf_preprocess + the float entry): same bits, at the op, through whole plans, through a training step, on a
  poisoned workspace and through the host package.
The one bound that is not "equal" is the suite's bound for fp32 convs against fp64 (tests/test_gpu_ops.py: 1e-6 of each output's sum of
|terms|), applied to the fp32 outputs of the op test."""
import contextlib
import copy
import functools
import hashlib
import io
import json
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import small_geometry_cases as sg
import workspace_guard as wg
from capf import lib as capf
from capf import synth
from conftest import ROOT
from test_gpu_workspace_hygiene import _inference_engine, _plan_model
from test_u8_input import STEMS

pytestmark = pytest.mark.gpu

F32, BF16, F16 = capf.F32, capf.BF16, capf.F16
TORCH_DT = {F32: torch.float32, BF16: torch.bfloat16, F16: torch.float16}
CPN_MEAN = [float(v) for v in (torch.tensor([122.7717, 115.9465, 102.9801]) / 255.0).tolist()]
J = 17


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _crops(shape, offset, seed):
    """uint8 [Bsrc,H,W,3] on the GPU as a dense view that starts `offset` bytes into a larger buffer (a misaligned base), random bytes with
    0 and 255 among them; the bytes around the view are 0x5A"""
    n = int(np.prod(shape))
    g = torch.Generator().manual_seed(seed)
    data = torch.randint(0, 256, (n,), generator=g, dtype=torch.uint8)
    data[torch.randperm(n, generator=g)[: max(2, n // 16)]] = 0
    data[torch.randperm(n, generator=g)[: max(2, n // 16)]] = 255
    buf = torch.full((n + 16,), 0x5A, dtype=torch.uint8)
    buf[offset:offset + n] = data
    dev = buf.cuda()
    view = dev[offset:offset + n].view(*shape)
    assert view.is_contiguous() and (view.data_ptr() - dev.data_ptr()) == offset
    return view, data.view(*shape).numpy()


def _constants(ks):
    """HRNet's constants for its 3x3 stem (and the 5x5 stand-in), CPN's mean-only form for the 7x7"""
    return (CPN_MEAN, None, "cpn") if ks == 7 else (list(capf.HRNET_MEAN), list(capf.HRNET_STD), "hrnet_32")


def _frames(bsrc, mode):
    return 2 * bsrc if mode == 2 else bsrc


def _formula_image(img_np, mode, mean, std):
    """the normalised RGB image [frames,H,W,3] the stem must see, from the header's byte formula and the HOST rule:
    byte ((bs * H + hi) * W + ws) * 3 + (2 - c), bs = f (modes 0, 1) or f mod Bsrc, ws = W - 1 - wi where the frame is mirrored"""
    Bsrc, H, W, _ = img_np.shape
    frames = _frames(Bsrc, mode)
    f = np.arange(frames).reshape(-1, 1, 1, 1)
    hi = np.arange(H).reshape(1, -1, 1, 1)
    wi = np.arange(W).reshape(1, 1, -1, 1)
    c = np.arange(3).reshape(1, 1, 1, -1)
    bs = f % Bsrc if mode == 2 else f
    mirrored = np.broadcast_to((f >= Bsrc) if mode == 2 else np.full_like(f, mode == 1, dtype=bool), (frames, 1, 1, 1))
    ws = np.where(mirrored, W - 1 - wi, wi)
    byte = img_np.reshape(-1)[((bs * H + hi) * W + ws) * 3 + (2 - c)]
    out = np.empty(byte.shape, dtype=np.float32)
    for ch in range(3):
        out[..., ch] = capf.input_rule_host(byte[..., ch], ch, mean, std)
    return torch.from_numpy(out)


# ---- 1. one-hot taps -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ks", [3, 7])
@pytest.mark.parametrize("H,W", [(9, 11), (6, 6)])
def test_one_hot_taps_read_the_byte_the_formula_names(ks, H, W):
    """identity BatchNorm, weight n of a 64-channel group = 1 at tap (kh, kw, c) and 0 elsewhere, stride 2, fp32 output: output channel n is
    input_rule_host of the formula's byte, or 0.0 for a tap outside the image -- bit for bit.  9 x 11 runs the streaming kernel (ks 3),
    6 x 6 (Wo = 3) leaves it; modes 0 / 1 / 2; the image starts 0..3 bytes into its buffer"""
    Bsrc, pad, taps = 3, ks // 2, ks * ks * 3
    mean, std, _ = _constants(ks)
    Ho, Wo = (H + 2 * pad - ks) // 2 + 1, (W + 2 * pad - ks) // 2 + 1
    packs = []
    for g0 in range(0, taps, 64):
        w = torch.zeros(64, 3, ks, ks)
        for n in range(min(64, taps - g0)):
            t = g0 + n
            w[n, t % 3, (t // 3) // ks, (t // 3) % ks] = 1.0
        packs.append(capf.pack_conv(w.cuda(), None))
    seen = set()
    for mode in (0, 1, 2):
        seen.add(capf.op_conv_u8_kernel_name(Bsrc, mode, H, W, 64, ks, 2, F32))
        for offset in (0, 1, 2, 3):
            view, img_np = _crops((Bsrc, H, W, 3), offset, seed=100 * ks + 10 * mode + offset)
            x = _formula_image(img_np, mode, mean, std)                                   # [frames, H, W, 3]
            xp = F.pad(x, (0, 0, pad, pad, pad, pad))                                      # zeros AFTER normalisation
            want = torch.empty(x.shape[0], Ho, Wo, taps)
            for t in range(taps):
                kh, kw, c = (t // 3) // ks, (t // 3) % ks, t % 3
                want[..., t] = xp[:, kh:kh + 2 * Ho:2, kw:kw + 2 * Wo:2, c]
            for gi, (wp, bias) in enumerate(packs):
                got = capf.op_conv_u8(view, wp, bias, ks, 2, 0, mode, mean, std, F32).cpu()
                n = min(64, taps - 64 * gi)
                w_g = want[..., 64 * gi:64 * gi + n]
                bad = (_bits(got[..., :n]) != _bits(w_g)).nonzero()
                assert bad.numel() == 0, (f"ks {ks} {H}x{W} mode {mode} offset {offset} group {gi}: {bad.shape[0]} outputs differ, first "
                                          f"(frame, ho, wo, tap) = {bad[0].tolist()}: got {got[tuple(bad[0])].item()!r} want {w_g[tuple(bad[0])].item()!r}")
                assert not got[..., n:].any()
    want_kernel = "igemm_f32_stem_stream<w4,64x64,u8>" if (ks == 3 and Wo >= 4) else "igemm_f32_smallc<w4,128x64,u8>"
    assert seen == {want_kernel}


# ---- 2. same bits as the float route, op level -----------------------------------------------------------------------------------------------
IMAGES = [(9, 11), (33, 35), (64, 48)]
STEM_OPS = sorted({(ks, co) for ks, co, _, _ in STEMS})             # the (ks, Cout) pairs of the CPU test's route table
OP_KERNELS = set()


@functools.lru_cache(maxsize=None)
def _random_pack(ks, cout):
    g = torch.Generator().manual_seed(1000 * ks + cout)
    w = torch.randn(cout, 3, ks, ks, generator=g) * 0.2
    bn = (torch.rand(cout, generator=g) + 0.5, torch.randn(cout, generator=g) * 0.1, torch.randn(cout, generator=g) * 0.1,
          torch.rand(cout, generator=g) + 0.5)
    wp, bias = capf.pack_conv(w.cuda(), tuple(t.cuda() for t in bn))
    sc = (bn[0] / torch.sqrt(bn[3] + 1e-5)).double()
    return wp, bias, w.double() * sc.view(-1, 1, 1, 1), wp.cpu()[:, :ks * ks * 3], bias.cpu()


def _digest(t):
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def _bits_key(dtype, ks, cout, H, W, bsrc, mode, act):
    return f"{dtype},{ks},{cout},{H},{W},{bsrc},{mode},{act}"


@functools.lru_cache(maxsize=None)
def _stem_bits():
    """sha256 of the float stem op's output bytes per case of the test below, recorded from the library as it stood before the five stem
    kernels got a translation unit, a route and a launcher of their own (tests/golden/stem_bits.json: case keys and digests only)"""
    with open(os.path.join(ROOT, "tests", "golden", "stem_bits.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("dtype", [F32, BF16, F16], ids=["fp32", "bf16", "fp16"])
@pytest.mark.parametrize("ks,cout", STEM_OPS, ids=[f"k{k}c{c}" for k, c in STEM_OPS])
def test_u8_op_equals_the_float_op_on_preprocessed_images(dtype, ks, cout):
    """random weights with random BatchNorm, ReLU on / off; 9 x 11, 33 x 35 (several tiles, ragged last tile) and 64 x 48; 1 and 5 source
    frames; modes 0 / 1 / 2.  fp32 outputs also against fp64 F.conv2d of the normalised image at 1e-6 of each output's sum of |terms|.
    The float op's own bits are the recorded ones (_stem_bits)"""
    wp, bias, w_fold, w_packed, bias_cpu = _random_pack(ks, cout)
    mean, std, backbone = _constants(ks)
    pad = ks // 2
    # the packed weights ARE the fold (K order (kh, kw, c)): the fp64 reference multiplies the fp32 values the kernel multiplies
    w64 = w_packed.double().view(cout, ks, ks, 3).permute(0, 3, 1, 2).contiguous()
    assert torch.allclose(w64, w_fold, rtol=1e-6, atol=1e-9)
    k = torch.zeros(5, J, 2, device="cuda")
    compares, elems, worst, nonzero = 0, 0, 0.0, 0
    for (H, W) in IMAGES:
        for bsrc in (1, 5):
            for mode in (0, 1, 2):
                frames = _frames(bsrc, mode)
                view, _ = _crops((bsrc, H, W, 3), (H + bsrc + mode) % 4, seed=H * 1000 + bsrc * 10 + mode)
                x = capf.preprocess(view, None, k[:bsrc], k[:bsrc], backbone, mode)[0].view(frames, H, W, 3)
                name = capf.op_conv_u8_kernel_name(bsrc, mode, H, W, cout, ks, 2, dtype)
                ref_name = capf.stem_kernel_name(frames, H, W, cout, ks, 2, dtype)
                assert name == ref_name[:-1] + ",u8>"
                OP_KERNELS.add(name)
                for act in (0, 1):
                    if dtype == F32:
                        want = capf.conv_nhwc(x, wp, bias, ks, 2, act)
                    else:
                        want = capf.conv_nhwc_16(x, wp, bias, ks, 2, act, dtype=dtype)
                    assert _digest(want) == _stem_bits()[_bits_key(dtype, ks, cout, H, W, bsrc, mode, act)], \
                        f"{ref_name}: {H}x{W} Bsrc {bsrc} mode {mode} act {act}: the float stem op's bits are not the recorded ones"
                    got = capf.op_conv_u8(view, wp, bias, ks, 2, act, mode, mean, std, dtype)
                    assert got.dtype == TORCH_DT[dtype]
                    compares += 1
                    elems += got.numel()
                    nonzero += int((got.float() != 0).sum().item())
                    assert _same(got, want), f"{name}: {H}x{W} Bsrc {bsrc} mode {mode} act {act}: differs from {ref_name} on capf_preprocess's output"
                    if dtype == F32:
                        xd = x.double().cpu().permute(0, 3, 1, 2)
                        ref = F.conv2d(xd, w64, bias_cpu.double(), 2, pad)
                        mass = F.conv2d(xd.abs(), w64.abs(), bias_cpu.double().abs(), 2, pad)
                        if act:
                            ref = F.relu(ref)
                        err = ((got.double().cpu().permute(0, 3, 1, 2) - ref).abs() / mass).max().item()
                        worst = max(worst, err)
                        assert err <= 1e-6, f"{name}: {H}x{W} Bsrc {bsrc} mode {mode} act {act}: {err:.3e} of the sum of |terms|"


    print(f"u8 op k{ks} c{cout} dtype {dtype}: {compares} bit comparisons over {elems} outputs ({nonzero} non-zero), "
          + (f"worst fp64 figure {worst:.3e} of the sum of |terms|" if dtype == F32 else "fp64 figure n/a (fp32 outputs only)"))
    assert compares == len(IMAGES) * 2 * 3 * 2 and nonzero > elems // 4


def test_the_op_test_reached_every_stem_kernel():
    """the (ks, Cout) x image x batch x mode table of the test above reaches the U8 form of all five Cin = 3 kernels, in both 16-bit
    formats (asked of the name query, so that it holds whichever cases ran)"""
    for dtype in (F32, BF16, F16):
        for ks, cout in STEM_OPS:
            for H, W in IMAGES:
                for bsrc in (1, 5):
                    for mode in (0, 1, 2):
                        OP_KERNELS.add(capf.op_conv_u8_kernel_name(bsrc, mode, H, W, cout, ks, 2, dtype))
    fam = {n.split("<")[0] for n in OP_KERNELS}
    assert fam >= {"igemm_f32_stem_stream", "igemm_f32_smallc", "igemm_bf16_stem_stream", "igemm_bf16_stem", "igemm_bf16_smallc",
                   "igemm_f16_stem_stream", "igemm_f16_stem", "igemm_f16_smallc"}, fam
    assert all(n.endswith(",u8>") for n in OP_KERNELS)


# ---- 3. same bits, whole plans ---------------------------------------------------------------------------------------------------------------
# the small-geometry table's HRNet-32 fp32 / bf16 / fp16 and CPN fp32 / bf16 plans at their smallest geometries, plus one non-square HRNet-32
# crop (64 x 96: capf_create takes multiples of 32 only, so 64 x 48 is not a plan)
def _smallest(backbone, dtype):
    rows = [r for r in sg.ROWS if r.backbone == backbone and r.dtype == dtype and r.plan_flags == "0"]
    return min(((r.H * r.W, r.H, r.W) for r in rows))[1:]


PLANS = [(bb, dt) + _smallest(bb, dt) for bb, dt in (("hrnet_32", "fp32"), ("hrnet_32", "bf16"), ("hrnet_32", "fp16"), ("cpn", "fp32"),
                                                     ("cpn", "bf16"))] + [("hrnet_32", "fp32", 64, 96)]
PLAN_IDS = [f"{p[0]}-{p[2]}x{p[3]}-{p[1]}" for p in PLANS]


def _points(B, H, W, seed):
    _, k2d, kc = synth.synth_inputs(B, H, W, seed=seed, crop_range=(W, H))
    return k2d.cuda(), kc.cuda()


def _float_route(eng, crops, k2d_src, kc_src, backbone, mode, run):
    """capf_preprocess + the float entry -> (out, kcrop, feat0..3, stem)"""
    img, _, k2d, kc = capf.preprocess(crops, None, k2d_src, kc_src, backbone, mode)
    B = _frames(crops.shape[0], mode)
    img, k2d, kc = img.view(B, *crops.shape[1:]), k2d.view(B, J, 2).contiguous(), kc.view(B, J, 2).contiguous()
    out = torch.full((B, 1, J, 3), float("nan"), device="cuda")
    run(eng, img, k2d, kc, out)
    return [out, kc] + [eng.tensor(f"feat{l}") for l in range(4)] + [eng.tensor("stem")]


def _u8_route(eng, crops, k2d_src, kc_src, backbone, mode, run):
    _, k2d, kc = capf.preprocess_points(None, k2d_src, kc_src, mode)
    B = _frames(crops.shape[0], mode)
    k2d, kc = k2d.view(B, J, 2).contiguous(), kc.view(B, J, 2).contiguous()
    out = torch.full((B, 1, J, 3), float("nan"), device="cuda")
    run(eng, crops, capf.input_constants(backbone), mode, k2d, kc, out)
    return [out, kc] + [eng.tensor(f"feat{l}") for l in range(4)] + [eng.tensor("stem")]


NAMES = ["joints", "kcrop", "feat0", "feat1", "feat2", "feat3", "stem"]


@pytest.mark.parametrize("backbone,dtype,H,W", PLANS, ids=PLAN_IDS)
def test_forward_u8_equals_preprocess_plus_forward(backbone, dtype, H, W):
    """batches 1, 2, 6; modes 0 / 1 and, with batch = 2 Bsrc, 2: joints, the crop keypoints, feat0..3 and the stem tensor bit for bit; and
    capf_backbone_forward_u8 + capf_lifter_forward against capf_forward_u8"""
    model = _plan_model(backbone, dtype, "0")
    bb = "cpn" if backbone == "cpn" else "hrnet_32"
    with torch.no_grad():
        eng = model._engine_at(torch.device("cuda", torch.cuda.current_device()), H, W)
        assert eng.op_table(1)[0][1].startswith(("igemm_f32_s", "igemm_bf16_s", "igemm_f16_s"))
        for batch in (1, 2, 6):
            for mode in (0, 1, 2):
                if mode == 2 and batch % 2:
                    continue
                bsrc = batch // 2 if mode == 2 else batch
                crops, _ = _crops((bsrc, H, W, 3), (batch + mode) % 4, seed=7 * batch + mode)
                k2d, kc = _points(bsrc, H, W, seed=batch)
                want = _float_route(eng, crops, k2d, kc, bb, mode, lambda e, img, a, b, o: e.forward(img, a, b, o, _stream()))
                got = _u8_route(eng, crops, k2d, kc, bb, mode,
                                lambda e, c, ms, m, a, b, o: e.forward_u8(c, ms[0], ms[1], m, a, b, o, _stream()))

                def two_calls(e, c, ms, m, a, b, o):
                    e.backbone_forward_u8(c, ms[0], ms[1], m, _stream())
                    e.lifter_forward(a, b, o, _stream())
                two = _u8_route(eng, crops, k2d, kc, bb, mode, two_calls)
                assert bool(torch.isfinite(want[0]).all())
                for name, w, g, t in zip(NAMES, want, got, two):
                    assert _same(g, w), f"batch {batch} mode {mode}: {name} of capf_forward_u8 differs from capf_preprocess + capf_forward"
                    assert _same(t, g), f"batch {batch} mode {mode}: {name} of capf_backbone_forward_u8 + capf_lifter_forward differs from capf_forward_u8"


# ---- 4. training -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batch", [2, 6])
def test_training_step_from_uint8_crops_has_the_float_routes_bits(batch):
    """HRNet-32 32 x 64, DropPath masks on, modes 0 / 1: the loss and all 191 gradients of capf_forward_train_u8 + capf_backward are the
    float route's"""
    from mvn.models.loss import MPJPE
    H, W = 32, 64
    model = _plan_model("hrnet_32", "fp32", "0")
    model.train(); model.backbone.eval()
    model.drop_path_rate = 0.2
    try:
        dev = torch.device("cuda", torch.cuda.current_device())
        eng = model._engine_at(dev, H, W)
        assert eng.cfg.training == 1
        layout, total = eng.grad_layout_cached()
        assert len(layout) == 191
        torch.manual_seed(batch)
        masks = model._drop_masks(batch, dev)
        assert masks is not None and bool((masks == 0).any())
        gt = synth.synth_inputs(batch, H, W, seed=3, with_gt=True)[3].cuda()
        k2d_src, kc_src = _points(batch, H, W, seed=batch + 1)
        for mode in (0, 1):
            crops, _ = _crops((batch, H, W, 3), mode + 1, seed=11 * batch + mode)
            res = []
            for route in ("float", "u8"):
                out = torch.empty(batch, 1, J, 3, device="cuda")
                if route == "float":
                    img, _, k2d, kc = capf.preprocess(crops, None, k2d_src, kc_src, "hrnet_32", mode)
                    eng.forward_train(img, k2d, kc, out, _stream(), masks)
                else:
                    _, k2d, kc = capf.preprocess_points(None, k2d_src, kc_src, mode)
                    m3, s3 = capf.input_constants("hrnet_32")
                    eng.forward_train_u8(crops, m3, s3, mode, k2d, kc, out, _stream(), masks)
                pred = out.clone().requires_grad_(True)
                loss = MPJPE()(pred, gt)
                loss.backward()
                flat = torch.full((total,), float("nan"), device="cuda")
                eng.backward(pred.grad.contiguous(), flat, _stream(), masks)
                res.append((loss.detach().clone(), flat, out.clone()))
            (l0, f0, o0), (l1, f1, o1) = res
            assert bool(torch.isfinite(f0).all()) and _same(o1, o0) and _same(l1, l0)
            print(f"train batch {batch} mode {mode}: loss {l0.item():.6f} / {l1.item():.6f}, {total} gradient elements, "
                  f"{int((f0 != 0).sum().item())} non-zero, |g| max {f0.abs().max().item():.3e}")
            assert int((f0 != 0).sum().item()) > total // 2
            for name, (off, n) in layout.items():
                assert _same(f1[off:off + n], f0[off:off + n]), f"batch {batch} mode {mode}: gradient of {name}"
    finally:
        model.eval()


# ---- 5. workspace guard ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp32", "bf16", "fp16"])
def test_forward_u8_on_the_poisoned_workspace(dtype):
    """one u8 forward per dtype on the exact-size, banded, NaN-filled workspace (training = 0 handle: the arena ends at the band): the bits
    of a clean workspace, every band intact -- the crops' own included (no byte outside [images, images + Bsrc H W 3) is even readable as
    anything but band)"""
    H, W, bsrc, mode = 64, 64, 3, 2
    model = _plan_model("hrnet_32", dtype, "0")
    with torch.no_grad():
        eng = _inference_engine(model, H, W)
        crops, _ = _crops((bsrc, H, W, 3), 1, seed=5)
        k2d_src, kc_src = _points(bsrc, H, W, seed=6)
        _, k2d, kc = capf.preprocess_points(None, k2d_src, kc_src, mode)
        k2d, kc = k2d.view(2 * bsrc, J, 2).contiguous(), kc.view(2 * bsrc, J, 2).contiguous()
        m3, s3 = capf.input_constants("hrnet_32")
        ws = wg.install(eng, 2 * bsrc, 0x00)
        res = []
        for fill in (0x00, 0xFF):
            ws.refill(fill)
            c, a, b = wg.flush(crops, fill), wg.flush(k2d, fill), wg.flush(kc.clone(), fill)
            out = wg.filled((2 * bsrc, 1, J, 3), torch.float32, "cuda", fill)
            eng.forward_u8(c, m3, s3, mode, a, b, out, _stream())
            ws.check(f"workspace under fill 0x{fill:02X}")
            wg.check_all((c, a, b, out), f"(crops, k2d, kcrop, out) under fill 0x{fill:02X}")
            res.append((out.clone(), b.clone(), [eng.tensor(f"feat{l}") for l in range(4)]))
    (o0, k0, f0), (o1, k1, f1) = res
    assert bool(torch.isfinite(o0).all()) and _same(o1, o0) and _same(k1, k0)
    for a, b in zip(f0, f1):
        assert _same(b, a)


# ---- 6. host package ---------------------------------------------------------------------------------------------------------------------------
def _host_model(backbone="hrnet_32"):
    from conftest import make_model
    return make_model(backbone, device="cuda", wseed=9)[0]


@pytest.fixture(scope="module")
def host_model():
    return _host_model()


def _batch(B, H=64, W=64, seed=5):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8), torch.randn(B, 1, J, 3, generator=g),
            torch.rand(B, J, 2, generator=g) * 2 - 1, torch.rand(B, J, 2, generator=g) * (W - 1))


@pytest.mark.parametrize("mirror,mode", [("none", 0), ("all", 1), ("pair", 2)])
def test_ca_pf_forward_u8_against_forward_on_preprocessed_inputs(host_model, mirror, mode):
    B = 3
    img, gt, k2d, kc = (t.cuda() for t in _batch(B))
    with torch.no_grad():
        x, _, a, b = capf.preprocess(img, gt, k2d, kc, "hrnet_32", mode)
        frames = _frames(B, mode)
        want_kc = b.view(frames, J, 2).clone()
        want = host_model(x.view(frames, 64, 64, 3), a.view(frames, J, 2), want_kc)
        _, a8, b8 = capf.preprocess_points(gt, k2d, kc, mode)
        assert _same(a8, a) and _same(b8, b)
        got_kc = b8.view(frames, J, 2).clone()
        got = host_model.forward_u8(img, a8.view(frames, J, 2), got_kc, mirror=mirror)
    assert got.shape == (frames, 1, J, 3) and _same(got, want) and _same(got_kc, want_kc)
    if mode == 2:       # ... and fused: today's single-forward flip test
        with torch.no_grad():
            fused = host_model.forward_flip_test(x, a, b.clone())
        assert _same(capf.fliptest_fuse(got.view(2, B, 1, J, 3)), fused)


def test_mpi_variant_forward_u8():
    from model.conpose import VolumetricTriangulationNet, mpi_preset
    from mvn.utils.cfg import config
    with contextlib.redirect_stdout(io.StringIO()):
        m = VolumetricTriangulationNet(mpi_preset(copy.deepcopy(config), "hrnet_32")).eval()
    synth.load_synthetic(m, seed=4, bn_mode="random")
    m = m.cuda()
    img, gt, k2d, kc = (t.cuda() for t in _batch(2, seed=8))
    with torch.no_grad():
        x, _, a, b = capf.preprocess(img, None, k2d, kc, "hrnet_32", 1)
        want, none = m(x, a, b.clone())
        got, none8 = m.forward_u8(img, a, b.clone(), mirror="all")
    assert none is None and none8 is None and got.shape == (2, 3, 1, J, 1) and _same(got, want)


def test_loss_backward_through_forward_u8(host_model):
    from mvn.models.loss import MPJPE
    B = 2
    img, gt, k2d, kc = (t.cuda() for t in _batch(B, seed=12))
    x, gt_rel, a, b = capf.preprocess(img, gt, k2d, kc, "hrnet_32", 1)
    model = host_model
    model.train(); model.backbone.eval()
    try:
        grads = []
        for route in ("float", "u8"):
            model.zero_grad(set_to_none=True)
            torch.manual_seed(31)                                 # the DropPath masks of both steps
            pred = model(x, a, b.clone()) if route == "float" else model.forward_u8(img, a, b.clone(), mirror="all")
            loss = MPJPE()(pred, gt_rel)
            loss.backward()
            grads.append((loss.detach().clone(), {n: p.grad.clone() for n, p in model.volume_net.named_parameters()}))
    finally:
        model.eval()
        model.zero_grad(set_to_none=True)
    assert len(grads[0][1]) == 191 and _same(grads[1][0], grads[0][0])
    for n, g in grads[0][1].items():
        assert _same(grads[1][1][n], g), n


@pytest.mark.parametrize("is_train,flip_test,coin", [(True, False, 0.25), (True, False, 0.75), (False, True, 0.0), (False, False, 0.0)])
def test_prefetcher_fused_input_feeds_forward_u8(host_model, monkeypatch, is_train, flip_test, coin):
    """data_prefetcher(fused_input=True) -> forward_u8 against fused_input=False -> forward, in both train-flip outcomes, the flip test and
    the plain evaluation; fused_input=False itself bit for bit against capf.preprocess"""
    from mvn.datasets.utils import data_prefetcher
    monkeypatch.setattr(random, "random", lambda: coin)
    B = 2
    batch = _batch(B, seed=21)
    mode = 1 if (is_train and coin <= 0.5) else 2 if (not is_train and flip_test) else 0
    dev = torch.device("cuda", torch.cuda.current_device())
    plain = data_prefetcher([batch], dev, is_train, flip_test, "hrnet_32")
    assert plain.fused_input is False
    images, gt, k2d, kc = plain.next()
    assert plain.next() is None
    x, g, a, b = capf.preprocess(*(t.cuda() for t in batch), "hrnet_32", mode)
    if mode == 2:
        x, a, b = x.transpose(0, 1), a.transpose(0, 1), b.transpose(0, 1)
    for got, want in ((images, x), (gt, g), (k2d, a), (kc, b)):
        assert got.shape == want.shape and _same(got, want)

    fused = data_prefetcher([batch], dev, is_train, flip_test, "hrnet_32", fused_input=True)
    crops, gt8, k2d8, kc8 = fused.next()
    assert fused.mirror == ("none", "all", "pair")[mode] and fused.next() is None
    assert crops.dtype == torch.uint8 and crops.shape == (B, 64, 64, 3) and torch.equal(crops.cpu(), batch[0]) and _same(gt8, gt)
    with torch.no_grad():
        got = host_model.forward_u8(crops, k2d8, kc8.clone(), mirror=("none", "all", "pair")[mode])
        if mode == 2:
            want = host_model.forward_flip_test(images.transpose(0, 1).contiguous(), k2d.transpose(0, 1).contiguous(),
                                                kc.transpose(0, 1).contiguous().clone())
            got = capf.fliptest_fuse(got.view(2, B, 1, J, 3))
        else:
            want = host_model(images, k2d, kc.clone())
    assert _same(got, want)


def test_forward_u8_argument_errors(host_model):
    img, gt, k2d, kc = (t.cuda() for t in _batch(3, seed=2))
    with torch.no_grad():
        with pytest.raises(TypeError, match="uint8"):
            host_model.forward_u8(img.float(), k2d, kc.clone())
        with pytest.raises(ValueError, match="contiguous"):
            host_model.forward_u8(img.transpose(1, 2), k2d, kc.clone())
        with pytest.raises(capf.CapfError, match="no CPU fallback"):
            host_model.forward_u8(img.cpu(), k2d.cpu(), kc.cpu())
        with pytest.raises(ValueError, match="is on"):
            host_model.forward_u8(img, k2d.cpu(), kc.clone())
        with pytest.raises(ValueError, match="mirror='pair'"):
            host_model.forward_u8(img, k2d, kc.clone(), mirror="pair")          # [B,17,2] keypoints for 2B engine frames
        with pytest.raises(ValueError, match="mirror='pair'"):
            host_model.forward_u8(img, torch.cat([k2d, k2d[:2]]), torch.cat([kc, kc[:2]]), mirror="pair")     # an odd 2B
        with pytest.raises(ValueError, match="mirror must be"):
            host_model.forward_u8(img, k2d, kc.clone(), mirror="both")
        with pytest.raises(TypeError, match="float32"):
            host_model.forward_u8(img, k2d.double(), kc.clone())
        # forward itself keeps its float32 check
        with pytest.raises(TypeError, match="float32"):
            host_model(img, k2d, kc.clone())
