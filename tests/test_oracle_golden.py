"""CPU: the oracle (oracle/capf_oracle.py) reproduces the golden vectors that oracle/make_goldens.py
captured from the REAL reference — this is what pins the oracle (the reference has no tests)."""
import numpy as np
import pytest
import torch

import capf_oracle as oracle
from conftest import load_golden, make_model
from golden_cases import CASES, case_inputs

TOL = 2e-5   # oracle and reference run the same ATen CPU kernels; only thread-count reassociation differs


@pytest.mark.parametrize("name", [n for n in CASES if not CASES[n].get("mpi")])
def test_oracle_matches_reference_golden(name):
    case = CASES[name]
    g = load_golden(name)
    _, sd = make_model(case["backbone"], wseed=case["wseed"], bn=case["bn"])
    img, k2d, kc = case_inputs(case)
    taps = {}
    with torch.no_grad():
        out = oracle.ca_pf_forward(sd, img, k2d, kc, backbone=case["backbone"], taps=taps)
    assert out.shape == (case["B"], 1, 17, 3)
    np.testing.assert_allclose(out.numpy(), g["out"], atol=TOL, rtol=0)
    np.testing.assert_array_equal(kc.numpy(), g["ref"])          # in-place normalisation, bit exact
    for l, f in enumerate(taps["features"]):
        assert tuple(f.shape) == tuple(g[f"feat{l}_shape"])
        np.testing.assert_allclose(f.double().sum().item(), g[f"feat{l}_sum"], rtol=1e-5, atol=1e-2)
        np.testing.assert_allclose(f.double().abs().sum().item(), g[f"feat{l}_abs"], rtol=1e-5)
        h0, w0 = f.shape[2] // 3, f.shape[3] // 3
        np.testing.assert_allclose(f[:, :, h0:h0 + 4, w0:w0 + 4].permute(0, 2, 3, 1).numpy(), g[f"feat{l}_slice"], atol=TOL)
        np.testing.assert_allclose(taps["sampled"][l].numpy(), g[f"sampled{l}"], atol=TOL)
    np.testing.assert_allclose(taps["tokens_ctx"].numpy(), g["tok_ctx"], atol=TOL)
    B = case["B"]
    np.testing.assert_allclose(taps["tokens_res"].numpy().reshape(B * 17, 5, -1), g["tok_res"], atol=TOL)
    np.testing.assert_allclose(taps["tokens_joint"].numpy(), g["tok_joint"], atol=5 * TOL)


@pytest.mark.parametrize("name", ["w32_256x256_adv", "w32_256x256_b2"])
def test_explicit_bilinear_restatement(name):
    """The numpy index arithmetic (bilinear_corners) gives the same samples as ATen grid_sample on
    in-range, out-of-range and pixel-boundary keypoints, for both padding modes."""
    case = CASES[name]
    g = load_golden(name)
    _, sd = make_model(case["backbone"], wseed=case["wseed"], bn=case["bn"])
    img, k2d, kc = case_inputs(case)
    with torch.no_grad():
        out = oracle.ca_pf_forward(sd, img, k2d, kc, backbone=case["backbone"], explicit=True)
    np.testing.assert_allclose(out.numpy(), g["out"], atol=1e-5, rtol=0)


def test_bilinear_corners_edge_cases():
    g = np.array([[-1.0, -1.0], [1.0, 1.0], [-0.0, 0.0], [1.5, -1.2], [np.nextafter(np.float32(1), 0), 0.3]], np.float32)
    z = oracle.bilinear_corners(g, 64, 48, "zeros")
    b = oracle.bilinear_corners(g, 64, 48, "border")
    assert z["ix0"].tolist()[:3] == [0, 47, 23] and z["iy0"].tolist()[:3] == [0, 63, 31]
    assert not z["valid"][3].all() and b["ix0"][3] == 47 and b["iy0"][3] == 0
    assert z["valid"][1].tolist() == [True, False, False, False]      # SE/NE/SW fall outside at +1
    assert b["wx1"][1] == 0.0 and b["wy1"][1] == 0.0


def test_mpjpe_matches_definition():
    p, q = torch.randn(3, 1, 17, 3), torch.randn(3, 1, 17, 3)
    want = ((p - q) ** 2).sum(-1).sqrt().mean()
    assert abs(oracle.mpjpe(p, q).item() - want.item()) < 1e-6


def _mpi_model(case, device=None):
    import copy, contextlib, io
    from capf import synth
    from model.conpose import VolumetricTriangulationNet, mpi_preset
    from mvn.utils.cfg import config
    cfg = mpi_preset(copy.deepcopy(config), case["backbone"])
    if case.get("depth"):
        cfg.model.poseformer.depth = case["depth"]
    with contextlib.redirect_stdout(io.StringIO()):
        m = VolumetricTriangulationNet(cfg).eval()
    sd = synth.load_synthetic(m, seed=case["wseed"], bn_mode=case["bn"])
    return (m.to(device) if device else m), sd


@pytest.mark.parametrize("name", [n for n in CASES if CASES[n].get("mpi")])
def test_oracle_matches_mpi_variant_golden(name):
    """the MPI-INF-3DHP model (no deformable blocks, embed 64 with HRNet-32 / 96 with HRNet-48, output
    [B,3,1,17,1]) — goldens captured from ContextPose_mpi/model/conpose.py; also pins the variant's state_dict names."""
    case = CASES[name]
    g = load_golden(name)
    m, sd = _mpi_model(case)
    assert sorted(m.state_dict().keys()) == sorted(str(n) for n in g["schema_names"])
    img, k2d, kc = case_inputs(case)
    with torch.no_grad():
        ref = oracle.normalise_crop_keypoints_(kc)
        feats = oracle.hrnet_forward(sd, img.permute(0, 3, 1, 2).contiguous())
        out = oracle.lifter_forward(sd, k2d, ref, feats, context_blocks=False, depth=case.get("depth"))   # [B,1,17,3]
    out = out.view(case["B"], 1, 17, 3, 1).permute(0, 3, 1, 2, 4)
    np.testing.assert_allclose(out.numpy(), g["out"], atol=TOL, rtol=0)
    np.testing.assert_array_equal(kc.numpy(), g["ref"])


def test_prefetch_preprocess_hand_computed():
    """N1 pin: one pixel / a few joints worked out by hand (datasets/utils.py:45-65)."""
    img = torch.zeros(1, 2, 3, 3, dtype=torch.uint8)
    img[0, 0, 0] = torch.tensor([255, 0, 128])                 # B, G, R
    gt = torch.zeros(1, 1, 17, 3); gt[0, 0, 0] = torch.tensor([1.0, 2.0, 3.0]); gt[0, 0, 4] = torch.tensor([2.0, 2.0, 2.0])
    k2d = torch.zeros(1, 17, 2); k2d[0, 1] = torch.tensor([0.25, -0.5])
    kc = torch.zeros(1, 17, 2); kc[0, 1] = torch.tensor([10.0, 20.0])
    im, g, k, c = oracle.prefetch_preprocess(img, gt, k2d, kc, "hrnet_32", is_train=True, flip=True)
    # the pixel moves from w=0 to w=2 and its channels become (R, G, B) = (128, 0, 255)
    want = (torch.tensor([128.0, 0.0, 255.0]) * torch.tensor(1.0).div(255.0) - torch.tensor([0.485, 0.456, 0.406])) / torch.tensor([0.229, 0.224, 0.225])
    assert torch.equal(im[0, 0, 2], want)
    assert g[0, 0, 0].tolist() == [-0.0, 0.0, 0.0]
    assert g[0, 0, 1].tolist() == [-1.0, 0.0, -1.0]            # joint 4 (left) lands on joint 1 (right), x negated
    assert k[0, 4].tolist() == [-0.25, -0.5] and k[0, 1].tolist() == [-0.0, 0.0]
    assert c[0, 4].tolist() == [181.0, 20.0] and c[0, 1].tolist() == [191.0, 0.0]
    # flip-test stacking and its fusion are inverse bookkeeping
    im2, g2, k2, c2 = oracle.prefetch_preprocess(img, gt, k2d, kc, "cpn", is_train=False, flip_test=True)
    assert im2.shape == (1, 2, 2, 3, 3) and k2.shape == (1, 2, 17, 2)
    assert torch.equal(im2[:, 1], torch.flip(im2[:, 0], [2])) and c2[0, 1, 4].tolist() == [181.0, 20.0]
    p = torch.randn(3, 1, 17, 3)
    pf = p.clone(); pf[..., 0] *= -1
    pf[:, :, oracle.JOINTS_LEFT + oracle.JOINTS_RIGHT] = pf[:, :, oracle.JOINTS_RIGHT + oracle.JOINTS_LEFT]
    assert torch.allclose(oracle.fliptest_fuse(p, pf), p, atol=0)


@pytest.mark.skipif(not __import__("os").path.isdir("/root/reference/ContextPose/mvn"),
                    reason="the reference only exists in the build container")
def test_golden_recipe_regenerates_committed_fixtures():
    """Guards the pin itself: oracle/make_goldens.py --check re-imports the REAL reference (asserting that
    `mvn.models.conpose` resolves under /root/reference, not to this repo's mirror), regenerates every fixture
    in memory and compares all keys with the committed .npz files."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    r = subprocess.run([sys.executable, os.path.join(root, "oracle", "make_goldens.py"), "--check"], cwd="/tmp", env=env,
                       capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.count(": OK") >= len(CASES) + 4


def test_oracle_droppath_training_step_matches_reference():
    """Training mode with DropPath ON: the multipliers the reference drew (recorded by make_goldens.py in the C ABI's
    drop_masks layout) injected into the oracle's keep= path reproduce the reference's prediction, loss and gradients
    (pose_dformer.py:71,76-79,101,137-138)."""
    from capf import synth
    name = "w32_256x256_b2"
    case, g = CASES[name], load_golden(name)
    _, sd = make_model(case["backbone"], wseed=case["wseed"], bn=case["bn"])
    img, k2d, kc = case_inputs(case)
    _, _, _, gt = synth.synth_inputs(case["B"], case["H"], case["W"], seed=case["iseed"], crop_range=case["crop"], with_gt=True)
    keys = [k[len("dp_grad:"):] for k in g.files if k.startswith("dp_grad:")]
    P = {k: (v.clone().requires_grad_(True) if k in keys else v) for k, v in sd.items()}
    masks = torch.from_numpy(g["dp_masks"])
    assert masks.numel() == 2 * 4 * (2 + 2 * 17 + 2) and (masks == 0).any()
    pred = oracle.ca_pf_forward(P, img, k2d, kc, backbone=case["backbone"], drop_masks=masks)
    loss = oracle.mpjpe(pred, gt)
    loss.backward()
    np.testing.assert_allclose(pred.detach().numpy(), g["dp_out"], atol=TOL)
    assert abs(loss.item() - float(g["dp_train_loss"])) < 1e-6
    assert abs(float(g["dp_train_loss"]) - float(g["train_loss"])) > 1e-3        # the drop really changed the step
    for k in keys:
        want = g["dp_grad:" + k]
        assert np.abs(P[k].grad.numpy() - want).max() <= 1e-5 * max(1e-6, np.abs(want).max()) + 1e-9, k


def test_bf16_emulation_rounds_where_the_engine_stores_bf16_and_nowhere_else():
    """oracle.ca_pf_forward(..., emulate_bf16=True): (a) every context map holds bf16-representable values; (b) the result
    moves away from the fp32 path by a bf16-sized amount (1e-4 .. 3e-2 m), not by fp32 roundoff and not by a blunder;
    (c) the fp32 path is untouched by the refactor (the golden tests above pin it to the reference at 0.0)."""
    import torch
    import capf_oracle as oracle
    from conftest import make_model
    from capf import synth
    for backbone, H, W in (("hrnet_32", 128, 96), ("cpn", 128, 96)):
        model, sd = make_model(backbone, wseed=61)
        img, k2d, kc = synth.synth_inputs(2, H, W, seed=62, crop_range=(W, H))
        te, tf = {}, {}
        with torch.no_grad():
            e = oracle.ca_pf_forward(sd, img, k2d, kc.clone(), backbone=backbone, taps=te, emulate_bf16=True)
            f = oracle.ca_pf_forward(sd, img, k2d, kc.clone(), backbone=backbone, taps=tf)
        for l in range(4):
            m = te["features"][l]
            assert torch.equal(m, oracle.bf16_round(m))
            assert not torch.equal(tf["features"][l], oracle.bf16_round(tf["features"][l]))
            rel = ((m - tf["features"][l]).norm() / tf["features"][l].norm()).item()
            assert 1e-4 < rel < 3e-2, (backbone, l, rel)
        d = (e - f).abs().max().item()
        assert 1e-5 < d < 3e-2, (backbone, d)
        if backbone == "cpn":
            # PLACEMENT of the roundings in globalNet's top-down path = the engine's (csrc/plan.cpp build_cpn: the `upsamples` 1x1 conv
            # runs on the low-resolution map and is stored in bf16, the lateral conv's epilogue adds its interpolation to the UNROUNDED
            # lateral and rounds once -- round 6; until round 5 a resize-add launch read a bf16 lateral): the low-resolution conv output is
            # bf16, has the PREVIOUS level's resolution, the lateral is NOT bf16, and each level is exactly round(interp(low) + lateral)
            import torch.nn.functional as F
            fms, lows, lats = te["cpn_fms"], te["cpn_up_low"], te["cpn_lateral"]
            assert len(lows) == 3 and len(fms) == 4
            for i in range(1, 4):
                low, lat = lows[i - 1], lats[i - 1]
                assert low.shape[-2:] == fms[i - 1].shape[-2:] and torch.equal(low, oracle.bf16_round(low))
                assert not torch.equal(lat + 0.0, lat * 0.0) and not torch.equal(lat, oracle.bf16_round(lat))
                want = oracle.bf16_round(F.interpolate(low, scale_factor=2, mode="bilinear", align_corners=True) + lat)
                assert torch.equal(fms[i], want)
            assert "cpn_up_low" not in tf                       # the fp32 path keeps the reference's order (goldens pin it)


def test_prefetch_restatement_equals_the_reference_prefetcher_golden():
    """N1 pinned by a RUN OF THE REFERENCE: tests/golden/prefetch.npz holds what the reference's own data_prefetcher.preload
    (datasets/utils.py:33-82, executed on CPU with its CUDA-stream plumbing stubbed: oracle/_refshim.run_reference_prefetcher)
    returned in six modes.  oracle.prefetch_preprocess(scalar_div="cpu") must equal it BIT FOR BIT; the "cuda" mode — the one
    capf_preprocess is held to on the GPU box — may differ only in the images and only by the reciprocal-multiply rounding of
    `x / 255.0` (ATen's CUDA scalar-divisor path), i.e. by at most one ulp of the quotient propagated through (.-mean)/std."""
    from golden_cases import PREFETCH_MODES, prefetch_inputs
    g = load_golden("prefetch")
    for name, (backbone, is_train, flip_test, flip) in PREFETCH_MODES.items():
        img, gt, k2d, kc = prefetch_inputs()
        got = oracle.prefetch_preprocess(img, gt, k2d, kc, backbone, is_train=is_train, flip=flip, flip_test=flip_test, scalar_div="cpu")
        for key, t in zip(("images", "gt", "k2d", "kcrop"), got):
            np.testing.assert_array_equal(t.numpy(), g[f"{name}:{key}"], err_msg=f"{name}:{key}")
        cuda = oracle.prefetch_preprocess(img, gt, k2d, kc, backbone, is_train=is_train, flip=flip, flip_test=flip_test)
        for key, t in zip(("gt", "k2d", "kcrop"), cuda[1:]):
            np.testing.assert_array_equal(t.numpy(), g[f"{name}:{key}"])
        d = np.abs(cuda[0].numpy() - g[f"{name}:images"])
        # one ulp of a quotient in [0, 1] is 6e-8; / std (>= 0.224) scales it by <= 4.5; + the roundings of values up to 2.7 (ulp 2.4e-7)
        assert d.max() <= 1e-6, (name, d.max())
        assert d.max() > 0 or backbone == "cpn"            # the two modes are not vacuously identical


def test_grid_sample_in_cells_is_grid_sample_with_the_cells_given():
    """The differentiable sampler of the gradient tests (capf_oracle.grid_sample_in_cells): with ATen's own cells (floor of the
    clipped pixel coordinate, bilinear_corners) it reproduces F.grid_sample(padding_mode='border', align_corners=True) and
    both of its gradients; with a neighbouring cell forced at a boundary it is the continuous extension of that branch."""
    import torch.nn.functional as F
    torch.manual_seed(0)
    f = torch.randn(2, 5, 9, 7, dtype=torch.float64, requires_grad=True)
    g = (torch.rand(2, 3, 4, 2, dtype=torch.float64) * 2.4 - 1.2).requires_grad_(True)          # some samples clipped at the border
    c = oracle.bilinear_corners(g.detach().numpy(), 9, 7, "border")
    ix0, iy0 = torch.from_numpy(c["ix0"].astype(np.int64)), torch.from_numpy(c["iy0"].astype(np.int64))
    a = F.grid_sample(f, g, mode="bilinear", padding_mode="border", align_corners=True)
    b = oracle.grid_sample_in_cells(f, g, ix0, iy0)
    assert (a - b).abs().max().item() < 1e-14
    ga = torch.autograd.grad(a.square().sum(), [f, g])
    gb = torch.autograd.grad(b.square().sum(), [f, g])
    assert (ga[0] - gb[0]).abs().max().item() < 1e-12 and (ga[1] - gb[1]).abs().max().item() < 1e-12
    # a sample exactly ON a vertical cell boundary (x = 3 of 0..6): the left and the right cell give the same value ...
    gx = torch.tensor([[[[2 * 3 / 6 - 1, 0.1]]]], dtype=torch.float64).expand(2, 1, 1, 2).clone().requires_grad_(True)
    cy = oracle.bilinear_corners(gx.detach().numpy(), 9, 7, "border")["iy0"].astype(np.int64)
    left = oracle.grid_sample_in_cells(f, gx, torch.full((2, 1, 1), 2), torch.from_numpy(cy))
    right = oracle.grid_sample_in_cells(f, gx, torch.full((2, 1, 1), 3), torch.from_numpy(cy))
    assert (left - right).abs().max().item() < 1e-14
    # ... and different one-sided derivatives w.r.t. x: what two evaluations a roundoff apart may disagree on
    dl = torch.autograd.grad(left.sum(), gx, retain_graph=True)[0][..., 0]
    dr = torch.autograd.grad(right.sum(), gx)[0][..., 0]
    assert (dl - dr).abs().max().item() > 1e-3


def test_grid_sample_in_cells_takes_the_clip_side_it_is_given():
    """grid_sample_in_cells(unclipped=...): with every coordinate's own side (0 < x < size - 1) it is the function without the argument,
    value and both gradients; a coordinate a roundoff INSIDE the last pixel that the implementation under test clipped (its fp32
    position is the border itself: found on a 4 x 3 map, test_gpu_train_widths.py) passes no gradient and moves the value by that
    roundoff; one a roundoff OUTSIDE that it left unclipped keeps the gradient of the last cell."""
    torch.manual_seed(1)
    f = torch.randn(2, 5, 4, 3, dtype=torch.float64, requires_grad=True)
    g = (torch.rand(2, 3, 4, 2, dtype=torch.float64) * 2.4 - 1.2).requires_grad_(True)
    c = oracle.bilinear_corners(g.detach().numpy(), 4, 3, "border")
    ix0, iy0 = torch.from_numpy(c["ix0"].astype(np.int64)), torch.from_numpy(c["iy0"].astype(np.int64))
    u = (g.detach() + 1) / 2 * torch.tensor([2.0, 3.0], dtype=torch.float64)
    own = (u > 0) & (u < torch.tensor([2.0, 3.0], dtype=torch.float64))
    assert own.any() and not own.all()
    a, b = oracle.grid_sample_in_cells(f, g, ix0, iy0), oracle.grid_sample_in_cells(f, g, ix0, iy0, own)
    assert torch.equal(a, b)
    ga, gb = torch.autograd.grad(a.square().sum(), [f, g]), torch.autograd.grad(b.square().sum(), [f, g])
    assert torch.equal(ga[0], gb[0]) and torch.equal(ga[1], gb[1])
    # y = 3 - 2.6e-7 of 0..3 (what float64 made of an fp32 position that is 3.0 itself), in the last cell (NW corner y0 = 2)
    eps = 2.6e-7
    for dy, free in ((-eps, False), (+eps, True)):
        gy = torch.tensor([[[[0.2, 2 * (3 + dy) / 3 - 1]]]], dtype=torch.float64).expand(2, 1, 1, 2).clone().requires_grad_(True)
        cells = (torch.full((2, 1, 1), 1), torch.full((2, 1, 1), 2))
        mine = oracle.grid_sample_in_cells(f, gy, *cells)
        told = oracle.grid_sample_in_cells(f, gy, *cells, torch.tensor([True, free]).expand(2, 1, 1, 2))
        assert (mine - told).abs().max().item() < 4 * eps * f.abs().max().item()
        d_mine = torch.autograd.grad(mine.sum(), gy, retain_graph=True)[0]
        d_told = torch.autograd.grad(told.sum(), gy)[0]
        assert (d_mine[..., 0] - d_told[..., 0]).abs().max().item() < 5 * 4 * eps * f.abs().max().item()      # (x is nowhere near a border; 5 channels)
        assert (d_mine[..., 1] != 0).all() == (not free) and (d_told[..., 1] != 0).all() == free
        assert (d_mine[..., 1] == 0).all() == free and (d_told[..., 1] == 0).all() == (not free)


@pytest.mark.parametrize("name", ["w48_256x256_b1", "cpn_384x288_b1"])
def test_bf16_emulation_sits_between_the_references_two_bf16_evaluations(name):
    """The bf16-emulating oracle (the yardstick of the end-to-end bf16 GPU tests, bf16_report.py) against what the REAL reference does
    in bf16 on the same golden frame (tests/golden/bf16_reference.npz: torch.autocast(bfloat16), and fp32 activations with bf16-rounded
    conv / linear operands): the emulation's distance to the reference's fp32 joints must not exceed the autocast run's, nor be
    implausibly small next to the operand-rounding run's -- i.e. the builder's emulation is a bf16 evaluation of the reference's
    arithmetic as the reference itself would produce one, not a private notion of bf16."""
    from bf16_report import reference_bf16_distances
    case = CASES[name]
    g = load_golden(name)
    _, sd = make_model(case["backbone"], wseed=case["wseed"], bn=case["bn"])
    img, k2d, kc = case_inputs(case)
    torch.set_num_threads(8)
    with torch.no_grad():
        emu = oracle.ca_pf_forward(sd, img, k2d, kc.clone(), backbone=case["backbone"], emulate_bf16=True).numpy()
    d = emu - g["out"]
    mean, worst = float(np.linalg.norm(d, axis=-1).mean()), float(np.abs(d).max())
    ref = reference_bf16_distances(name)
    print(f"{name}: emulation {mean:.3e} m mean / {worst:.3e} max from the reference's fp32 joints;  reference under autocast "
          f"{ref['ac']['joints_mean_dist']:.3e} / {ref['ac']['joints_maxabs']:.3e};  with bf16 operands only {ref['opr']['joints_mean_dist']:.3e} / {ref['opr']['joints_maxabs']:.3e}")
    assert mean <= 1.25 * ref["ac"]["joints_mean_dist"] and worst <= 1.25 * ref["ac"]["joints_maxabs"]
    assert mean >= 0.4 * ref["opr"]["joints_mean_dist"]
    # the reference's two bf16 joint sets are data of this test too: they differ from the fp32 golden by what the fixture says
    for tag in ("ac", "opr"):
        dd = ref[tag]["out"] - g["out"]
        assert abs(float(np.abs(dd).max()) - ref[tag]["joints_maxabs"]) <= 1e-7


def test_fp32_residual_stream_under_bf16_is_the_operands_only_evaluation():
    """The A/B VERDICT r4 and r5 asked for instead of an argument: HRNet-48 with EVERY backbone activation kept fp32 in memory and rounded to
    bf16 only as an MFMA operand (oracle emulate_bf16="stream_fp32"; SURVEY section 7's prescription) against the engine's placement (bf16
    activations in memory, emulate_bf16=True), six frames, distance of the joints to the fp32 evaluation.  Numbers of this run are in
    EXPERIMENTS.md R6.3 next to the bytes the fp32 stream would cost; asserted here: the fp32 stream is closer to fp32 (it removes one
    rounding per stored activation), and on the golden frame it lands on the REFERENCE's own operands-only evaluation."""
    from bf16_report import reference_bf16_distances
    from capf import synth
    case = CASES["w48_256x256_b1"]
    _, sd = make_model(case["backbone"], wseed=case["wseed"], bn=case["bn"])
    img, k2d, kc = synth.synth_inputs(6, 256, 256, seed=case["iseed"], crop_range=(256, 256))
    torch.set_num_threads(8)
    with torch.no_grad():
        ref = oracle.ca_pf_forward(sd, img, k2d, kc.clone(), backbone="hrnet_48").numpy()
        eng = oracle.ca_pf_forward(sd, img, k2d, kc.clone(), backbone="hrnet_48", emulate_bf16=True).numpy()
        stm = oracle.ca_pf_forward(sd, img, k2d, kc.clone(), backbone="hrnet_48", emulate_bf16="stream_fp32").numpy()
    def dist(a):
        d = a - ref
        return float(np.linalg.norm(d, axis=-1).mean()), float(np.abs(d).max())
    (em, ew), (sm, sw) = dist(eng), dist(stm)
    g = reference_bf16_distances("w48_256x256_b1")
    print(f"HRNet-48, 6 frames, joints vs fp32 (mean distance / max abs, m): bf16 activations in memory (the engine) {em:.3e} / {ew:.3e};  "
          f"fp32 residual stream, bf16 operands {sm:.3e} / {sw:.3e};  the reference with bf16 operands only (golden frame) "
          f"{g['opr']['joints_mean_dist']:.3e} / {g['opr']['joints_maxabs']:.3e}")
    assert sm < em
    # frame 0 of this batch is the golden frame (same seed): the fp32-stream emulation must sit within a factor of the reference's operands-only run
    d0 = float(np.linalg.norm(stm[0] - ref[0], axis=-1).mean())
    assert 0.4 * g["opr"]["joints_mean_dist"] <= d0 <= 2.0 * g["opr"]["joints_mean_dist"], d0
