"""GPU: training steps across backbones, dtypes and batch regimes against the fp64 yardstick (train_yardstick.py).

Each step runs forward + MPJPE + backward through CA_PF in train mode (backbone eval) with debug taps on, and is held to the lifter
evaluated in float64 on the engine's own context maps and in its own bilinear cells: deformable corners bit for bit against the index
rule, prediction within 1e-5, loss within 1e-6 relative, and all 191 gradients within the batch-512 test's bounds (2e-5 relative L2
and 2e-5 of the fp64 gradient's max per entry).  Because the maps are the engine's, one fp32-sized bound holds for every backbone and
dtype.

What each case pins (csrc/train.cpp; rows of the largest products: 85 per frame in the level blocks, 68 in the context blocks):
  W32 fp32 B=1    fp32 pipe (the two-piece GEMM starts at H2G_MIN_BATCH = 5); one 17-row chunk per column reduction
  W32 fp32 B=4    fp32 pipe, rows-split-K forward GEMMs, ragged last 32-row chunks everywhere (68 joint rows)
  W32 fp32 B=5    the first two-piece step; 85 joint rows, 425 level-block rows: ragged chunks, one weight-gradient slice
  W32 fp32 B=13   two-piece, DropPath 0.2 (the host's multipliers injected into the yardstick); 1105 level-block rows: 35 chunks,
                  the first split-K weight-gradient slabs, a ragged last slice
  W32 fp32 B=100  two-piece; 1700 joint rows (3 slices), 8500 level-block rows (16 slices), ragged last slices
  W48 fp32 B=3    fp32 pipe; the first context level has 48 channels: feat_embed.0 / embed_proj.0 with K = 48 (K % 32 != 0)
  W48 fp32 B=37   two-piece; K = 48 on the two-piece pack, split-K slabs
  W48 bf16 B=9    bf16 context maps read by the samplers and deform_bwd (feat_bf16), the fp32 pipe (no two-piece under bf16)
  CPN fp32 B=6    256-channel maps on every level, two-piece, 384 x 288 crop
  CPN bf16 B=5    bf16 256-channel maps, fp32 pipe, 256 x 192 crop

test_steps_after_an_optimizer_update: three steps, the third held to the yardstick at the parameters' CURRENT values -- stale packs of
the training forward (the [attention_weights | sampling_offsets] pack, the two-piece packs) would fail it."""
import pytest
import torch

from capf import synth
from conftest import make_model
from train_yardstick import (check_cells_against_index_rule, check_gradients, engine_cells, engine_gradients, engine_yardstick,
                             lifter64)

pytestmark = pytest.mark.gpu

H2G_MIN_BATCH = 5        # csrc/engine.h: the first batch whose step runs on the two-piece GEMM


def _train_model(backbone, dtype, wseed, drop):
    model, _ = make_model(backbone, device="cuda", wseed=wseed, bn="random", compute_dtype=dtype)
    model.train(); model.backbone.eval(); model.volume_net.train()
    model.drop_path_rate = drop
    return model


def _route(eng, B):
    """What the step ran on: the two-piece GEMM or the fp32 pipe, and whether the largest weight gradients were split into row slices
    (csrc/train.cpp t_linear_bwd: at least 16 chunks of 32 rows per slice)."""
    n_h2 = eng.lib.capf_train_h2_matrices(eng.h)              # (the plan's table: the step packs it from H2G_MIN_BATCH on)
    chunks = (B * 17 * 5 + 31) // 32
    h2 = n_h2 > 0 and B >= H2G_MIN_BATCH
    return n_h2, f"{'two-piece' if h2 else 'fp32 pipe'}, {'slices > 1' if chunks // 16 > 1 else 'one slice'}"


def _step(model, img, k2d, kc, gt):
    from mvn.models.loss import MPJPE
    kc_dev = kc.clone().cuda()
    pred = model(img.cuda(), k2d.cuda(), kc_dev)
    loss = MPJPE()(pred, gt.cuda())
    loss.backward()
    torch.cuda.synchronize()
    return pred.detach().cpu(), loss.item(), kc_dev.cpu()


def _hold_to_yardstick(tag, model, eng, B, k2d, ref, gt, pred, loss, masks=None):
    g64, w64, l64 = engine_yardstick(model, eng, B, k2d, ref, gt, masks)
    perr = (pred.double() - w64).abs().max().item()
    lerr = abs(loss - l64) / abs(l64)
    print(f"  {tag}: prediction max|hip - fp64| {perr:.2e}, loss {loss:.6f} (relative error {lerr:.2e})")
    assert torch.isfinite(pred).all()
    assert perr <= 1e-5 and lerr <= 1e-6, (perr, lerr)
    return check_gradients(tag, engine_gradients(model, eng), g64), w64


CASES = [
    # backbone, dtype, (H, W), B, DropPath rate
    ("hrnet_32", "fp32", (256, 256), 1, 0.0),
    ("hrnet_32", "fp32", (256, 256), 4, 0.0),
    ("hrnet_32", "fp32", (256, 256), 5, 0.0),
    ("hrnet_32", "fp32", (256, 256), 13, 0.2),
    ("hrnet_32", "fp32", (256, 256), 100, 0.0),
    ("hrnet_48", "fp32", (256, 192), 3, 0.0),
    ("hrnet_48", "fp32", (256, 192), 37, 0.0),
    ("hrnet_48", "bf16", (256, 256), 9, 0.0),
    ("cpn", "fp32", (384, 288), 6, 0.0),
    ("cpn", "bf16", (256, 192), 5, 0.0),
]


@pytest.mark.parametrize("backbone,dtype,hw,B,drop", CASES,
                         ids=[f"{b}-{d}-{h}x{w}-B{n}" + ("-droppath" if p else "") for b, d, (h, w), n, p in CASES])
def test_training_step_vs_fp64_yardstick(backbone, dtype, hw, B, drop):
    H, W = hw
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = _train_model(backbone, dtype, 61 + B, drop)
    img, k2d, kc, gt = synth.synth_inputs(B, H, W, seed=62 + B, crop_range=(W, H), with_gt=True)
    masks = None
    if drop:
        torch.manual_seed(7)
        masks = model._drop_masks(B, torch.device("cuda"))
        assert (masks == 0).any() and masks.numel() == 2 * 4 * (B + 17 * B + B)
        model._drop_masks = lambda b, dev: masks                 # the step below uses exactly these multipliers
    eng = model.engine_for(img.cuda())
    eng.set_debug(True)                                        # cidx / cpos taps of the deformable samplers
    pred, loss, ref = _step(model, img, k2d, kc, gt)
    n_h2, route = _route(eng, B)
    assert (n_h2 > 0) == (dtype == "fp32"), n_h2                # (no two-piece table under bf16)
    tag = f"{backbone} {dtype} {H}x{W} B={B} DropPath {drop} [{route}]"
    check_cells_against_index_rule(eng, B, tag)
    (l2, mx), _ = _hold_to_yardstick(tag, model, eng, B, k2d, ref, gt, pred, loss, masks)
    print(f"  {tag}: worst gradient {l2:.2e} relative L2, {mx:.2e} of max")


@pytest.mark.parametrize("how", ["torch_adamw", "fused_adamw_flat"])
def test_steps_after_an_optimizer_update(how):
    """Three consecutive steps at HRNet-32 B = 7 (two-piece GEMM, DropPath off), parameters updated between them:
    torch_adamw: torch.optim.AdamW over model.parameters(), the reference's loop (the host notices the parameters' _version bumps);
    fused_adamw_flat: flatten_ + FusedAdamW on the flat gradient of flat_grad_only + lifter_params_changed(), the way bench.py steps.
    The third step's prediction and 191 gradients are held to the fp64 yardstick at the CURRENT parameter values, and the update must
    have moved the prediction far beyond that bound (else the test could not see a stale pack)."""
    from capf.optim import FusedAdamW, flatten_
    B = 7
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = _train_model("hrnet_32", "fp32", 71, 0.0)
    start = {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if k.startswith("volume_net.")}
    if how == "torch_adamw":
        opt = torch.optim.AdamW(model.parameters(), lr=6.4e-4, weight_decay=0.1)
        update = opt.step
    else:
        flat_p = flatten_(model.volume_net)
        opt = FusedAdamW(flat_p, lr=6.4e-4, weight_decay=0.1)
        model.flat_grad_only = True

        def update():
            opt.step(model.last_flat_grad)
            model.lifter_params_changed()
    for t in range(3):
        img, k2d, kc, gt = synth.synth_inputs(B, 256, 256, seed=72 + t, crop_range=(256, 256), with_gt=True)
        eng = model.engine_for(img.cuda())
        eng.set_debug(True)
        model.zero_grad(set_to_none=True)
        pred, loss, ref = _step(model, img, k2d, kc, gt)
        if t < 2:
            update()
    n_h2, route = _route(eng, B)
    assert n_h2 > 0
    tag = f"hrnet_32 fp32 256x256 B={B}, step 3 after {how} [{route}]"
    check_cells_against_index_rule(eng, B, tag)
    (l2, mx), _ = _hold_to_yardstick(tag, model, eng, B, k2d, ref, gt, pred, loss)
    feats = [eng.tensor(f"feat{l}")[:B].cpu().double().permute(0, 3, 1, 2).contiguous() for l in range(4)]
    _, w_start, _ = lifter64(start, k2d, ref, gt, feats, engine_cells(eng, B))
    moved = (pred.double() - w_start).abs().max().item()
    print(f"  {tag}: worst gradient {l2:.2e} relative L2, {mx:.2e} of max; the two updates moved the prediction by {moved:.2e}")
    assert moved >= 1e-4
