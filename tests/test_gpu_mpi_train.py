"""GPU: training steps of the MPI-INF-3DHP variant (VolumetricTriangulationNet, no context blocks, embed 64 / 96, depth 1..8) against
the fp64 yardstick, the way ContextPose_mpi/run_3dhp.py:60-101 trains it: `out, _ = model(img, k2d, kcrop)`, the permute / view of
:83, mpjpe_cal (common/utils.py:14-16) against a target whose joint 14 is zeroed (:66), backward, AdamW(weight_decay = 0.1) (:277).

The yardstick is oracle.lifter_forward(..., context_blocks=False, depth=d) in float64 on the engine's own context maps (feat{l} taps),
as train_yardstick.lifter64 does for the H36M model, with the bounds of test_gpu_train_matrix.py: prediction within 1e-5, loss within
1e-6 relative, every gradient within 2e-5 relative L2 and 2e-5 of the fp64 gradient's largest entry.  Head dims 8 / 12 (res blocks,
C = 64 / 96 over 8 heads) and 40 / 60 (joint blocks, D = 320 / 480), K = 64 / 96 / 320 / 480 in every product, ragged 64-wide tiles in
the weight gradients (288, 96, 1440, 480), K = 48 (HRNet-48's first map) on the zero-padded pack.

  B = 1, 4     fp32 matrix pipe (the two-piece GEMM starts at batch 5)
  B = 5        the first two-piece step
  B = 13       DropPath 0.2 (fixed multipliers, the variant's layout: res | joint, depth blocks each)
  B = 160      run_3dhp.py's default batch: split-K weight-gradient slabs
  depth 1, 2, 6, 8 (W32), one bf16 case (bf16 maps, fp32 pipe)."""
import contextlib
import copy
import io

import pytest
import torch

import capf_oracle as oracle
from capf import synth
from train_yardstick import GRAD_L2_BOUND, GRAD_MAX_BOUND

pytestmark = pytest.mark.gpu


def _model(backbone, depth, dtype="fp32", wseed=0, drop=0.0):
    from model.conpose import VolumetricTriangulationNet, mpi_preset
    from mvn.utils.cfg import config
    cfg = mpi_preset(copy.deepcopy(config), backbone)
    cfg.model.poseformer.depth = depth
    with contextlib.redirect_stdout(io.StringIO()):
        m = VolumetricTriangulationNet(cfg, compute_dtype=dtype)
    synth.load_synthetic(m, seed=wseed, bn_mode="random")
    m = m.cuda()
    m.train(); m.backbone.eval(); m.volume_net.train()
    m.drop_path_rate = drop
    return m


def _target(gt):
    t = gt.clone()
    t[:, :, 14] = 0                                   # run_3dhp.py:66 (out_target[:, :, 14] = 0)
    return t


def _step(model, img, k2d, kc, gt):
    """run_3dhp.py:79-101 for one batch: forward, permute / view, mpjpe_cal, backward."""
    kc_dev = kc.clone().cuda()
    N = img.shape[0]
    out, aux = model(img.cuda(), k2d.cuda(), kc_dev)
    assert aux is None and tuple(out.shape) == (N, 3, 1, 17, 1)
    out = out.permute(0, 2, 3, 4, 1).contiguous().view(N, -1, 17, 3)
    target = _target(gt).cuda()
    loss = torch.mean(torch.norm(out - target, dim=len(target.shape) - 1))
    loss.backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), loss.item(), kc_dev.cpu()


def _oracle_masks(masks, B, depth):
    """The variant's DropPath buffer (res | joint, `depth` blocks) in the oracle's layout (ctx | res | joint, 4 blocks each, ones where
    the variant has no block): split_drop_masks then hands block i the engine's multipliers."""
    J = 17
    res = masks[:2 * depth * B * J]
    joint = masks[2 * depth * B * J:]
    assert joint.numel() == 2 * depth * B and depth <= 4
    pad = lambda t, per: torch.cat([t, torch.ones(2 * (4 - depth) * per, dtype=t.dtype)])
    return torch.cat([torch.ones(2 * 4 * B, dtype=masks.dtype), pad(res, B * J), pad(joint, B)])


def _yardstick(model, eng, B, depth, k2d, ref, gt, masks=None):
    feats = [eng.tensor(f"feat{l}")[:B].cpu().double().permute(0, 3, 1, 2).contiguous() for l in range(4)]
    Q = {"volume_net." + n: p.detach().cpu().double().clone().requires_grad_(True) for n, p in model.volume_net.named_parameters()}
    dm = _oracle_masks(masks.cpu().double(), B, depth) if masks is not None else None
    w = oracle.lifter_forward(Q, k2d.cpu().double(), ref.cpu().double(), feats, context_blocks=False, depth=depth, drop_masks=dm)
    loss = oracle.mpjpe(w, _target(gt).cpu().double())
    loss.backward()
    return {k: q.grad for k, q in Q.items()}, w.detach(), loss.item()


def _gradients(model, eng):
    named = list(model.volume_net.named_parameters())
    if all(p.grad is not None for _, p in named):
        return {"volume_net." + n: p.grad.detach().cpu().clone() for n, p in named}
    layout, _ = eng.grad_layout_cached()
    flat = model.last_flat_grad.detach().cpu()
    return {"volume_net." + n: flat[layout["volume_net." + n][0]:][:p.numel()].view(p.shape).clone() for n, p in named}


def _check(tag, model, eng, B, depth, k2d, ref, gt, pred, loss, masks=None):
    g64, w64, l64 = _yardstick(model, eng, B, depth, k2d, ref, gt, masks)
    perr = (pred.double() - w64).abs().max().item()
    lerr = abs(loss - l64) / abs(l64)
    print(f"  {tag}: prediction max|hip - fp64| {perr:.2e}, loss {loss:.6f} (relative error {lerr:.2e})")
    assert torch.isfinite(pred).all()
    assert perr <= 1e-5 and lerr <= 1e-6, (perr, lerr)
    got = _gradients(model, eng)
    n_params = 3 + 4 * 2 + 2 * depth * 12 + 4                 # pos, coord_embed, feat_embed x 4, 12 tensors per block, head
    assert set(got) == set(g64) and len(got) == n_params, (len(got), n_params)
    rows = []
    for k, t in g64.items():
        g = got[k]
        assert torch.isfinite(g).all(), k
        d = g.double() - t
        rows.append(((d.norm() / t.norm().clamp_min(1e-30)).item(), (d.abs().max() / t.abs().max().clamp_min(1e-30)).item(), k))
    rows.sort(reverse=True)
    for l2, mx, k in rows[:3]:
        print(f"    {k:52s} {l2:9.2e} | {mx:9.2e}")
    for l2, mx, k in rows:
        assert l2 <= GRAD_L2_BOUND and mx <= GRAD_MAX_BOUND, (k, l2, mx)
    return w64


CASES = [
    # backbone, depth, dtype, B, DropPath rate
    ("hrnet_32", 4, "fp32", 1, 0.0),
    ("hrnet_32", 4, "fp32", 4, 0.0),
    ("hrnet_32", 4, "fp32", 5, 0.0),
    ("hrnet_32", 4, "fp32", 13, 0.2),
    ("hrnet_32", 4, "fp32", 160, 0.0),
    ("hrnet_48", 4, "fp32", 4, 0.0),
    ("hrnet_48", 4, "fp32", 5, 0.2),
    ("hrnet_48", 4, "fp32", 160, 0.0),
    ("hrnet_32", 1, "fp32", 5, 0.0),
    ("hrnet_32", 2, "fp32", 13, 0.2),
    ("hrnet_32", 6, "fp32", 4, 0.0),
    ("hrnet_32", 8, "fp32", 13, 0.0),
    ("hrnet_32", 4, "bf16", 9, 0.0),
]


@pytest.mark.parametrize("backbone,depth,dtype,B,drop", CASES,
                         ids=[f"{b}-d{d}-{t}-B{n}" + ("-droppath" if p else "") for b, d, t, n, p in CASES])
def test_mpi_training_step_vs_fp64_yardstick(backbone, depth, dtype, B, drop):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    model = _model(backbone, depth, dtype, wseed=80 + B + depth, drop=drop)
    img, k2d, kc, gt = synth.synth_inputs(B, 256, 192, seed=81 + B + depth, crop_range=(192, 256), with_gt=True)
    masks = None
    if drop:
        torch.manual_seed(9)
        masks = model._drop_masks(B, torch.device("cuda"))
        assert masks.numel() == 2 * depth * (B * 17 + B) and (masks == 0).any()
        model._drop_masks = lambda b, dev: masks               # the step below uses exactly these multipliers
    eng = model.engine_for(img.cuda())
    pred, loss, ref = _step(model, img, k2d, kc, gt)
    tag = f"{backbone} depth {depth} {dtype} B={B} DropPath {drop}"
    _check(tag, model, eng, B, depth, k2d, ref, gt, pred, loss, masks)


def test_fused_adamw_on_the_flattened_variant_matches_torch_adamw():
    """Three steps at HRNet-32 depth 4, B = 7: capf.optim.flatten_ + FusedAdamW (weight decay 0.1) on the flat gradient vs
    torch.optim.AdamW with run_3dhp.py:261-277's two parameter groups (the sampling_offsets group is empty here: no
    DeformableBlock) fed the same gradients.  Parameters after every step agree to fp32 rounding; the third step is held to the
    fp64 yardstick at the parameters' CURRENT values, and the updates must have moved the prediction beyond that bound."""
    from capf.optim import FusedAdamW, flatten_
    torch.set_num_threads(min(16, torch.get_num_threads()))
    B = 7
    model = _model("hrnet_32", 4, wseed=90)
    start = {n: p.detach().clone() for n, p in model.volume_net.named_parameters()}
    shadow = {n: torch.nn.Parameter(p.detach().clone()) for n, p in model.volume_net.named_parameters()}
    groups = [{"params": [p for n, p in shadow.items() if "sampling_offsets" not in n], "lr": 6.4e-4},
              {"params": [p for n, p in shadow.items() if "sampling_offsets" in n], "lr": 6.4e-5}]
    assert not groups[1]["params"]
    ref_opt = torch.optim.AdamW(groups, weight_decay=0.1)
    flat_p = flatten_(model.volume_net)
    opt = FusedAdamW(flat_p, lr=6.4e-4, weight_decay=0.1)
    model.flat_grad_only = True
    layout = None
    for t in range(3):
        img, k2d, kc, gt = synth.synth_inputs(B, 256, 192, seed=91 + t, crop_range=(192, 256), with_gt=True)
        eng = model.engine_for(img.cuda())
        pred, loss, ref = _step(model, img, k2d, kc, gt)
        if t == 2:
            break
        layout, _ = eng.grad_layout_cached()
        flat_g = model.last_flat_grad
        for n, p in shadow.items():
            off, cnt = layout["volume_net." + n]
            p.grad = flat_g[off:off + cnt].view(p.shape).clone()
        ref_opt.step()
        opt.step(flat_g)
        model.lifter_params_changed()
        torch.cuda.synchronize()
        worst = 0.0
        for n, p in model.volume_net.named_parameters():
            d = (p.detach() - shadow[n].detach()).abs().max().item()
            worst = max(worst, d / max(1e-30, shadow[n].detach().abs().max().item()))
            assert torch.allclose(p.detach(), shadow[n].detach(), rtol=1e-6, atol=1e-7), (t, n, d)
        print(f"  step {t + 1}: FusedAdamW vs torch AdamW, worst parameter difference {worst:.2e} of the tensor's max")
    w64 = _check("hrnet_32 depth 4 fp32 B=7, step 3 after two FusedAdamW updates", model, eng, B, 4, k2d, ref, gt, pred, loss)
    feats = [eng.tensor(f"feat{l}")[:B].cpu().double().permute(0, 3, 1, 2).contiguous() for l in range(4)]
    Q = {"volume_net." + n: v.cpu().double() for n, v in start.items()}
    with torch.no_grad():
        w_start = oracle.lifter_forward(Q, k2d.double(), ref.double(), feats, context_blocks=False, depth=4)
    moved = (w64 - w_start).abs().max().item()
    print(f"  the two updates moved the prediction by {moved:.2e}")
    assert moved >= 1e-4
