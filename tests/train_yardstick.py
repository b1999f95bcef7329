"""The fp64 yardstick of the training step's gradients (shared by test_gpu_fullsize.py and test_gpu_train_matrix.py).

A training step's gradients are compared with the same lifter evaluated in float64 (capf_oracle.lifter_forward, MPJPE, autograd).
Two things would make a naive comparison meaningless (derivation: test_gpu_fullsize.py's batch-512 test):
  (a) a sampling-offset gradient is the small remainder of tens of thousands of cancelling rows -- the bound is relative to the fp64
      gradient, not to an fp32 evaluation;
  (b) grid_sample's derivative w.r.t. the position is one-sided at cell boundaries -- the yardstick evaluates its deformable samplers IN
      THE CELLS THE ENGINE USED (its cidx taps, themselves checked bit for bit against ATen's index rule: check_cells_against_index_rule).
  (c) the border clip is one-sided in the same way: a coordinate clipped to 0 or size - 1 passes no gradient (ATen's
      clip_coordinates_set_grad), one a roundoff inside does -- the yardstick clips the coordinates THE ENGINE'S POSITIONS clip under
      ATen's rule in fp32 (engine_clip_sides: from the cpos taps, not from any flag of the kernels).  On maps as small as 4 x 3, where
      most samples sit on a border, a step in a few hundred has such a coordinate; without this its one sample's derivative shows as an error
      of 2e-4 in that block's sampling_offsets and norm1 gradients (found at embed_dim_ratio 160, B = 6: test_gpu_train_widths.py).
engine_yardstick() also takes the engine's own context maps (feat{l} taps, upcast to float64; bf16 maps upcast exactly), so the bound
measures the lifter alone, whatever the backbone and its dtype."""
import numpy as np
import torch

import capf_oracle as oracle

# every one of the 191 gradients: relative L2 and max-entry error (of the fp64 gradient's max); measured at HRNet-32 B = 512:
# 1.4e-6 / 3.1e-6
GRAD_L2_BOUND = 2e-5
GRAD_MAX_BOUND = 2e-5
N_LIFTER_GRADS = 191


def _joints(eng):
    """the engine's joint count (capf_config.num_joints: the tap views below are [B, J, 4, 16, 2])"""
    return int(eng.cfg.num_joints)


def check_cells_against_index_rule(eng, B, tag):
    """At a PRODUCTION batch: the NW corners the deformable sampler gathered from (cidx{i}) == oracle.bilinear_corners(the positions the
    kernel itself computed (cpos{i}), 'border') bit for bit, for all 4 blocks x 4 levels x B x J x 16 samples; prints how many samples
    sit within 4 ulp of a cell boundary (where grid_sample's one-sided derivative makes the choice of cell matter)."""
    n, near, J = 0, 0, _joints(eng)
    for i in range(4):
        pos = eng.tensor(f"cpos{i}")[:B].cpu().view(B, J, 4, 16, 2).numpy()
        idx = eng.tensor(f"cidx{i}")[:B].cpu().view(B, J, 4, 16, 2).numpy()
        for l in range(4):
            f = eng.tensor(f"feat{l}")
            H, W = f.shape[1], f.shape[2]
            want = oracle.bilinear_corners(pos[:, :, l], H, W, "border")
            np.testing.assert_array_equal(idx[:, :, l, :, 0], want["ix0"])
            np.testing.assert_array_equal(idx[:, :, l, :, 1], want["iy0"])
            for g, size in ((pos[:, :, l, :, 0], W), (pos[:, :, l, :, 1], H)):
                x = np.clip(((g + np.float32(1)) / np.float32(2)) * np.float32(size - 1), 0, size - 1).astype(np.float32)
                inside = (x > 0) & (x < size - 1)                 # (a coordinate the border clip pinned to 0 / size - 1 has no choice of cell)
                near += int((inside & (np.abs(x - np.rint(x)) <= 4 * np.spacing(np.maximum(np.abs(x), np.float32(1))))).sum())
            n += want["ix0"].size
    print(f"  {tag}: {n} deformable samples, corner indices == ATen's rule on the kernel's own positions bit for bit; "
          f"{near} unclipped coordinates within 4 ulp of a cell boundary")
    assert n == 4 * 4 * B * J * 16
    return near


# parameters whose gradient contains NO derivative of a sample w.r.t. its position (everything behind the last deformable sampler, and
# the last context block's value / weight path): grid_sample's one-sided position derivative cannot touch them, so they are compared
# against the oracle with its OWN floor() cells
def independent_of_cells(k):
    return (k.startswith(("volume_net.res_blocks.", "volume_net.joint_blocks.", "volume_net.head.")) or
            k.startswith(("volume_net.context_blocks.3.embed_proj.", "volume_net.context_blocks.3.attention_weights.",
                          "volume_net.context_blocks.3.mlp.", "volume_net.context_blocks.3.norm2.")))


def engine_cells(eng, B):
    """The bilinear cells the engine's deformable samplers used (cidx{i} taps of a set_debug(True) step): int64 [B, J, 4, 16, 2] per block."""
    return [eng.tensor(f"cidx{i}")[:B].cpu().view(B, _joints(eng), 4, 16, 2).long() for i in range(4)]


def engine_clip_sides(eng, B):
    """Which coordinates of the deformable samplers the border clip left alone, by ATen's rule (0 < x < size - 1 on the unnormalised
    coordinate) in the kernels' fp32 arithmetic on the positions the engine computed (cpos{i} taps of a set_debug(True) step): bool
    [B, J, 4, 16, 2] per block."""
    out = []
    for i in range(4):
        pos = eng.tensor(f"cpos{i}")[:B].cpu().view(B, _joints(eng), 4, 16, 2).numpy()
        free = np.zeros(pos.shape, dtype=bool)
        for l in range(4):
            f = eng.tensor(f"feat{l}")
            for axis, size in ((0, f.shape[2]), (1, f.shape[1])):
                x = ((pos[:, :, l, :, axis] + np.float32(1)) / np.float32(2)) * np.float32(size - 1)
                assert x.dtype == np.float32
                free[:, :, l, :, axis] = (x > 0) & (x < size - 1)
        out.append(torch.from_numpy(free))
    return out


def lifter64(params, k2d, ref, gt, feats, cells=None, drop_masks=None, sides=None, heads=8):
    """oracle.lifter_forward in float64 on `feats` (NCHW), MPJPE against gt, backward.  params: name -> tensor (the volume_net.* entries
    are used).  cells / sides: engine_cells / engine_clip_sides; heads: the Blocks' head count.  Returns ({name: fp64 gradient}, fp64 prediction, fp64 loss)."""
    Q = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in params.items() if k.startswith("volume_net.")}
    w = oracle.lifter_forward(Q, k2d.cpu().double(), ref.cpu().double(), feats, cells=cells, unclipped=sides,
                              drop_masks=drop_masks.cpu().double() if drop_masks is not None else None, heads=heads)
    loss = oracle.mpjpe(w, gt.cpu().double())
    loss.backward()
    return {k: q.grad for k, q in Q.items()}, w.detach(), loss.item()


def engine_yardstick(model, eng, B, k2d, ref, gt, drop_masks=None):
    """The fp64 yardstick of a step the engine has just taken with set_debug(True): the lifter at the model's CURRENT volume_net values,
    on the engine's own context maps and in the engine's own cells.  ref: the normalised crop keypoints the step used (the forward's
    third argument after it returned).  Returns ({'volume_net.<name>': fp64 gradient}, fp64 prediction, fp64 loss)."""
    feats = [eng.tensor(f"feat{l}")[:B].cpu().double().permute(0, 3, 1, 2).contiguous() for l in range(4)]
    params = {"volume_net." + n: p for n, p in model.volume_net.named_parameters()}
    return lifter64(params, k2d, ref, gt, feats, engine_cells(eng, B), drop_masks, engine_clip_sides(eng, B), heads=int(eng.cfg.num_heads))


def engine_gradients(model, eng):
    """The 191 gradients of the last backward, keyed 'volume_net.<name>': the .grad views, or the flat buffer under flat_grad_only."""
    named = list(model.volume_net.named_parameters())
    if all(p.grad is not None for _, p in named):
        return {"volume_net." + n: p.grad.detach().cpu().clone() for n, p in named}
    layout, _ = eng.grad_layout_cached()
    flat = model.last_flat_grad.detach().cpu()
    out = {}
    for n, p in named:
        off, cnt = layout["volume_net." + n] if ("volume_net." + n) in layout else layout[n]
        out["volume_net." + n] = flat[off:off + cnt].view(p.shape).clone()
    return out


def check_gradients(tag, got, want):
    """Every one of the 191 gradients within GRAD_L2_BOUND relative L2 and GRAD_MAX_BOUND of the fp64 gradient's largest entry; prints the
    worst five and returns the worst (relative L2, max entry) pair."""
    assert len(got) == N_LIFTER_GRADS and set(got) == set(want), (len(got), sorted(set(want) ^ set(got))[:5])
    rows = []
    for k, t in want.items():
        g = got[k]
        assert torch.isfinite(g).all(), k
        nrm, scale = t.norm().clamp_min(1e-30), t.abs().max().clamp_min(1e-30)
        d = g.double() - t
        rows.append(((d.norm() / nrm).item(), (d.abs().max() / scale).item(), k))
    rows.sort(reverse=True)
    print(f"  {tag}: {len(rows)} gradients vs the fp64 yardstick; worst five (relative L2 | max entry / max):")
    for l2, mx, k in rows[:5]:
        print(f"    {k:58s} {l2:9.2e} | {mx:9.2e}")
    for l2, mx, k in rows:
        assert l2 <= GRAD_L2_BOUND and mx <= GRAD_MAX_BOUND, (k, l2, mx)
    return rows[0][0], max(r[1] for r in rows)
