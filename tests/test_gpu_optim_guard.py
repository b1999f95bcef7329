"""GPU: the guarded AdamW step (capf_grad_sumsq + capf_adamw_step_guarded behind capf.optim.FusedAdamW) against
torch.optim.AdamW + torch.nn.utils.clip_grad_norm_ with the same parameter groups, fed the same gradients: the optimizer end of
the reference's loop (ContextPose/train.py:187-206, 398-407; ContextPose_mpi/run_3dhp.py:260-277).  The sizes are the ones at which
these two kernels can go wrong (one element, one float4, a block, a block + 1, a scalar tail, more elements than one pass of the
fixed grid holds), not the workload's -- except one pass at the real lifter size."""
import copy
import math

import numpy as np
import pytest
import torch

from conftest import make_model
from capf import synth

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-6, 1e-7          # what tests/test_gpu_mpi_train.py holds FusedAdamW to against torch.optim.AdamW


def _lifter_elems():
    from capf import Engine
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), "hrnet_32")
    cfg.model.backbone.fix_weights = True
    eng = Engine(_native.make_capf_config(cfg, 256, 192), device=None)
    total = eng.grad_layout()[1]
    eng.close()
    return total


@pytest.fixture(scope="module")
def noise():
    """one read-only randn buffer of the real lifter size; every size below is a prefix of it"""
    g = torch.Generator(device="cuda").manual_seed(1234)
    return torch.randn(max(_lifter_elems(), (1 << 20) + 5), device="cuda", generator=g)


def _measure(opt, grad, grad_scale):
    opt.step(grad, grad_scale=grad_scale)
    return opt.report()


SIZES = [1, 3, 255, 256, 257, 4099, (1 << 20) + 5, "lifter"]


@pytest.mark.parametrize("n", SIZES)
def test_sum_of_squares_and_nonfinite_flag(noise, n):
    from capf.optim import FusedAdamW
    n = _lifter_elems() if n == "lifter" else n
    p = torch.zeros(n, device="cuda")
    opt = FusedAdamW(p, lr=0.0, weight_decay=0.0, skip_nonfinite=True)
    for scale in (1e-20, 1.0, 1e15):
        g = (noise[:n] * scale).contiguous()
        for gs in (1.0, 0.125):
            want = (gs * g).double().square().sum().item()
            r1 = _measure(opt, g, gs)
            r2 = _measure(opt, g, gs)
            rel = abs(r1["grad_sumsq"] - want) / want
            print(f"  n={n} scale={scale:g} grad_scale={gs}: sumsq {r1['grad_sumsq']:.17e} vs fp64 {want:.17e}, relative {rel:.2e} "
                  f"(bound {2 * n * 2.0 ** -53:.2e})")
            assert rel <= 2 * n * 2.0 ** -53                     # any fp64 summation order of n non-negative terms
            assert np.float64(r1["grad_sumsq"]).tobytes() == np.float64(r2["grad_sumsq"]).tobytes()       # two runs: the same bits
            assert not r1["grad_nonfinite"] and r1["grad_norm"] == pytest.approx(math.sqrt(r1["grad_sumsq"]), rel=1e-15)
    taken = opt.report()["steps_taken"]
    assert taken == 12 and opt.report()["steps_skipped"] == 0
    g = noise[:n].clone()
    places = sorted({0, n - 1} | ({n - n % 4} if n % 4 else set()))          # first, last, first element of the scalar tail
    skipped = 0
    for at in places:
        for bad in (float("nan"), float("inf"), float("-inf")):
            keep = g[at].item()
            g[at] = bad
            r = _measure(opt, g, 1.0)
            skipped += 1
            assert r["grad_nonfinite"] and r["steps_skipped"] == skipped and r["steps_taken"] == taken, (n, at, bad)
            g[at] = keep
    r = _measure(opt, g, 1.0)
    assert not r["grad_nonfinite"] and r["steps_taken"] == taken + 1          # a clean buffer leaves the flag clear


N2 = 4099
A, B_ = 0.1, 0.01                # two weight decays
# five stretches at odd boundaries, one of a single element; the (0.1, B_) group is empty
SEGS = [(0, 1001, 1.0, A), (1001, 1002, 0.1, A), (1002, 2047, 1.0, B_), (2047, 2047, 0.1, B_), (2047, 3333, 0.1, A), (3333, N2, 1.0, B_)]
GROUPS = [(1.0, A), (0.1, A), (1.0, B_), (0.1, B_)]


def _shadow(p0, lr):
    """torch.optim.AdamW over one nn.Parameter per stretch, grouped as SEGS says"""
    params = [torch.nn.Parameter(p0[b:e].clone()) for b, e, _, _ in SEGS]
    groups = [{"params": [q for q, s in zip(params, SEGS) if s[2:] == key and s[1] > s[0]], "lr": lr * key[0], "weight_decay": key[1]}
              for key in GROUPS]
    assert not groups[3]["params"]
    return params, torch.optim.AdamW(groups)


def _feed(params, g):
    for q, (b, e, _, _) in zip(params, SEGS):
        q.grad = g[b:e].clone()


def _close(a, b, what):
    d = (a - b).abs().max().item() if a.numel() else 0.0
    assert torch.allclose(a, b, rtol=RTOL, atol=ATOL), (what, d)


def _agree(opt, params, ref, what):
    torch.cuda.synchronize()
    for q, (b, e, _, _) in zip(params, SEGS):
        if e == b:
            continue
        _close(opt.p[b:e], q.detach(), f"{what}: parameters [{b}, {e})")
        _close(opt.m[b:e], ref.state[q]["exp_avg"], f"{what}: exp_avg [{b}, {e})")
        _close(opt.v[b:e], ref.state[q]["exp_avg_sq"], f"{what}: exp_avg_sq [{b}, {e})")


def test_four_steps_against_torch_adamw_with_clipping_groups_and_a_skipped_step(noise):
    from capf.optim import FusedAdamW
    lr, max_norm = 1e-3, 1.0
    p0 = noise[100:100 + N2].clone()
    params, ref = _shadow(p0, lr)
    opt = FusedAdamW(p0.clone(), lr=lr, weight_decay=0.5, max_grad_norm=max_norm, groups=SEGS)
    grads = [noise[10000 * (t + 1):10000 * (t + 1) + N2] * s for t, s in enumerate((1e-3, 5e-2, 1e-3, 1e-3))]

    def coef32(total):            # clip_grad_norm_'s own arithmetic, fp32
        return torch.clamp(max_norm / (total + 1e-6), max=1.0).item()

    # 1: max_norm far above the norm -> the coefficient is exactly 1
    _feed(params, grads[0])
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    ref.step()
    opt.step(grads[0])
    r = opt.report()
    assert total.item() < 0.1 and r["clip_coef"] == 1.0 and (r["steps_taken"], r["steps_skipped"]) == (1, 0)
    _agree(opt, params, ref, "step 1")
    # 2: a gradient 50 x larger is clipped; the fp64 sum puts the coefficient within 2 fp32 ulp of torch's
    _feed(params, grads[1])
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    ref.step()
    opt.step(grads[1])
    r = opt.report()
    want, got = np.float32(coef32(total)), np.float32(r["clip_coef"])
    print(f"  step 2: norm {r['grad_norm']:.9e} (torch fp32 {total.item():.9e}), coefficient {got!r} vs torch {want!r}")
    assert want < 0.5 and abs(float(got) - float(want)) <= 2 * float(np.spacing(want))
    _agree(opt, params, ref, "step 2")
    # 3: one NaN -> nothing is written, the count does not advance, and the shadow does not step (train.py:194)
    bad = grads[2].clone()
    bad[2046] = float("nan")
    before = [t.clone() for t in (opt.p, opt.m, opt.v)]
    opt.step(bad)
    r = opt.report()
    assert all(torch.equal(a, b) for a, b in zip(before, (opt.p, opt.m, opt.v)))
    assert (r["steps_taken"], r["steps_skipped"]) == (2, 1) and r["grad_nonfinite"]
    # 4: a clean gradient; the shadow's step is now 3 -- a counter that advanced on the skip has the wrong bias correction here
    _feed(params, grads[3])
    torch.nn.utils.clip_grad_norm_(params, max_norm)
    ref.step()
    opt.step(grads[3])
    assert all(int(ref.state[q]["step"]) == 3 for q, (b, e, _, _) in zip(params, SEGS) if e > b)
    assert (opt.report()["steps_taken"], opt.report()["steps_skipped"]) == (3, 1)
    _agree(opt, params, ref, "step 4")


def test_one_group_without_clipping_agrees_with_the_legacy_kernel(noise):
    from capf.optim import FusedAdamW
    p0 = noise[7:7 + N2].clone()
    old = FusedAdamW(p0.clone(), lr=6.4e-4, weight_decay=0.1)
    new = FusedAdamW(p0.clone(), lr=6.4e-4, weight_decay=0.1, skip_nonfinite=True)
    assert not old.guarded and new.guarded
    for t in range(3):
        g = noise[20000 * (t + 1):20000 * (t + 1) + N2] * 1e-2
        old.step(g, grad_scale=0.5)
        new.step(g, grad_scale=0.5)
        for a, b, what in ((old.p, new.p, "parameters"), (old.m, new.m, "exp_avg"), (old.v, new.v, "exp_avg_sq")):
            _close(a, b, f"step {t + 1} {what}")
    assert new.report()["steps_taken"] == 3 == old.t


def test_loss_accumulation(noise):
    from capf.optim import FusedAdamW
    opt = FusedAdamW(noise[:257].clone(), skip_nonfinite=True)
    g = noise[300:557] * 1e-3
    for loss, rows in ((0.5, 4), (float("nan"), 4), (0.25, 8)):
        opt.step(g, loss=torch.tensor(loss, device="cuda"), rows=rows)
    r = opt.report()
    assert r["loss_sum"] == 4.0 and r["loss_rows"] == 12.0 and r["nonfinite_losses"] == 1
    assert (r["steps_taken"], r["steps_skipped"]) == (3, 0)                   # the guard looks at the gradient, not at the loss


# ---- on the model -------------------------------------------------------------------------------------------------------
def _train_model(wseed):
    model, _ = make_model("hrnet_32", device="cuda", wseed=wseed)
    model.train(); model.backbone.eval(); model.volume_net.train()
    model.drop_path_rate = 0.0
    model.flat_grad_only = True
    return model


def _batch(seed, B=2):
    img, k2d, kc, gt = synth.synth_inputs(B, 256, 192, seed=seed, with_gt=True)
    return img.cuda(), k2d.cuda(), kc.cuda(), gt.cuda()


def _forward_backward(model, batch):
    from mvn.models.loss import MPJPE
    img, k2d, kc, gt = batch
    loss = MPJPE()(model(img, k2d, kc.clone()), gt)
    loss.backward()
    return loss.detach()


def _model_optimizer(model, flat, first_norm):
    from capf.optim import FusedAdamW
    from mvn.utils.cfg import config
    cfg = copy.deepcopy(config)
    cfg.train.volume_net_lr = 6.4e-4
    cfg.loss.grad_clip = 0.5 * first_norm * cfg.train.volume_net_lr           # max_grad_norm = half the first step's norm: clipping engages
    return FusedAdamW.from_config(cfg, model, flat, rules=[("sampling_offsets", 0.1)])


def _poisoned_step_is_skipped(model, opt, flat, clean, poisoned):
    with torch.no_grad():
        before = model(clean[0], clean[1], clean[2].clone())
    flat_before = flat.clone()
    taken = opt.report()["steps_taken"]
    loss = _forward_backward(model, poisoned)
    assert torch.isnan(loss)                                                  # the reference's own test (train.py:194) ...
    opt.step(model.last_flat_grad, loss=loss, rows=2)
    model.lifter_params_changed()
    r = opt.report()
    assert r["grad_nonfinite"]                                                # ... is subsumed by the gradient's: the guard rests on this
    assert r["steps_taken"] == taken and r["steps_skipped"] == 1 and r["nonfinite_losses"] == 1
    assert torch.equal(flat, flat_before)
    with torch.no_grad():
        after = model(clean[0], clean[1], clean[2].clone())
    assert torch.equal(before, after)                                         # bit for bit


def test_on_the_model_two_clipped_steps_match_torch_and_a_nan_keypoint_is_skipped():
    from capf.optim import flatten_
    model = _train_model(41)
    flat = flatten_(model.volume_net)
    batches = [_batch(50 + t) for t in range(3)]
    _forward_backward(model, batches[0])
    first_norm = model.last_flat_grad.double().norm().item()
    opt = _model_optimizer(model, flat, first_norm)
    assert len(opt.groups) == 9
    layout, _ = model.engine_for(batches[0][0]).grad_layout_cached()
    shadow = {n: torch.nn.Parameter(p.detach().clone()) for n, p in model.volume_net.named_parameters()}
    ref = torch.optim.AdamW([{"params": [p for n, p in shadow.items() if "sampling_offsets" not in n], "lr": opt.lr},
                             {"params": [p for n, p in shadow.items() if "sampling_offsets" in n], "lr": opt.lr * 0.1}], weight_decay=0.1)
    assert len(ref.param_groups[1]["params"]) == 8
    for t in range(2):
        if t:
            _forward_backward(model, batches[t])
        flat_g = model.last_flat_grad
        for n, p in shadow.items():
            off, cnt = layout["volume_net." + n]
            p.grad = flat_g[off:off + cnt].view(p.shape).clone()
        torch.nn.utils.clip_grad_norm_(list(shadow.values()), opt.max_grad_norm)
        ref.step()
        opt.step(flat_g)
        model.lifter_params_changed()
        r = opt.report()
        assert r["clip_coef"] < 1.0 and r["steps_taken"] == t + 1, r
        for n, p in model.volume_net.named_parameters():
            _close(p.detach(), shadow[n].detach(), f"step {t + 1} {n}")
    img, k2d, kc, gt = batches[2]
    k2d = k2d.clone()
    k2d[1, 5, 0] = float("nan")
    _poisoned_step_is_skipped(model, opt, flat, batches[0], (img, k2d, kc, gt))


def test_on_the_model_a_nan_pixel_gives_a_nan_loss_and_a_skipped_step():
    """A NaN in the IMAGE, as the reference sees it: torch's ReLU hands a NaN on, and so do the conv epilogues here (csrc/relu.h --
    fmaxf(t, 0) alone returned 0 for it, the stem's first ReLU swallowed the pixel and the poisoned batch trained on with a finite loss)."""
    from capf.optim import flatten_
    model = _train_model(42)
    flat = flatten_(model.volume_net)
    batches = [_batch(60 + t) for t in range(3)]
    _forward_backward(model, batches[0])
    opt = _model_optimizer(model, flat, model.last_flat_grad.double().norm().item())
    for t in range(2):
        if t:
            _forward_backward(model, batches[t])
        opt.step(model.last_flat_grad)
        model.lifter_params_changed()
    img, k2d, kc, gt = batches[2]
    img = img.clone()
    img[1, 100, 90, 1] = float("nan")
    _poisoned_step_is_skipped(model, opt, flat, batches[0], (img, k2d, kc, gt))


# ---- the checkpoint's 'optimizer' entry (train.py:398-407) ------------------------------------------------------------------
class _Two(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Linear(37, 11)
        self.sampling_offsets = torch.nn.Linear(11, 5)
        self.b = torch.nn.Linear(5, 3, bias=False)


def _torch_adamw(module, lr):
    named = list(module.named_parameters())
    return torch.optim.AdamW([{"params": [p for n, p in named if "sampling_offsets" not in n], "lr": lr},
                              {"params": [p for n, p in named if "sampling_offsets" in n], "lr": lr * 0.1}], weight_decay=0.1)


def _fused(module, lr):
    from capf.optim import FusedAdamW, flatten_, module_layout, param_groups
    flat = flatten_(module)
    opt = FusedAdamW(flat, lr=lr, weight_decay=0.1, groups=param_groups(module_layout(module, flat), [("sampling_offsets", 0.1)]))
    return opt.attach(module), flat


def _grads(module, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    return [torch.randn(p.shape, device="cuda", generator=g) * 1e-2 for p in module.parameters()]


def _same(mod_a, mod_b, what):
    for (n, a), b in zip(mod_a.named_parameters(), mod_b.parameters()):
        _close(a.detach(), b.detach(), f"{what} {n}")


def test_state_dict_round_trip_with_torch_adamw():
    torch.manual_seed(5)
    theirs = _Two().cuda()
    ours = copy.deepcopy(theirs)
    ref = _torch_adamw(theirs, 1e-3)
    for t in range(2):
        for p, g in zip(theirs.parameters(), _grads(theirs, 70 + t)):
            p.grad = g
        ref.step()
    # torch -> here: the moments and the step count resume
    ours.load_state_dict(theirs.state_dict())
    opt, flat = _fused(ours, 1e-3)
    opt.load_state_dict(ref.state_dict())
    g3 = _grads(theirs, 72)
    for p, g in zip(theirs.parameters(), g3):
        p.grad = g
    ref.step()
    opt.step(torch.cat([g.reshape(-1) for g in g3]))
    assert opt.report()["steps_taken"] == 3
    _same(ours, theirs, "after loading torch's state, step 3:")
    # here -> a fresh torch AdamW
    fresh = copy.deepcopy(ours)
    ref2 = _torch_adamw(fresh, 1e-3)
    sd = opt.state_dict()
    assert sorted(sd["state"]) == list(range(5)) and all(float(e["step"]) == 3.0 for e in sd["state"].values())
    assert [g["params"] for g in sd["param_groups"]] == [[0, 1, 2], [3, 4]] and sd["param_groups"][1]["lr"] == pytest.approx(1e-4)
    ref2.load_state_dict(copy.deepcopy(sd))          # (as a checkpoint file would: torch keeps same-dtype tensors it is handed, and these are views)
    g4 = _grads(theirs, 73)
    for p, g in zip(fresh.parameters(), g4):
        p.grad = g
    ref2.step()
    opt.step(torch.cat([g.reshape(-1) for g in g4]))
    _same(ours, fresh, "after torch loaded this state, step 4:")
    # one count for the whole buffer: unequal per-parameter steps are refused
    bad = ref.state_dict()
    bad["state"][0]["step"] = torch.tensor(7.0)
    with pytest.raises(ValueError, match="step"):
        opt.load_state_dict(bad)
