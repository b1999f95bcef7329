"""CPU: the host side of the guarded AdamW step -- capf.optim.param_groups turns Engine.grad_layout() and name rules
(ContextPose_mpi/run_3dhp.py:260-277: sampling_offsets at 0.1 x lr) into the merged segment list the kernel takes, and
FusedAdamW.from_config reads the reference's config keys (ContextPose/train.py:196-200, 335).  No GPU: nothing is launched."""
import copy

import pytest
import torch

from conftest import make_model


def _check_cover(segs, total):
    at = 0
    for b, e, _, _ in segs:
        assert b == at and e > b            # sorted, disjoint, no gap, none empty
        at = e
    assert at == total


def test_param_groups_on_a_synthetic_layout():
    from capf.optim import param_groups
    layout = {"a.weight": (0, 7), "a.bias": (7, 1), "blk.sampling_offsets.weight": (8, 5), "blk.sampling_offsets.bias": (13, 3),
              "b.weight": (16, 9), "c.sampling_offsets.weight": (25, 2)}
    segs = param_groups(layout, [("sampling_offsets", 0.1)], total=27)
    # adjacent parameters of one group are ONE segment
    assert segs == [(0, 8, 1.0, None), (8, 16, 0.1, None), (16, 25, 1.0, None), (25, 27, 0.1, None)]
    _check_cover(segs, 27)
    # a weight decay of the rule's own, and the first matching rule wins
    segs = param_groups(layout, [("c.sampling", 0.5, 0.0), ("sampling_offsets", 0.1)], total=27)
    assert segs[-1] == (25, 27, 0.5, 0.0) and segs[1] == (8, 16, 0.1, None)
    # a rule that matches nothing, or no rule: one segment
    assert param_groups(layout, [("no_such_name", 0.1)]) == [(0, 27, 1.0, None)]
    assert param_groups(layout) == [(0, 27, 1.0, None)]
    # a layout that does not tile the buffer is refused
    with pytest.raises(ValueError):
        param_groups({"a": (0, 4), "b": (5, 3)})
    with pytest.raises(ValueError):
        param_groups(layout, total=28)


def test_more_than_64_segments_raises():
    from capf.optim import param_groups
    layout = {f"p{i}.{'sampling_offsets' if i % 2 else 'weight'}": (3 * i, 3) for i in range(65)}
    with pytest.raises(ValueError, match="64"):
        param_groups(layout, [("sampling_offsets", 0.1)])
    layout.pop("p64.weight")
    assert len(param_groups(layout, [("sampling_offsets", 0.1)])) == 64


def test_param_groups_on_the_hrnet32_plan_layout():
    from capf import Engine
    from capf.optim import param_groups
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), "hrnet_32")
    cfg.model.backbone.fix_weights = True
    eng = Engine(_native.make_capf_config(cfg, 256, 192), device=None)
    layout, total = eng.grad_layout()
    segs = param_groups(layout, [("sampling_offsets", 0.1)], total=total)
    _check_cover(segs, total)
    assert all(a[2:] != b[2:] for a, b in zip(segs, segs[1:]))          # merged: neighbours differ
    low = [(b, e) for b, e, f, _ in segs if f == 0.1]
    assert {f for _, _, f, _ in segs} == {1.0, 0.1}
    # every sampling_offsets element lands in the 0.1 group, and nothing else does
    want = sorted((off, off + n) for name, (off, n) in layout.items() if "sampling_offsets" in name)
    assert want and sum(e - b for b, e in low) == sum(e - b for b, e in want)
    for b, e in want:
        assert any(lb <= b and e <= le for lb, le in low)
    # one context block per level, weight + bias adjacent: four low-lr stretches, nine segments in all
    assert len(low) == 4 and len(segs) == 9
    assert param_groups(layout, [("no_such_name", 0.1)], total=total) == [(0, total, 1.0, None)]
    eng.close()


@pytest.mark.parametrize("grad_clip, lr", [(0, 1e-3), (0.005, 1e-3), (2.0, 6.4e-4)])
def test_from_config_reads_the_reference_keys(grad_clip, lr):
    from capf.optim import FusedAdamW, flatten_
    from mvn.utils.cfg import config
    model, _ = make_model("hrnet_32")
    flat = flatten_(model.volume_net)
    cfg = copy.deepcopy(config)
    cfg.loss.grad_clip, cfg.train.volume_net_lr = grad_clip, lr
    opt = FusedAdamW.from_config(cfg, model, flat, rules=[("sampling_offsets", 0.1)])
    assert opt.guarded and opt.lr == lr and opt.wd == 0.1
    assert opt.max_grad_norm == (grad_clip / lr if grad_clip else 0.0)      # train.py:199 divides; 0 = no clipping
    assert len(opt.groups) == 9 and [n for n, _, _ in opt.layout] == [n for n, _ in model.volume_net.named_parameters()]
    # lr stays a plain attribute (train.py:410-412); the group rates follow it
    opt.lr *= 0.99
    rates = {round(s.lr / opt.lr, 6) for s in opt._segments()}
    assert rates == {1.0, 0.1}
    # the legacy constructor keeps the legacy route
    assert not FusedAdamW(flat, lr=lr, weight_decay=0.1).guarded


def test_skip_is_part_of_the_guarded_route_not_a_switch():
    from capf.optim import FusedAdamW
    flat = torch.zeros(10)
    assert not FusedAdamW(flat, skip_nonfinite=False).guarded and FusedAdamW(flat, skip_nonfinite=True).guarded
    assert FusedAdamW(flat, max_grad_norm=1.0).guarded
    for kw in (dict(max_grad_norm=1.0), dict(groups=[(0, 10, 1.0, None)])):
        with pytest.raises(ValueError, match="skip_nonfinite"):
            FusedAdamW(flat, skip_nonfinite=False, **kw)


class _OnlyOffsets(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.sampling_offsets = torch.nn.Linear(3, 2)


def test_state_groups_without_a_default_member_and_with_other_rates():
    from capf.optim import FusedAdamW, flatten_, module_layout, param_groups
    mod = _OnlyOffsets()
    flat = flatten_(mod)
    opt = FusedAdamW(flat, lr=1e-3, groups=param_groups(module_layout(mod, flat), [("sampling_offsets", 0.1)])).attach(mod)
    assert [(f, idx) for f, _, idx in opt._param_groups()] == [(0.1, [0, 1])]          # no empty default group, as torch has none
    ref = torch.optim.AdamW([{"params": list(mod.parameters()), "lr": 2e-4}], weight_decay=0.1)
    opt.load_state_dict(ref.state_dict())
    assert opt.lr == pytest.approx(2e-3) and opt.t == 0
    # a loaded group whose rate does not follow this optimizer's factors is refused, not ignored
    two = torch.nn.Sequential(torch.nn.Linear(3, 2), _OnlyOffsets())
    flat2 = flatten_(two)
    opt2 = FusedAdamW(flat2, lr=1e-3, groups=param_groups(module_layout(two, flat2), [("sampling_offsets", 0.1)])).attach(two)
    named = list(two.named_parameters())
    other = torch.optim.AdamW([{"params": [p for n, p in named if "sampling" not in n], "lr": 1e-3},
                               {"params": [p for n, p in named if "sampling" in n], "lr": 5e-4}], weight_decay=0.1)
    with pytest.raises(ValueError, match="lr"):
        opt2.load_state_dict(other.state_dict())
