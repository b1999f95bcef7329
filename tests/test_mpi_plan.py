"""CPU (plan-only handles, device = -1): training plans of the MPI-INF-3DHP variant (no context blocks) at any depth 1..8.

ContextPose_mpi/run_3dhp.py:60-101 trains VolumetricTriangulationNet, whose PoseTransformer builds config.depth blocks per group
(ContextPose_mpi/model/pose_dformer.py:199, 217-227).  capf_create accepts training = 1 with depth != levels for that variant at the
app's two widths (embed 64 over base 32, 96 over 48); the H36M model (context_blocks = 1) still needs depth == levels, and its schema, gradient layout and workspace sizes are unchanged (the
numbers below were read from the library before depth-aware training plans existed)."""
import copy
import json
import math
import os

import pytest

from conftest import ROOT


def _mpi_cfg(backbone, depth):
    from model.conpose import mpi_preset
    from mvn.utils.cfg import config
    cfg = mpi_preset(copy.deepcopy(config), backbone)
    cfg.model.poseformer.depth = depth
    return cfg


def _h36m_cfg(backbone):
    from mvn.utils.cfg import backbone_preset, config
    c = backbone_preset(copy.deepcopy(config), backbone)
    c.model.backbone.fix_weights = True
    return c


def _plan(cfg, context_blocks, training=1, depth=None, H=256, W=192):
    from capf import Engine
    from mvn.models import _native
    c = _native.make_capf_config(cfg, H, W, context_blocks=context_blocks)
    c.training = training
    if depth is not None:
        c.depth = depth
    return Engine(c, device=None)


@pytest.mark.parametrize("backbone,embed", [("hrnet_32", 64), ("hrnet_48", 96)])
@pytest.mark.parametrize("depth", range(1, 9))
def test_training_plan_accepted_and_gradient_offsets_cover_volume_net(backbone, embed, depth):
    """Every volume_net parameter of the variant has exactly one slice of the flat gradient, the slices tile [0, total) without gaps
    or overlaps in schema order, and the step's two-piece table holds the four feat_embed linears plus four linears per block."""
    eng = _plan(_mpi_cfg(backbone, depth), False)
    try:
        schema = eng.schema()
        lifter = [(n, s) for n, s, _ in schema if n.startswith("volume_net.")]
        assert sum(n.endswith(".attn.qkv.weight") for n, _ in lifter) == 2 * depth
        assert not any(".context_blocks." in n for n, _ in lifter)
        assert list(dict(lifter)["volume_net.res_blocks.0.attn.qkv.weight"]) == [3 * embed, embed]
        layout, total = eng.grad_layout()
        assert set(layout) == {n for n, _ in lifter}
        cur = 0
        for n, s in lifter:                                      # schema (= registration) order, back to back
            off, cnt = layout[n]
            assert off == cur and cnt == math.prod(s), (n, off, cur, cnt, s)
            cur += cnt
        assert cur == total
        assert eng.lib.capf_train_h2_matrices(eng.h) == 4 + 8 * depth
        assert eng.workspace_bytes(160) > eng.workspace_bytes(5) > 0
    finally:
        eng.close()


def test_training_workspace_grows_with_depth():
    sizes = []
    for depth in range(1, 9):
        eng = _plan(_mpi_cfg("hrnet_32", depth), False)
        sizes.append(eng.workspace_bytes(13))
        eng.close()
    assert all(b > a for a, b in zip(sizes, sizes[1:])), sizes


def test_depth_refusals_that_remain():
    """depth != levels together with context blocks (same text as before), and depth outside 1..8, are still refused."""
    from capf.lib import CapfError
    for depth in (1, 2, 3, 5, 8):
        with pytest.raises(CapfError, match="only for the variant without context blocks"):
            _plan(_h36m_cfg("hrnet_32"), True, depth=depth)
        with pytest.raises(CapfError, match="only for the variant without context blocks"):
            _plan(_h36m_cfg("hrnet_32"), True, training=0, depth=depth)
    for depth in (9, 12, -1):
        for training in (0, 1):
            with pytest.raises(CapfError, match="1..8 blocks per group"):
                _plan(_mpi_cfg("hrnet_32", 4), False, training=training, depth=depth)


def test_depth_training_plans_at_the_variants_widths_only():
    """test_abi.py's depth test, extended to training plans: at the ContextPose_mpi widths (embed 64 over base 32, 96 over 48;
    run_3dhp.py:219-232) a training plan builds `depth` blocks per group; at any other width without context blocks (the H36M preset's
    embed 128, or a hand-made 64 over 48) depth != levels stays inference-only, and depth == levels trains as before."""
    from capf.lib import CapfError
    for backbone in ("hrnet_32", "hrnet_48"):
        for depth in (1, 2, 6, 8):
            for training in (0, 1):
                eng = _plan(_mpi_cfg(backbone, depth), False, training=training)
                names = [n for n, _, _ in eng.op_table(2)]
                schema = [s[0] for s in eng.schema()]
                eng.close()
                assert sum(n.endswith(".qkv") and n.startswith("joint") for n in names) == depth
                assert sum(s.endswith("attn.qkv.weight") for s in schema) == 2 * depth
    odd = _mpi_cfg("hrnet_48", 2)
    odd.model.poseformer.embed_dim_ratio = 64
    for cfg in (_h36m_cfg("hrnet_32"), _h36m_cfg("hrnet_48"), odd):
        for depth in (2, 6):
            _plan(cfg, False, training=0, depth=depth).close()
            with pytest.raises(CapfError, match="only at the ContextPose_mpi widths"):
                _plan(cfg, False, training=1, depth=depth)
        _plan(cfg, False, training=1, depth=4).close()
    # the host module asks for a training plan only where one exists (mvn/models/_native.py)
    from mvn.models import _native
    assert _native.make_capf_config(_mpi_cfg("hrnet_32", 2), 256, 192, context_blocks=False).training == 1
    h = _h36m_cfg("hrnet_32")
    h.model.poseformer.depth = 2
    assert _native.make_capf_config(h, 256, 192, context_blocks=False).training == 0
    assert _native.make_capf_config(h, 256, 192, context_blocks=True).training == 1


# H36M training plans at 256 x 192 before this change: workspace bytes per batch, flat-gradient elements, two-piece matrices
H36M_PINS = {
    "hrnet_32": dict(grad=14094147, h2=56, ws={1: 784630784, 5: 853041920, 13: 989866240, 160: 3504022016, 512: 9524313856}),
    "hrnet_48": dict(grad=14155587, h2=56, ws={1: 785723648, 5: 857225984, 13: 1000232704, 160: 3627990016, 512: 9920307456}),
    "cpn": dict(grad=14233411, h2=60, ws={1: 793374720, 5: 894384384, 13: 1096405760, 160: 4808557568, 512: 13697519872}),
}


@pytest.mark.parametrize("backbone", sorted(H36M_PINS))
def test_h36m_training_plan_unchanged(backbone):
    want_schema = json.load(open(os.path.join(ROOT, "tests", "golden", f"schema_{backbone}.json")))
    eng = _plan(_h36m_cfg(backbone), True)
    try:
        assert {n: list(s) for n, s, _ in eng.schema()} == want_schema
        pins = H36M_PINS[backbone]
        assert {b: eng.workspace_bytes(b) for b in pins["ws"]} == pins["ws"]
        layout, total = eng.grad_layout()
        assert total == pins["grad"] and len(layout) == 191
        assert eng.lib.capf_train_h2_matrices(eng.h) == pins["h2"]
    finally:
        eng.close()


@pytest.mark.parametrize("depth", [1, 4, 6])
def test_drop_masks_layout_of_the_variant(depth):
    """CA_PF._drop_masks without context blocks: res [depth][2][B*17] then joint [depth][2][B] (include/capf.h), rates
    linspace(0, 0.2, depth) shared by res block i and joint block i (ContextPose_mpi/model/pose_dformer.py:215) -- the first
    block of each group never drops; with context blocks the H36M layout, ctx | res | joint over `levels`, is unchanged."""
    import contextlib, io
    import torch
    from model.conpose import VolumetricTriangulationNet
    with contextlib.redirect_stdout(io.StringIO()):
        m = VolumetricTriangulationNet(_mpi_cfg("hrnet_32", depth))
    m.train()
    B = 64
    torch.manual_seed(3)
    masks = m._drop_masks(B, torch.device("cpu"))
    assert masks.numel() == 2 * depth * (B * 17 + B)
    res = masks[:2 * depth * B * 17].view(depth, 2, B * 17)
    joint = masks[2 * depth * B * 17:].view(depth, 2, B)
    assert torch.equal(res[0], torch.ones_like(res[0])) and torch.equal(joint[0], torch.ones_like(joint[0]))
    rates = torch.linspace(0, 0.2, depth).tolist()
    for i in range(1, depth):
        keep = 1.0 - rates[i]
        for t in (res[i], joint[i]):
            nz = torch.unique(t[t != 0])
            assert nz.numel() <= 1 and (nz.numel() == 0 or abs(nz.item() * keep - 1.0) < 1e-6), (i, nz)
    # the H36M model: same draws, same layout as before (ctx | res | joint, `levels` blocks each)
    from conftest import make_model
    h, _ = make_model("hrnet_32")
    h.train()
    torch.manual_seed(3)
    hm = h._drop_masks(B, torch.device("cpu"))
    torch.manual_seed(3)
    want = []
    for per in (B, B * 17, B):
        for r in torch.linspace(0, 0.2, 4).tolist():
            for _ in range(2):
                want.append(torch.ones(per) if r == 0.0 else torch.empty(per).bernoulli_(1.0 - r).div_(1.0 - r))
    assert torch.equal(hm, torch.cat(want))
