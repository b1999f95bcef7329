"""GPU: the default schedule (capf_set_lanes 3: two grouped chains on two streams at batch 16..128) computes what one chain on
the caller's stream computes, bit for bit.

HRNet-32 at 64 x 64 is the smallest input at which all four branches and the three-hop fuse chains exist.  Batch 2 runs a
region as one chain in either mode, batch 16 is where mode 3 switches to two chains.  Same kernels on the same operands in
every schedule compared here, so every comparison is torch.equal: a launch that starts before its producer has finished, or a
join that is missing, shows up as a difference (from the other schedule, or from call to call).

Batch 24 at 64 x 64 and at 96 x 96 are the engine-level runs of levels that mix kernel families: an F(4,3) Winograd group with a
lone F(2,3) conv (W = 2), and at 96 x 96 with the two-fp16-piece GEMM too (W = 3 is odd).  Batch 80 at 64 x 64 runs the
split-fp32 tile on the 16 x 16 .. 2 x 2 maps, which it takes from batch 79.

HRNet-32 bf16 at 128 x 128 is the 16-bit model beside them: the smallest runs in which the engine routes convs to the 2-D halo
tile (Engine::gemm_family: BF16_TILE, from 1 GFLOP per conv and batch 24).  What capf_op_info names there (checked below):
at batch 24 the tile runs layer1's four conv2 and transition1's 256 -> 32 conv -- the latter in ONE level with transition1's
stride-2 conv, which it does not run -- while every branch conv is still on igemm_bf16.hip's kernels; at batch 56 (the branch
convs reach 1 GFLOP at 53) the branch levels are tile launches on both concurrent chains.  (layer1's conv2 shares no level with
another conv at either batch: its block's downsample conv sits one level earlier, beside conv1.)"""
import contextlib
import copy
import io
import re

import pytest
import torch

from capf import synth

pytestmark = pytest.mark.gpu
H = W = 64
FUSE = 1


def _model(flags=0, dtype="fp32"):
    from mvn.models.conpose import CA_PF
    from mvn.utils.cfg import backbone_preset, config
    cfg = backbone_preset(copy.deepcopy(config), "hrnet_32")
    cfg.model.backbone.fix_weights = True
    with contextlib.redirect_stdout(io.StringIO()):
        model = CA_PF(cfg, compute_dtype=dtype, plan_flags=flags).eval()
    synth.load_synthetic(model, seed=3, bn_mode="random")
    return model.cuda()


@pytest.fixture(scope="module")
def models():
    return {"default": _model(), "one_chain": _model()}


@pytest.fixture(scope="module")
def models16():
    return {"default": _model(dtype="bf16"), "one_chain": _model(dtype="bf16")}


TILE_KERNEL = re.compile(r"^igemm_\w+_ws<")


def _tile_ops(eng, B):
    """names of the ops capf_op_info puts on the 2-D halo tile at batch B"""
    return {name for name, kern, _ in eng.op_table(B) if TILE_KERNEL.match(kern)}


def _inputs(B, size=H):
    img, k2d, kc = synth.synth_inputs(B, size, size, seed=5, crop_range=(size, size))
    return img.cuda(), k2d.cuda(), kc.cuda()


def _forward(model, inputs):
    img, k2d, kc = inputs
    eng = model.engine_for(img)
    with torch.no_grad():
        out = model(img, k2d, kc.clone()).clone()
    return out, [eng.tensor(f"feat{l}") for l in range(4)]


def _fuse_sums(model, inputs):
    """every fuse sum's output, read behind its region's join (a prefix run up to the op's checkpoint), by op index"""
    img = inputs[0]
    eng = model.engine_for(img)
    n = len(eng.op_schedule())
    descs = [eng.op_describe(i) for i in range(n)]
    sums = [i for i in range(n) if descs[i].kind == FUSE and descs[i].backbone]
    stream = torch.cuda.current_stream().cuda_stream
    got = {}
    for cp in sorted(set(descs[i].checkpoint for i in sums)):
        eng.forward_prefix(img, cp, stream)
        torch.cuda.synchronize()
        for i in sums:
            d = descs[i]
            if d.checkpoint == cp:
                got[i] = eng.op_tensor(i, 5, (img.shape[0], d.Ho, d.Wo, d.Cout), d.out_dtype).clone()
    return got


@pytest.mark.parametrize("B, size", [pytest.param(2, 64, id="2"), pytest.param(16, 64, id="16"), pytest.param(24, 64, id="24"),
                                     pytest.param(24, 96, id="96x96-24"), pytest.param(80, 64, id="80")])
def test_the_default_schedule_equals_one_chain(models, B, size):
    _default_equals_one_chain(models, B, size)


@pytest.mark.parametrize("B", [24, 56])
def test_the_default_schedule_equals_one_chain_with_2d_halo_tile_launches(models16, B):
    eng = models16["default"].engine_for(_inputs(B, 128)[0])
    tile = _tile_ops(eng, B)
    assert "backbone.transition1.0.0" in tile and "backbone.transition1.1.0.0" not in tile and "backbone.layer1.1.conv2" in tile
    sched = {name: s[:2] for (name, _, _), s in zip(eng.op_table(B), eng.op_schedule())}
    assert sched["backbone.transition1.0.0"] == sched["backbone.transition1.1.0.0"]          # one region, one level
    branch = {name for name in sched if ".branches." in name and ".conv" in name}
    assert len(branch) == 208 and (branch <= tile if B == 56 else not branch & tile)
    _default_equals_one_chain(models16, B, 128)


def test_a_launch_is_2d_halo_tile_convs_or_none_and_its_variant_says_which(models16):
    """Batch 24 at 128 x 128, the launch log of the product schedule: the members of every bracket (the ops that share a leader) are
    either all named igemm_*_ws<...> by capf_op_info or none is, and the bracket's variant is 3 exactly when they are.  (Until the
    engine routed these convs itself, transition1's level was one bracket of variant 3 around a tile launch and a ring launch.)"""
    B = 24
    img, k2d, kc = _inputs(B, 128)
    model = models16["default"]
    with torch.no_grad():
        out = model(img, k2d, kc.clone())
    eng = model.engine_for(img)
    _, leader = eng.forward_profile_launches(img, k2d, kc.clone(), torch.empty_like(out), torch.cuda.current_stream().cuda_stream)
    variants = eng.profile_variants()
    table = eng.op_table(B)
    members = {}
    for i, l in enumerate(leader):
        if l >= 0:
            members.setdefault(l, []).append(i)
    n_tile = 0
    for l, ops in members.items():
        on_tile = [bool(TILE_KERNEL.match(table[i][1])) for i in ops]
        assert all(on_tile) or not any(on_tile), [table[i][:2] for i in ops]
        assert (variants[l] == 3) == all(on_tile), (table[l][:2], variants[l])
        n_tile += all(on_tile)
    assert n_tile == 5                                         # layer1's four conv2, transition1's 256 -> 32 conv


def _default_equals_one_chain(models, B, size):
    inputs = _inputs(B, size)
    eng = models["default"].engine_for(inputs[0])               # (no set_lanes call on this engine: the handle's default)
    assert (1 in eng.op_stream_classes(B)) == (B >= 16)
    one = models["one_chain"].engine_for(inputs[0])
    one.set_lanes(2)
    assert set(one.op_stream_classes(B)) == {0}
    want_out, want_maps = _forward(models["one_chain"], inputs)
    want_sums = _fuse_sums(models["one_chain"], inputs)
    assert len(want_sums) == 2 + 4 * 3 + 2 * 4 + 1      # stage 2, stage 3, stage 4 (its last module keeps output 0)
    out, maps = _forward(models["default"], inputs)
    assert torch.equal(out, want_out), "joints"
    for l in range(4):
        assert torch.equal(maps[l], want_maps[l]), f"feat{l}"
    sums = _fuse_sums(models["default"], inputs)
    assert sums.keys() == want_sums.keys()
    for i in sums:
        assert torch.equal(sums[i], want_sums[i]), f"fuse sum op {i}"


@pytest.mark.parametrize("B", [2, 16])
def test_consecutive_forwards_and_a_side_torch_stream_give_the_same_bits(models, B):
    inputs = _inputs(B)
    first, first_maps = _forward(models["default"], inputs)
    for _ in range(2):                        # no event or stream state leaks from call to call
        again, maps = _forward(models["default"], inputs)
        assert torch.equal(again, first)
        assert all(torch.equal(a, b) for a, b in zip(maps, first_maps))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):             # the side chain forks from and joins to the caller's stream, whichever it is
        other, maps = _forward(models["default"], inputs)
    side.synchronize()
    assert torch.equal(other, first)
    assert all(torch.equal(a, b) for a, b in zip(maps, first_maps))


def test_backbone_forward_and_a_prefix_run_keep_working(models):
    inputs = _inputs(16)
    _, want_maps = _forward(models["default"], inputs)
    img = inputs[0]
    eng = models["default"].engine_for(img)
    stream = torch.cuda.current_stream().cuda_stream
    eng.backbone_forward(img, stream)
    torch.cuda.synchronize()
    assert all(torch.equal(eng.tensor(f"feat{l}"), want_maps[l]) for l in range(4))
    # a prefix that ends inside a fuse layer's region runs that region in program order on the caller's stream
    sched = eng.op_schedule()
    descs = [eng.op_describe(i) for i in range(len(sched))]
    cls = eng.op_stream_classes(16)
    i = max(k for k in range(len(sched)) if cls[k] == 1 and descs[k].kind == FUSE)          # the last fuse sum of a side chain
    d = descs[i]
    eng.forward_prefix(img, d.checkpoint, stream)
    torch.cuda.synchronize()
    whole = eng.op_tensor(i, 5, (16, d.Ho, d.Wo, d.Cout), d.out_dtype).clone()
    eng.forward_prefix(img, i + 1, stream)
    torch.cuda.synchronize()
    assert torch.equal(eng.op_tensor(i, 5, (16, d.Ho, d.Wo, d.Cout), d.out_dtype), whole)
