"""GPU: the training step of the full H36M model (context blocks, depth == levels) at every kind of lifter width Engine::build() accepts,
against the fp64 yardstick (train_yardstick.py).

The step, the yardstick and the bounds are test_gpu_train_matrix.py's, unchanged: forward + MPJPE + backward through CA_PF in train mode
(backbone eval) with debug taps on; deformable corners bit for bit against the index rule, prediction within 1e-5, loss within 1e-6
relative, all 191 gradients within 2e-5 relative L2 and 2e-5 of the fp64 gradient's largest entry.  Only embed_dim_ratio moves: that test
runs at 128 alone.  With C = embed_dim_ratio and D = 5 C the res and context blocks work on C-wide rows ("res rows": 5 or 4 tokens per
joint), the joint blocks on D-wide rows of 17 tokens ("joint rows"), and every branch below is taken by C or D (the rules are restated
under "routes", with their csrc lines; every case asserts the routes it is here for, and the module ends on what the cases cover together).

The only case to reach it (crop 128 x 96 unless said: maps of 32 x 24 ... 4 x 3, most samples next to a border):
  W32 fp32  32 B=2    fp32 pipe at C < 64: attention_bwd<5> at d = 4, <17> at d = 20
  W32 fp32  32 B=6    a two-piece step whose table (48 matrices) lacks feat_embed (N = 32), embed_proj.0 and the res proj, holds fc2
                      (context, res) only as W^T and the res qkv / fc1 only as W; no layer on wgrad_tn_h2_kernel (D = 160); embed_proj's
                      transposes wider than qkv's (train_layout tA / tB)
  W32 fp32  32 B=100  (added with the fix of the bug these cases led to) embed_proj.3's transposed operand, 256 channels x 6816 rows, is twice
                      what train_layout gave tA / tB below width 128 (15 C floats per joint against 4 x 256): it ran over the transposed-weight
                      area into the slab area, where the context MLP's weight-gradient slabs of 13 slices wait for their sum
  W32 fp32  64 B=6    C on the 64-column threshold of the table: feat_embed and the res proj enter it, both sides of every pair; D = 320
  W32 fp32  96 B=13   D = 480; wgrad_tn_kernel in more than one row slice under a two-piece step; DropPath 0.2 (embed_proj on wgrad_tn)
  W32 fp32 160 B=6    layernorm_train<10> / layernorm_bwd<10> on res rows (with 288: B=2, B=13 and W48), <24> on joint rows at D = 800
  W32 fp32 256 B=2    <24> on the fp32 pipe; wgrad_tn_kernel on 1280-wide layers
  W32 fp32 256 B=13   256 x 256 crop (ref beyond +-1), DropPath 0.2: wgrad_tn_h2_kernel on every C- and D-wide layer, its slabs 4 x the
                      default width's, more than one slice; embed_proj (N = 64) in the table as W
  W32 fp32 288 B=2    the widest width accepted: attention_bwd<17> at d = 180 (51 680 bytes of LDS), <5> at d = 36
  W32 fp32 288 B=13   two-piece forward / dX GEMMs at D = 1440 with every weight gradient on wgrad_tn_kernel
  W48 fp32 288 B=6    feat_embed.0 / embed_proj.0 with K = 48: the zero-padded weight copies (wpad) at C != 128
  W48 bf16  96 B=5    bf16 maps into the samplers and deform_bwd at a narrow width; no table, so the fp32 pipe at B >= 5
  CPN fp32  64 B=6    256-channel maps four times wider than the tokens, 256 x 192 crop
Instances and the cases that reach them -- layernorm <2> on res rows: 32, 64 and 96; <10> on res rows: 160, 256 and 288; <10> on joint rows:
32 .. 96; <24> on joint rows: 160 .. 288; wgrad_tn_h2_kernel: 256 B=13 ALONE; wgrad_tn_kernel under a two-piece step in several slices:
32 B=100, 96 B=13 and 288 B=13; the bf16 maps: W48 bf16 ALONE.

Measured (worst relative L2 | worst max entry of the 191 gradients, MI355X; EXPERIMENTS.md R16.1): 4.9e-7 | 6.1e-7 (32 B=2),
6.5e-7 | 9.2e-7 (32 B=6), 4.6e-7 | 9.8e-7 (64), 1.5e-6 | 1.9e-6 (96), 4.9e-7 | 1.1e-6 (160), 7.7e-7 | 1.2e-6 and 9.1e-7 | 1.3e-6 (256),
8.4e-7 | 9.4e-7 and 5.5e-7 | 1.2e-6 (288), 5.8e-7 | 9.6e-7 (W48 288), 1.1e-6 | 9.7e-7 (W48 bf16 96), 5.8e-6 | 8.3e-6 (CPN 64): no growth
with the width, and no width needed a bound from the float32 oracle (max(2e-5, 2 x its own error) would apply to a width whose
kernels exceed 2e-5 without an error in the code).
Found here: train_layout's tA / tB (the 32 B=100 case; before the fix context_blocks.*.mlp.fc{1,2} were 8e+02 off), and the yardstick's
blind spot at the border clip (160 B=6: one coordinate exactly ON the last pixel in fp32 and 2.6e-7 inside it in float64 --
train_yardstick.py (c), engine_clip_sides)."""
import pytest
import torch

from capf import synth
from lifter_models import lifter_model
from test_gpu_train_matrix import H2G_MIN_BATCH, _hold_to_yardstick, _step
from train_yardstick import check_cells_against_index_rule

pytestmark = pytest.mark.gpu

J, LEVELS, HEADS, DEFORM_HEADS, DEFORM_SAMPLES = 17, 4, 8, 4, 4
MAP_CHANNELS = {"hrnet_32": (32, 64, 128, 256), "hrnet_48": (48, 96, 192, 384), "cpn": (256, 256, 256, 256)}
WIDTHS = tuple(range(32, 289, 32))       # Engine::build (csrc/plan.cpp): embed_dim_ratio % 32 == 0 and 5 * embed_dim_ratio <= 1536


# ---- routes: the selection rules of the training step, restated -----------------------------------------------------------------------
def layernorm_instance(which, C):
    """csrc/train_kernels.hip launch_layernorm_train (:73-86) / launch_layernorm_bwd (:141-154): values per lane by the row width"""
    assert which in ("train", "bwd") and C <= 1536
    return f"layernorm_{which}<{2 if C <= 128 else 10 if C <= 640 else 24}>"


def attention_bwd_instance(N, d):
    """csrc/train_kernels.hip launch_attention_bwd (:761-779): NMAX by the token count; q, k, v, dO [NMAX][d + 1] and P, dS
    [NMAX][NMAX + 1] floats of dynamic LDS, refused above 64 KiB.  Returns (instance, LDS bytes)."""
    nmax = 5 if N <= 5 else 17
    assert N <= 17
    lds = (4 * nmax * (d + 1) + 2 * nmax * (nmax + 1)) * 4
    assert lds <= 64 * 1024
    return f"attention_bwd<{nmax}> d={d}", lds


def step_linears(C, maps, drop):
    """Every nn.Linear product of the step whose weight gradient is a GEMM (csrc/train.cpp forward_train / backward):
    (name, N, K, rows per frame, plain).  plain: dY and X are read with plain row pitches (RowMap G == 1), t_linear_bwd's condition
    (:285) for wgrad_tn; embed_proj's dY is the [b, p, 1 + l, h * HD:] slice of dX (G = NH) unless DropPath copies it out scaled."""
    D, HD = (LEVELS + 1) * C, C // DEFORM_HEADS
    out = [(f"feat_embed.{l}", C, maps[l], J, True) for l in range(LEVELS)]
    for i in range(LEVELS):
        out.append((f"ctx{i}.attn_off", 3 * DEFORM_HEADS * DEFORM_SAMPLES, C, J * LEVELS, True))
        out += [(f"ctx{i}.embed_proj.{l}", HD, maps[l], J * DEFORM_HEADS, bool(drop)) for l in range(LEVELS)]
        out += [(f"ctx{i}.fc1", 2 * C, C, J * LEVELS, True), (f"ctx{i}.fc2", C, 2 * C, J * LEVELS, True)]
    for g, dim, rows in (("res", C, J * (LEVELS + 1)), ("joint", D, J)):
        for i in range(LEVELS):
            out += [(f"{g}{i}.qkv", 3 * dim, dim, rows, True), (f"{g}{i}.proj", dim, dim, rows, True),
                    (f"{g}{i}.fc1", 2 * dim, dim, rows, True), (f"{g}{i}.fc2", dim, 2 * dim, rows, True)]
    return out


def h2_table(C, maps, dtype):
    """csrc/train.cpp t_h2_plan (:116-143): [(name, W packed for y = x W^T, W^T packed for dX = dY W)] -- a side joins with at least 64
    output columns of its product (N for the forward, K for dX); the 48-column [attention_weights | sampling_offsets] pack never
    does (3 * NH * NS >= 64 is false); feat_embed's dX is no part of a parameter step; no table under a 16-bit compute dtype."""
    if dtype != "fp32":
        return []
    tab = []
    for name, N, K, _, _ in step_linears(C, maps, 0.0):
        if name.endswith(".attn_off"):
            continue
        fwd, bwd = N >= 64, K >= 64 and not name.startswith("feat_embed.")
        if fwd or bwd:
            tab.append((name, fwd, bwd))
    return tab


def wgrad_route(N, K, rows, plain, two_piece, D):
    """csrc/train.cpp t_linear_bwd (:285-315): the kernel of one weight gradient and its number of row slices."""
    if not (plain and N % 4 == 0 and K % 4 == 0):
        return "transpose_pad + igemm_f32", 1
    h2 = two_piece and N % 128 == 0 and K % 128 == 0            # (:291: the two-piece kernel's 128 x 128 slabs)
    tiles = (N // 128) * (K // 128) if h2 else ((N + 63) // 64) * ((K + 63) // 64)
    chunks = (rows + 31) // 32
    slab, slab_cap = N * K + N, 16 * (3 * D * D + 3 * D)          # (train_layout :89)
    splits = max(1, ((512 if h2 else 2048) + tiles - 1) // tiles)
    splits = min(splits, max(1, chunks // 16))
    splits = min(splits, max(1, slab_cap // slab))
    cps = (chunks + splits - 1) // splits
    return ("wgrad_tn_h2_kernel" if h2 else "wgrad_tn_kernel"), (chunks + cps - 1) // cps


def routes(backbone, dtype, E, B, drop):
    """The set of route names a case takes, and the number of table entries its plan must report."""
    maps, D = MAP_CHANNELS[backbone], (LEVELS + 1) * E
    table = h2_table(E, maps, dtype)
    two_piece = bool(table) and B >= H2G_MIN_BATCH                # (t_h2_prepare :167)
    pipe = "two-piece" if two_piece else "fp32 pipe"
    r = {f"{dtype} maps"}
    for which in ("train", "bwd"):
        r.add(layernorm_instance(which, E) + " res rows")
        r.add(layernorm_instance(which, D) + " joint rows")
    r.add(attention_bwd_instance(LEVELS + 1, E // HEADS)[0])
    r.add(attention_bwd_instance(J, D // HEADS)[0])
    for name, N, K, rows, plain in step_linears(E, maps, drop):
        kern, slices = wgrad_route(N, K, rows * B, plain, two_piece, D)
        r.add(f"{kern} | {pipe}")
        if slices > 1:
            r.add(f"{kern} | {pipe} | slices > 1")
    return r, table, pipe


# every instance a width Engine::build accepts can reach: both LayerNorm kernels in <2> and <10> on res rows (<24> would need C > 640), in
# <10> and <24> on joint rows (<2> would need 5 C <= 128); both weight-gradient kernels under both pipes, except that wgrad_tn_h2_kernel
# exists under a two-piece step only (t_linear_bwd :291 asks for the step's packs)
REACHABLE = ({f"layernorm_{w}<{v}> {rows}" for w in ("train", "bwd") for v, rows in ((2, "res rows"), (10, "res rows"), (10, "joint rows"),
                                                                                     (24, "joint rows"))} |
             {"wgrad_tn_kernel | fp32 pipe", "wgrad_tn_kernel | two-piece", "wgrad_tn_h2_kernel | two-piece",
              "wgrad_tn_kernel | two-piece | slices > 1", "wgrad_tn_h2_kernel | two-piece | slices > 1", "fp32 maps", "bf16 maps"})

LN2R, LN10R, LN10J, LN24J = ({f"layernorm_train<{v}> {rows}", f"layernorm_bwd<{v}> {rows}"}
                             for v, rows in ((2, "res rows"), (10, "res rows"), (10, "joint rows"), (24, "joint rows")))
TN, TNH2 = "wgrad_tn_kernel", "wgrad_tn_h2_kernel"

CASES = [
    # backbone, dtype, E, (H, W), B, DropPath rate, table entries, routes the case is here for
    ("hrnet_32", "fp32", 32, (128, 96), 2, 0.0, 48, LN2R | LN10J | {"attention_bwd<5> d=4", "attention_bwd<17> d=20", f"{TN} | fp32 pipe"}),
    ("hrnet_32", "fp32", 32, (128, 96), 6, 0.0, 48, LN2R | LN10J | {f"{TN} | two-piece"}),
    ("hrnet_32", "fp32", 32, (128, 96), 100, 0.0, 48, LN2R | LN10J | {f"{TN} | two-piece | slices > 1", "transpose_pad + igemm_f32 | two-piece"}),
    ("hrnet_32", "fp32", 64, (128, 96), 6, 0.0, 56, LN2R | LN10J | {f"{TN} | two-piece", "attention_bwd<17> d=40"}),
    ("hrnet_32", "fp32", 96, (128, 96), 13, 0.2, 56, LN2R | LN10J | {f"{TN} | two-piece | slices > 1", "attention_bwd<17> d=60"}),
    ("hrnet_32", "fp32", 160, (128, 96), 6, 0.0, 56, LN10R | LN24J | {f"{TN} | two-piece", "attention_bwd<17> d=100"}),
    ("hrnet_32", "fp32", 256, (128, 96), 2, 0.0, 60, LN10R | LN24J | {f"{TN} | fp32 pipe", "attention_bwd<17> d=160"}),
    ("hrnet_32", "fp32", 256, (256, 256), 13, 0.2, 60, LN10R | LN24J | {f"{TNH2} | two-piece | slices > 1"}),
    ("hrnet_32", "fp32", 288, (128, 96), 2, 0.0, 60, LN10R | LN24J | {"attention_bwd<17> d=180", "attention_bwd<5> d=36", f"{TN} | fp32 pipe"}),
    ("hrnet_32", "fp32", 288, (128, 96), 13, 0.0, 60, LN10R | LN24J | {f"{TN} | two-piece | slices > 1"}),
    ("hrnet_48", "fp32", 288, (128, 96), 6, 0.0, 60, LN10R | LN24J | {f"{TN} | two-piece"}),
    ("hrnet_48", "bf16", 96, (128, 96), 5, 0.0, 0, LN2R | LN10J | {"bf16 maps", f"{TN} | fp32 pipe"}),
    ("cpn", "fp32", 64, (256, 192), 6, 0.0, 60, LN2R | LN10J | {f"{TN} | two-piece"}),
]


def _id(case):
    b, d, e, (h, w), n, p = case[:6]
    return f"{b}-{d}-E{e}-{h}x{w}-B{n}" + ("-droppath" if p else "")


@pytest.mark.parametrize("case", CASES, ids=[_id(c) for c in CASES])
def test_training_step_vs_fp64_yardstick_at_width(case):
    backbone, dtype, E, (H, W), B, drop, n_table, pins = case
    torch.set_num_threads(min(16, torch.get_num_threads()))
    taken, table, pipe = routes(backbone, dtype, E, B, drop)
    assert pins <= taken, sorted(pins - taken)
    assert len(table) == n_table
    if (E, B) == (288, 2):
        assert attention_bwd_instance(J, 5 * E // HEADS)[1] == 51680
    if (E, B) == (256, 13):                                     # every C- and D-wide layer of the res / joint / context-MLP blocks
        D = 5 * E
        assert all(wgrad_route(N, K, r * B, p, True, D)[0] == TNH2 for nm, N, K, r, p in step_linears(E, MAP_CHANNELS[backbone], drop)
                   if nm.split(".")[1] in ("qkv", "proj", "fc1", "fc2"))
    if E in (32, 96, 160, 288):                                 # D % 128 != 0 and C % 128 != 0: no layer on the two-piece weight gradient
        assert not any(t.startswith(TNH2) for t in taken)
    model, _ = lifter_model(backbone, dtype=dtype, embed=E, wseed=61 + B + E)
    try:
        model.train(); model.backbone.eval(); model.volume_net.train()
        model.drop_path_rate = drop
        assert sum(1 for _ in model.volume_net.parameters()) == 191
        assert model.volume_net.Spatial_pos_embed.shape[-1] == E
        img, k2d, kc, gt = synth.synth_inputs(B, H, W, seed=62 + B + E, crop_range=(W, H) if (H, W) == (256, 256) else (192, 256), with_gt=True)
        masks = None
        if drop:
            torch.manual_seed(7)
            masks = model._drop_masks(B, torch.device("cuda"))
            assert (masks == 0).any() and masks.numel() == 2 * 4 * (B + 17 * B + B)
            model._drop_masks = lambda b, dev: masks             # the step below uses exactly these multipliers
        eng = model.engine_for(img.cuda())
        eng.set_debug(True)                                    # cidx / cpos taps of the deformable samplers
        assert [c for _, _, c in eng.feature_shapes()] == list(MAP_CHANNELS[backbone])
        pred, loss, ref = _step(model, img, k2d, kc, gt)
        # the library's own table against the restated rule; no table under bf16
        assert eng.lib.capf_train_h2_matrices(eng.h) == len(table) and (len(table) == 0) == (dtype == "bf16")
        tag = (f"{backbone} {dtype} E={E} {H}x{W} B={B} DropPath {drop} [{pipe}, table {len(table)}, "
               + ", ".join(sorted(t for t in taken if not t.endswith(" maps"))) + "]")
        check_cells_against_index_rule(eng, B, tag)
        (l2, mx), _ = _hold_to_yardstick(tag, model, eng, B, k2d, ref, gt, pred, loss, masks)
        print(f"  {_id(case)}: worst gradient {l2:.2e} relative L2, {mx:.2e} of max")
    finally:                                                   # (the training workspace grows with D^2: 3 GB at 288 -- freed before the next case)
        for e in model._engines.values():
            e.close()
        model._engines.clear()
        del model
        torch.cuda.empty_cache()


# what the cases cover together: a later edit of CASES cannot silently drop an instance
assert set().union(*(routes(c[0], c[1], c[2], c[4], c[5])[0] for c in CASES)) >= REACHABLE, \
    sorted(REACHABLE - set().union(*(routes(c[0], c[1], c[2], c[4], c[5])[0] for c in CASES)))
