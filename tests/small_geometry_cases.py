"""The small-map and odd-geometry plans the suite holds to the oracle ON THE GPU (tests/test_gpu_small_geometry.py), and whose routes
tests/test_small_geometry_routes.py pins on the CPU plan: one table, plain data plus the helpers that made it.

capf_create accepts any crop whose height and width are multiples of 32.  Which kernel runs a conv is a function of map size and batch
(Engine::gemm_family, tile_takes, fused_at, gemm_f32_route), so every geometry has its own batches at which a route moves.  A row is

    (backbone, H, W, dtype, plan_flags, batch, frames_to_check, expected_kernel_prefixes)

* plan_flags: tools/dump_op_routes.py's spelling ("0", or CAPF_PLAN_ names without the prefix joined with "|").
* batch: on one side of a route switch of that plan; every switch has a row on either side.  The batches were read off the CPU plan
  (Engine(cfg, device=None).op_table(B)), and test_small_geometry_routes.py asserts the side from the plan again.  A batch on the side
  where the split-fp32 tile (256 output pixels of a flattened [B * H * W] row space) has taken the level is no multiple of the frames one
  tile holds on any branch (83, 161, 317, ...): the last tile of every branch is ragged.
* frames_to_check: frame 0, the last frame, a frame inside the ragged last tile of the two smallest branches -- and, where a map of the
  plan is smaller than 4 x 4, at least 8 frames (all of them below batch 8), so that every compared tensor has 2048 or more elements and
  op_oracle.compare's "at most 3 % inexact" stays a statistic.  The first four are the ones the end-to-end comparison runs the CPU oracle on.
* expected_kernel_prefixes: every entry is the beginning of a kernel name the plan must run at that batch; "!" in front: of none.
  Backbone kernels only, so that the layer-wise walker's set can be held to them as well."""
import collections

Row = collections.namedtuple("Row", "backbone H W dtype plan_flags batch frames_to_check expected_kernel_prefixes")

TILE_PIXELS = 256      # output pixels of one split-fp32 tile (csrc/igemm_f32h2_ws_tile.h)
E2E_FRAMES = 4         # the CPU oracle costs ~0.7 s a frame


def branch_maps(H, W):
    """the four map sizes of a plan: strides 4, 8, 16, 32 (HRNet's branches, ResNet-50's stages under CPN)"""
    return [(H >> s, W >> s) for s in (2, 3, 4, 5)]


def frames_for(H, W, B):
    maps = branch_maps(H, W)
    tiny = min(h * w for h, w in maps) < 16
    want = 8 if tiny else 4
    if B <= want:
        return list(range(B))
    picks = [0, B - 1]
    for h, w in reversed(maps):                                  # smallest map first: the most frames per tile
        total = B * h * w
        if total > TILE_PIXELS and total % TILE_PIXELS:
            start = (total - 1) // TILE_PIXELS * TILE_PIXELS     # first pixel of the ragged last tile
            f = ((start + total) // 2) // (h * w)
            if f not in picks and len(picks) < 4:
                picks.append(f)
    k = 1
    while len(picks) < want:                                     # spread the rest over the batch
        f = (k * B) // (want + 1)
        if f not in picks:
            picks.append(f)
        k += 1
    return picks


# ---- what a side of a switch runs, as prefixes ---------------------------------------------------------------------------------------
FP32_PIPE = ("igemm_f32<", "!igemm_f32h2g", "!igemm_f32h2_group_ws", "!igemm_wino")                    # batch < 5: the fp32 matrix pipe
TWO_PIECE = ("igemm_f32h2g<", "!igemm_f32h2_group_ws", "!igemm_wino")                                  # 5 ..: the two-piece GEMM
TWO_PIECE_TILE = ("igemm_f32h2g<", "igemm_f32h2_group_ws", "!igemm_wino")                              # ... and the tile on the largest convs
WINO_MIXED = ("igemm_wino43_group", "igemm_wino<w4,F(2,3)>", "igemm_f32h2g<")                          # 24 ..: F(4,3) group + lone F(2,3) + two-piece
WINO_MIXED_TILE = WINO_MIXED + ("igemm_f32h2_group_ws",)
WINO43_TILE = ("igemm_wino43_group", "igemm_f32h2_group_ws", "igemm_f32h2g<", "!igemm_wino<")          # 32 x 1056: F(4,3) on branch 0 only
TILE_ALL = ("igemm_f32h2_group_ws", "igemm_f32h2g<", "!igemm_wino")                                    # the tile took every eligible conv
CPN_PIPE = ("igemm_f32<", "igemm_f32_smallc<", "bilinear_resize", "maxpool3x3s2", "!igemm_f32h2g", "!igemm_wino")
CPN_TWO_PIECE = ("igemm_f32h2g<", "bilinear_resize", "!igemm_wino", "!igemm_f32h2_group_ws")
CPN_WINO23 = ("igemm_f32h2g<", "igemm_wino<w4,F(2,3)>", "bilinear_resize", "!igemm_wino43")


def _b16(t, tile=None, bneck=False):
    out = [f"igemm_{t}<", f"igemm_{t}_stem_stream<"]
    out.append(f"igemm_{t}_ws<{tile}" if tile else f"!igemm_{t}_ws<")
    out += [f"bneck0_{t}<8x8>", f"bneck1_{t}<8x8>"] if bneck else [f"!bneck0_{t}", f"!bneck1_{t}"]
    return tuple(out)


_PLANS = [
    # HRNet-32 fp32 64 x 64 (maps 16^2, 8^2, 4^2, 2^2): 4 | 5 two-piece GEMM, 23 | 24 Winograd (one F(4,3) group, a lone F(2,3) conv at W = 2,
    # two-piece GEMMs), 78 | 79 the tile takes all 213 convs (a tile spans 64 frames of the 2 x 2 branch); 1, 64, 128, 512: the other tile
    # shapes tests/golden/op_routes_small.npz pins
    ("hrnet_32", 64, 64, "fp32", "0", [(1, FP32_PIPE), (4, FP32_PIPE), (5, TWO_PIECE), (23, TWO_PIECE_TILE), (24, WINO_MIXED_TILE),
                                       (64, WINO_MIXED_TILE + ("igemm_f32h2g<128x64,conv>",)), (78, WINO_MIXED_TILE), (83, TILE_ALL),
                                       (128, TILE_ALL + ("igemm_f32<w4,128x128,conv>",)), (317, TILE_ALL + ("igemm_f32_pw<",)),
                                       (512, TILE_ALL + ("igemm_f32_pw<",))]),
    # 96 x 96 (24^2 .. 3^2): the W = 3 branch is odd -- never Winograd or tile, two-piece GEMM inside a grouped level; the tile from 35
    ("hrnet_32", 96, 96, "fp32", "0", [(1, FP32_PIPE), (4, FP32_PIPE), (5, TWO_PIECE_TILE), (23, TWO_PIECE_TILE), (24, WINO_MIXED_TILE),
                                       (34, WINO_MIXED_TILE), (37, TILE_ALL),
                                       (48, TILE_ALL + ("igemm_f32<w4,128x128,conv>",)), (512, TILE_ALL + ("igemm_f32_pw<",))]),
    # 32 x 32 (8^2 .. 1 x 1): the samplers divide by size - 1 = 0 on the top map; the tile takes 189 convs from 314 (never the 1 x 1 branch)
    ("hrnet_32", 32, 32, "fp32", "0", [(23, TWO_PIECE), (24, WINO_MIXED + ("!igemm_f32h2_group_ws",)), (313, WINO_MIXED_TILE), (317, TILE_ALL)]),
    # non-square, top map 1 x 2 / 2 x 1
    ("hrnet_32", 32, 64, "fp32", "0", [(23, TWO_PIECE_TILE), (24, WINO_MIXED_TILE), (156, WINO_MIXED_TILE), (161, TILE_ALL)]),
    ("hrnet_32", 64, 32, "fp32", "0", [(23, TWO_PIECE_TILE), (24, WINO_MIXED_TILE), (156, WINO_MIXED_TILE), (161, TILE_ALL)]),
    # 160 x 96 (40 x 24 .. 5 x 3): odd top map; the tile takes 1 conv at 5, 5 at 6, 189 at 21
    ("hrnet_32", 160, 96, "fp32", "0", [(4, FP32_PIPE), (5, TWO_PIECE_TILE), (6, TWO_PIECE_TILE), (20, TWO_PIECE_TILE), (23, TILE_ALL)]),
    # 32 x 1056: branch 0 is 8 x 264, wider than the tile's 256 -- no tile pack, Winograd F(4,3) from 24 while 120 other convs run the tile
    # from 10 in the same levels
    ("hrnet_32", 32, 1056, "fp32", "0", [(9, TWO_PIECE), (11, TWO_PIECE_TILE), (23, TWO_PIECE_TILE), (24, WINO43_TILE)]),
    # HRNet-48: the 48-channel branch is not Winograd-eligible; the tile takes 4 convs at 14, 124 at 24
    ("hrnet_48", 64, 96, "fp32", "0", [(13, TWO_PIECE), (17, TWO_PIECE_TILE), (23, TWO_PIECE_TILE), (29, TWO_PIECE_TILE)]),
    # CPN: refineNet resizes 1 x 1 .. 8 x 8 maps to the fixed 64 x 48 (bilinear_rows_kernel, Ho > 2 H with H = 1)
    ("cpn", 32, 32, "fp32", "0", [(1, CPN_PIPE), (2, CPN_PIPE), (4, CPN_PIPE), (5, CPN_TWO_PIECE), (23, CPN_TWO_PIECE), (24, CPN_WINO23)]),
    ("cpn", 64, 96, "fp32", "0", [(1, CPN_PIPE), (2, CPN_PIPE), (4, CPN_PIPE), (5, CPN_TWO_PIECE),
                                  (23, ("igemm_f32h2g<", "igemm_f32h2_group_ws", "bilinear_resize", "!igemm_wino")), (24, ("igemm_f32h2g<", "igemm_f32h2_group_ws", "igemm_wino<w4,F(2,3)>", "bilinear_resize"))]),
    # 16-bit, HRNet-32 64 x 64: the 2-D halo tile takes 1 conv at 27, 5 at 53, all 213 at 212; the fused bottlenecks start at 256 (64 Ki pixels)
    ("hrnet_32", 64, 64, "bf16", "0", [(26, _b16("bf16")), (29, _b16("bf16", tile="w4,256x32")), (52, _b16("bf16", tile="w4,256x32")),
                                       (53, _b16("bf16", tile="w4,256x64")),                                       (60, _b16("bf16", tile="w4,256x64")), (211, _b16("bf16", tile="w4,256x")), (223, _b16("bf16", tile="w4,256x")),
                                       (255, _b16("bf16", tile="w4,256x")),
                                       (257, _b16("bf16", tile="w4,256x", bneck=True))]),
    ("hrnet_32", 64, 64, "fp16", "0", [(26, _b16("f16")), (29, _b16("f16", tile="w4,256x32")), (52, _b16("f16", tile="w4,256x32")),
                                       (53, _b16("f16", tile="w4,256x64")), (211, _b16("f16", tile="w4,256x")),                                       (223, _b16("f16", tile="w4,256x")), (255, _b16("f16", tile="w4,256x")),
                                       (257, _b16("f16", tile="w4,256x", bneck=True))]),
    ("hrnet_32", 64, 64, "bf16", "BF16_F32_STREAM", [(53, ("igemm_bf16<", "igemm_bf16_ws<"))]),
    # HRNet-32 bf16 128 x 128, the row tests/golden/op_routes_16bit.npz pins: 23 | 24, 52 | 53, the bottlenecks at 64
    ("hrnet_32", 128, 128, "bf16", "0", [(23, _b16("bf16")), (24, _b16("bf16", tile="w4,256x")), (32, _b16("bf16", tile="w4,256x")),
                                         (52, _b16("bf16", tile="w4,256x")),                                         (53, _b16("bf16", tile="w4,256x")), (64, _b16("bf16", tile="w4,256x", bneck=True))]),
    # CPN bf16: the tile at 36 (64 x 96); the bottlenecks at 86 (128 x 96)
    ("cpn", 64, 96, "bf16", "0", [(35, _b16("bf16") + ("bilinear_resize",)), (37, _b16("bf16", tile="w4,256x64") + ("bilinear_resize",))]),
    ("cpn", 128, 96, "bf16", "0", [(85, _b16("bf16", tile="w4,256x64")), (89, _b16("bf16", tile="w4,256x64", bneck=True))]),
]

ROWS = [Row(bb, H, W, dt, fl, B, tuple(frames_for(H, W, B)), tuple(pre)) for bb, H, W, dt, fl, sides in _PLANS for B, pre in sides]


def row_id(r):
    return f"{r.backbone}-{r.H}x{r.W}-{r.dtype}{'' if r.plan_flags == '0' else '-' + r.plan_flags}-B{r.batch}"


def plans():
    """[(backbone, H, W, dtype, plan_flags)] in table order, each once"""
    seen = []
    for r in ROWS:
        if r[:5] not in seen:
            seen.append(r[:5])
    return seen


def flag_bits(spec):
    from capf import lib
    return 0 if spec == "0" else sum(getattr(lib, "PLAN_" + f) for f in spec.split("|"))


def prefixes_hold(kernels, prefixes):
    """the expected_kernel_prefixes that a set of kernel names does NOT meet (empty: the row is on the side it claims)"""
    bad = []
    for p in prefixes:
        hit = any(k.startswith(p.lstrip("!")) for k in kernels)
        if hit == p.startswith("!"):
            bad.append(p)
    return bad


# ---- the other lists of tests/test_gpu_small_geometry.py -------------------------------------------------------------------------------
# the lifter op by op, on the geometries whose top map is 1 x 1, 1 x 2, 5 x 3 and CPN's: (backbone, H, W, batch)
LIFTER_FP32 = [("hrnet_32", 32, 32, 9), ("hrnet_32", 32, 64, 6), ("hrnet_32", 160, 96, 5), ("cpn", 32, 32, 7)]
# ... and the 16-bit lifter: (backbone, H, W, batch, dtype)
LIFTER_16BIT = [("hrnet_32", 32, 32, 9, "bf16"), ("hrnet_32", 32, 64, 8, "fp16"), ("hrnet_32", 160, 96, 5, "bf16"), ("cpn", 32, 32, 8, "bf16")]
# the levels whose grouped lists mix kernel families: capf_set_lanes 0 / 2 / 3 must give the same bits
SCHEDULES = [("hrnet_32", 64, 64, "fp32", 24), ("hrnet_32", 96, 96, "fp32", 24), ("hrnet_32", 32, 1056, "fp32", 24), ("hrnet_32", 64, 64, "bf16", 60)]
# training through tiny maps (8 x 16 .. 1 x 2: on the top map every sample of every joint collides): (backbone, (H, W), batch, map-grad mode)
TRAIN_TINY = [("hrnet_32", (32, 64), 2, 0), ("hrnet_32", (32, 64), 2, 1), ("hrnet_32", (32, 64), 6, 0), ("hrnet_32", (32, 64), 6, 1)]
