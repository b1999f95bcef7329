"""CPU: the table of tests/small_geometry_cases.py against the plan (Engine(cfg, device=None).op_table(B)): every row is on the side of
its route switch that it claims, the rows together run every kernel name the route fixtures pin for the small-map plans, and the table
holds the geometries it is there for.  tests/test_gpu_small_geometry.py executes the rows."""
import pytest

import small_geometry_cases as sg
from conftest import load_golden
from test_op_routes import _tool


@pytest.fixture(scope="module")
def kernel_sets():
    """{row: the kernel name of every op of its plan at its batch}"""
    tool = _tool()
    out = {}
    for bb, H, W, dt, fl in sg.plans():
        eng = tool._engine(bb, H, W, dt, fl)
        for r in sg.ROWS:
            if r[:5] == (bb, H, W, dt, fl):
                out[r] = [k for _, k, _ in eng.op_table(r.batch)]
        eng.close()
    return out


def test_every_row_is_on_the_side_of_the_switch_it_claims(kernel_sets):
    assert len(set(sg.row_id(r) for r in sg.ROWS)) == len(sg.ROWS)
    for r in sg.ROWS:
        assert sg.prefixes_hold(set(kernel_sets[r]), r.expected_kernel_prefixes) == [], (sg.row_id(r), sorted(set(kernel_sets[r])))


def test_the_rows_of_a_plan_are_on_different_sides(kernel_sets):
    """per plan: ascending batches, and at least as many different routings (the kernel of every op, in order) as sides the rows claim"""
    for plan in sg.plans():
        rows = [r for r in sg.ROWS if r[:5] == plan]
        assert all(a.batch < b.batch for a, b in zip(rows, rows[1:])), plan
        claimed = {r.expected_kernel_prefixes for r in rows}
        routed = {tuple(kernel_sets[r]) for r in rows}
        assert len(routed) >= len(claimed) and (len(rows) == 1 or len(routed) >= 2), (plan, len(routed), len(claimed))


def _fixture_names(g, key, limit=None):
    batches = list(g[key + ".batches"]) if key + ".batches" in g.files else list(g["batches"])
    strings, kern = g["strings"], g[key + ".kernel"]
    return set().union(*(set(strings[kern[i]]) for i, b in enumerate(batches) if limit is None or b <= limit)) - {""}


def test_the_table_runs_what_the_route_fixtures_pin(kernel_sets):
    small, wide = load_golden("op_routes_small"), load_golden("op_routes_16bit")
    for g, key, plan, limit in ((small, "hrnet_32_64x64_fp32_0", ("hrnet_32", 64, 64, "fp32", "0"), None),
                                (small, "hrnet_32_96x96_fp32_0", ("hrnet_32", 96, 96, "fp32", "0"), None),
                                (wide, "hrnet_32_128x128_bf16_0", ("hrnet_32", 128, 128, "bf16", "0"), 64)):
        pinned = _fixture_names(g, key, limit)
        run = set().union(*(set(k) for r, k in kernel_sets.items() if r[:5] == plan))
        assert len(pinned) > 10 and pinned <= run, (key, sorted(pinned - run))


def test_the_table_holds_the_geometries_it_is_there_for():
    tool = _tool()
    maps = {p: sg.branch_maps(p[1], p[2]) for p in sg.plans()}
    assert any((1, 1) in m for p, m in maps.items() if p[0] != "cpn")                    # a 1 x 1 map: the samplers' size - 1 = 0
    assert any(w % 2 == 1 and w > 1 for m in maps.values() for _, w in m)                # an odd width: never Winograd or tile
    assert any(m[0][1] > 256 for m in maps.values())                                     # branch 0 wider than the split-fp32 tile's 256
    # ... and a CPN plan whose resize source is 1 x 1, from the plan's own descriptors
    cpn = [p for p in sg.plans() if p[0] == "cpn" and (1, 1) in maps[p]]
    assert cpn
    eng = tool._engine(*cpn[0])
    descs = [eng.op_describe(i) for i in range(eng.lib.capf_num_ops(eng.h))]
    eng.close()
    assert any(d.backbone and d.kind == 3 and (d.H, d.W) == (1, 1) and d.Ho > 2 * d.H for d in descs)


def test_frames_to_check():
    for r in sg.ROWS:
        f, B = r.frames_to_check, r.batch
        assert 0 in f and B - 1 in f and len(set(f)) == len(f) and all(0 <= x < B for x in f), sg.row_id(r)
        tiny = min(h * w for h, w in sg.branch_maps(r.H, r.W)) < 16
        assert len(f) >= min(B, 8 if tiny else 4), sg.row_id(r)
        if {"igemm_f32h2_group_ws", "!igemm_wino"} <= set(r.expected_kernel_prefixes) and B > 64 and B not in (128, 512):
            # the side where the split-fp32 tile has taken every level (128 and 512 are the route fixture's own batches, kept for its kernel names): no branch has a whole
            # number of 256-pixel tiles, and a checked frame other than the last lies in the ragged last tile of a branch
            hit = False
            for h, w in sg.branch_maps(r.H, r.W):
                if 256 % (h * w) == 0 and h * w < 256:
                    per = 256 // (h * w)
                    assert B % per != 0, (sg.row_id(r), h, w)
                    hit |= any(B // per * per <= x < B - 1 for x in f)
            assert hit, sg.row_id(r)
