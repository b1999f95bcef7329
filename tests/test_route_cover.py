"""CPU: every launch route a production plan can take has a layer-wise check.  The universe of route signatures (tests/route_cover_cases.py:
kernel name + launch shape of every backbone op of kind 0 - 3, over the production plans and batches 1 .. 64, 96, 128) is recomputed from the
plan (Engine(cfg, device=None)) and held against what the suite's whole-plan walks reach plus what the rows of route_cover_cases.ROWS name --
a row counts for the ops it names and no others.  A route change that makes a new signature fails here until the table is regenerated:

    python -c "import __graft_entry__ as g; g.build()" && python tools/route_cover.py

tests/test_gpu_route_cover.py walks the rows on the GPU."""
import importlib.util
import os

import pytest

import route_cover_cases as rc
import small_geometry_cases as sg
from conftest import ROOT


@pytest.fixture(scope="module")
def cover():
    spec = importlib.util.spec_from_file_location("route_cover", os.path.join(ROOT, "tools", "route_cover.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    skipped = []
    plans = tool.open_plans(rc.plans(), skipped.append)
    uni, ends = tool.universe(plans)
    seen, walked = tool.covered_by_existing(plans, ends)
    yield tool, plans, (uni, ends), seen, walked, skipped
    for p in plans.values():
        p.close()


def test_the_universe_is_the_production_matrix(cover):
    tool, plans, (uni, ends), seen, walked, skipped = cover
    # the one combination capf_create refuses: fp16 is an HRNet plan
    assert len(skipped) == 2 and all("'cpn'" in s and "fp16" in s and "CPN50 is not supported" in s for s in skipped), skipped
    assert sum(k[4] == "0" for k in plans) == 16 and len(plans) == 16 + len(rc.FLAGGED_PLANS)
    assert rc.BATCHES == tuple(range(1, 65)) + (96, 128)
    kernels = {rc.kernel_of(s) for s in uni}
    for prefix in ("igemm_f32<", "igemm_f32h2g<", "igemm_f32h2_group_ws", "igemm_f32x3_group_ws", "igemm_wino", "igemm_bf16<", "igemm_bf16_ws<",
                   "igemm_f16<", "igemm_f16_ws<", "bneck0_bf16<", "bneck1_f16<", "fuse_sum", "bilinear_resize", "maxpool3x3s2"):
        assert any(k.startswith(prefix) for k in kernels), prefix
    assert len({rc.plain(k) for k in uni}) > 1000
    # a signature that may split K is there at the smallest and at the largest of its batches, marked; any other signature once, unmarked
    for s, (lo, hi) in ends.items():
        assert rc.split_k_capable(s) and rc.at_batch(s, lo) in uni and rc.at_batch(s, hi) in uni and s not in uni
    assert all(rc.plain(k) in ends for k in uni if k != rc.plain(k)) and len(ends) > 100


def test_every_route_signature_has_a_layerwise_check(cover):
    tool, plans, (uni, ends), seen, walked, skipped = cover
    named = {s for r in rc.ROWS for _, s in r.ops}
    missing = [(s, uni[s][0]) for s in uni if s not in seen and s not in named and s not in rc.LEFT_OUT]
    assert missing == [], f"{len(missing)} route signatures no layer-wise walk reaches (python tools/route_cover.py), the first: {missing[:5]}"
    assert all(s in uni and reason for s, reason in rc.LEFT_OUT.items())


def test_every_plan_without_a_whole_plan_walk_has_its_batch_1_row(cover):
    tool, plans, (uni, ends), seen, walked, skipped = cover
    rows_at_1 = {r[:5] for r in rc.ROWS if r.batch == 1}
    for key, p in plans.items():
        if key not in walked and key[4] == "0":          # (a flagged plan's batch 1 runs the default plan's kernels on the default plan's shapes)
            assert key in rows_at_1, key


def test_the_rows_name_ops_of_their_plans_with_the_signatures_they_record(cover):
    tool, plans, (uni, ends), seen, walked, skipped = cover
    assert len({rc.row_id(r) for r in rc.ROWS}) == len(rc.ROWS)
    for r in rc.ROWS:
        assert r[:5] in plans and r.batch in rc.BATCHES and r.ops, rc.row_id(r)
        assert list(r.frames_to_check) == sg.frames_for(r.H, r.W, r.batch), rc.row_id(r)
        at = dict(plans[r[:5]].keys(r.batch, ends))
        for name, s in r.ops:
            assert at.get(name) == s, (rc.row_id(r), name, s, at.get(name))


def test_every_row_is_needed(cover):
    """a signature is named once, by one op of one row, and by no whole-plan walk: take any row out and
    test_every_route_signature_has_a_layerwise_check fails"""
    tool, plans, (uni, ends), seen, walked, skipped = cover
    named = [s for r in rc.ROWS for _, s in r.ops]
    assert len(set(named)) == len(named) and not set(named) & seen and set(named) <= set(uni)


def test_the_table_is_what_the_tool_writes(cover):
    tool, plans, (uni, ends), seen, walked, skipped = cover
    assert tool.greedy_cover(plans, uni, ends, seen, walked, lambda *_: None) == rc.ROWS
