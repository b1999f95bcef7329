"""CPU: the table of tests/session_cases.py against the plan (Engine(cfg, device=None)): the ladders cross the route switches they are there
for, in both directions; every named switch is where the table says; prefix(n) ends behind a fork / join region inside the backbone; every
uint8 step's plan has the stem capf_forward_u8 needs.  tests/test_gpu_sessions.py executes the sessions.  When a routing threshold moves,
this file says which batch of which session to move with it."""
import pytest

import session_cases as sc
import small_geometry_cases as sg
from test_op_routes import _tool


@pytest.fixture(scope="module")
def plans():
    """{plan: plan-only engine} for every plan a session or a switch names"""
    tool = _tool()
    want = {sc.step_plan(x, st) for x in sc.SESSIONS for st in x.steps} | {v[0] for v in sc.SWITCHES.values()}
    engines = {p: tool._engine(*p) for p in sorted(want)}
    yield engines
    for e in engines.values():
        e.close()


def _kernels(eng, B):
    return tuple(k for _, k, _ in eng.op_table(B))


def _streams(eng, B):
    eng.set_lanes(3)                         # the default schedule
    return tuple(eng.op_stream_classes(B))


def _differs(eng, what, a, b):
    return (_kernels if what == "kernels" else _streams)(eng, a) != (_kernels if what == "kernels" else _streams)(eng, b)


def test_every_named_switch_is_where_the_table_says(plans):
    """the two batches of a switch are neighbours as far as the plan goes: what the switch names differs between them, and the side below
    runs what the batch below it runs too (so the switch is AT lo | hi and not further down)"""
    for name, (plan, lo, hi, what) in sc.SWITCHES.items():
        eng = plans[plan]
        assert _differs(eng, what, lo, hi), name
        assert hi - lo == 1 or not _differs(eng, what, lo, lo + 1) or not _differs(eng, what, hi - 1, hi), name
    # the two-chain window is 16 .. 128: some op is on the side chain inside it, none outside
    eng = plans[sc.F32]
    assert any(_streams(eng, 16)) and any(_streams(eng, 128)) and not any(_streams(eng, 15)) and not any(_streams(eng, 129))


def test_consecutive_ladder_steps_run_different_kernels_wherever_a_switch_lies_between(plans):
    for sid in sc.LADDERS:
        sess = sc.session(sid)
        eng = plans[sess.plan]
        n_crossings = 0
        for a, b in zip(sess.steps, sess.steps[1:]):
            for name, _ in sc.crossed(sess.plan, a.batch, b.batch):
                what = sc.SWITCHES[name][3]
                assert _differs(eng, what, a.batch, b.batch), (sid, a.batch, b.batch, name)
                n_crossings += 1
            if a.batch != b.batch:                                   # (the table's own claim: no two neighbours on the same routing)
                assert _differs(eng, "kernels", a.batch, b.batch) or _differs(eng, "streams", a.batch, b.batch), (sid, a.batch, b.batch)
        assert n_crossings >= len(sess.steps) - 2, (sid, n_crossings)
        assert len({st.batch for st in sess.steps}) < len(sess.steps), f"{sid}: no batch is visited twice"


def test_every_named_switch_is_crossed_in_both_directions():
    seen = set()
    for sess in sc.SESSIONS:
        runs = [st for st in sess.steps if st.kind in sc.INFERENCE + sc.TRAINING and sc.opt(st, "at") is None]
        for a, b in zip(runs, runs[1:]):
            seen.update(sc.crossed(sess.plan, a.batch, b.batch))
    missing = sorted((n, d) for n in sc.SWITCHES for d in ("up", "down") if (n, d) not in seen)
    assert not missing, missing


def test_the_ladders_are_large_after_small_and_small_after_large():
    for sid in sc.LADDERS:
        b = [st.batch for st in sc.session(sid).steps]
        assert any(x > y for x, y in zip(b, b[1:])) and any(x < y for x, y in zip(b, b[1:])), sid


def test_the_inference_batches_that_are_rows_are_on_the_side_the_row_claims(plans):
    rows = {(r[:5], r.batch): r for r in sg.ROWS}
    hits = 0
    for plan, B in sc.inference_batches():
        r = rows.get((plan, B))
        if r is not None:
            assert sg.prefixes_hold(set(_kernels(plans[plan], B)), r.expected_kernel_prefixes) == [], (plan, B)
            hits += 1
    assert hits >= 20, hits


def test_prefix_ends_behind_a_region_inside_the_backbone(plans):
    for sess in sc.SESSIONS:
        if not any(st.kind == "prefix" for st in sess.steps):
            continue
        eng = plans[sess.plan]
        n_ops = eng.lib.capf_num_ops(eng.h)
        descs = [eng.op_describe(i) for i in range(n_ops)]
        n, last = sc.prefix_ops(descs)
        n_backbone = sum(1 for d in descs if d.backbone)
        sched = eng.op_schedule()
        assert 0 < last < n < n_backbone
        region = sched[last][0]
        names = [name for name, _, _ in eng.op_table(1)]
        assert region >= 0 and names[n - 1] == "join" and last == n - 2      # op n - 1 is the join of the region `last` closes
        assert sched[n][0] != region                                # ... and op n is outside it
        members = [i for i, x in enumerate(sched) if x[0] == region]
        assert names[members[0] - 1] == "fork"
        assert len({sched[i][2] for i in members}) > 1              # more than one lane: a real fork
        assert any(d.backbone and d.kind in (0, 1) for d in descs[n:n_backbone])      # the maps are not finished


def test_every_u8_step_has_the_single_three_channel_stem(plans):
    n = 0
    for sess in sc.SESSIONS:
        for st in sess.steps:
            if st.kind not in sc.U8:
                continue
            eng = plans[sc.step_plan(sess, st)]
            descs = [eng.op_describe(i) for i in range(eng.lib.capf_num_ops(eng.h))]
            stems = [i for i, d in enumerate(descs) if d.kind == 0 and d.conv and d.backbone and d.Cin == 3]
            assert len(stems) == 1 and descs[stems[0]].in_dtype == 0, (sess.id, stems)
            kern = _kernels(eng, st.batch)[stems[0]]
            assert kern.startswith(("igemm_f32_stem_stream<", "igemm_f32_smallc<", "igemm_f32<")), kern      # Family::F32: the route Engine::begin requires
            assert sc.opt(st, "mode", 0) != 2 or st.batch % 2 == 0
            n += 1
    assert n >= 2


def test_the_table_is_well_formed():
    assert len({x.id for x in sc.SESSIONS}) == len(sc.SESSIONS)
    kinds = {st.kind for x in sc.SESSIONS for st in x.steps}
    assert kinds == set(sc.KINDS), sorted(set(sc.KINDS) - kinds)
    for x in sc.SESSIONS:
        trained = False
        for st in x.steps:
            assert (st.batch > 0) == (st.kind in sc.INFERENCE + sc.TRAINING + ("features", "prefix")), (x.id, st)
            if st.kind == "optim":
                assert trained or sc.opt(st, "grad") == "synthetic", (x.id, "optim before any gradient")
                assert sc.opt(st, "how") in ("torch", "fused")
            trained |= st.kind in sc.TRAINING
            if st.kind in sc.TRAINING or st.kind == "features":
                assert x.plan[3] != "fp16"                               # fp16 plans are inference only
            if st.kind in ("features", "train_features"):
                assert x.plan[3] == "fp32"                               # caller-supplied maps: fp32 plans only
    hows = {sc.opt(st, "how") for x in sc.SESSIONS for st in x.steps if st.kind == "optim"}
    assert hows == {"torch", "fused"}
    assert {sc.opt(st, "mode") for x in sc.SESSIONS for st in x.steps if st.kind == "set_lanes"} >= {0, 1, 3}
    assert any(sc.opt(st, "masks") for x in sc.SESSIONS for st in x.steps if st.kind == "train")
    assert sc.step_seed("forward", 24) != sc.step_seed("train", 24) and sc.step_seed("forward", 24) != sc.step_seed("forward", 5)
