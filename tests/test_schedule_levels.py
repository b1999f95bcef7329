"""CPU: the dependency levels of the fork/join regions and the default stream schedule (plan-only handles, no GPU).

The conflicts are recomputed here from the ops' buffer slots; the engine's own levels are only what is checked.  The default
of capf_set_lanes is mode 3, as include/capf.h says: at batch 16..128 lanes 1 + 2 of every region with two or more lanes run
as a second grouped chain on a library-owned stream, outside that range everything stays on the caller's stream."""
import copy

import pytest

FUSE = 1          # capf_op_desc::kind of a fuse sum (a debug copy reports -1)


def _plan(backbone, dtype, flags=0):
    from capf import Engine
    from mvn.models import _native
    from mvn.utils.cfg import backbone_preset, config
    c = backbone_preset(copy.deepcopy(config), backbone)
    c.model.backbone.fix_weights = True
    return Engine(_native.make_capf_config(c, 256, 256, compute_dtype=dtype, plan_flags=flags), device=None)


def _regions(sched):
    regions = {}
    for i, (rg, lv, _, _, _) in enumerate(sched):
        if rg >= 0:
            assert lv >= 0, f"op {i} of region {rg} has no level"
            regions.setdefault(rg, []).append(i)
    return regions


def _conflicts(sched, a, b):
    """b precedes a in program order: read-after-write, write-after-write or write-after-read on a workspace buffer"""
    _, _, _, ra, wa = sched[a]
    _, _, _, rb, wb = sched[b]
    return (set(wb) & (set(ra) | set(wa))) or (set(rb) & set(wa))


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("backbone", ["hrnet_32", "hrnet_48", "cpn"])
def test_levels_respect_every_conflict_and_a_modules_sums_share_the_last_level(backbone, dtype):
    eng = _plan(backbone, dtype)
    sched = eng.op_schedule()
    kinds = [eng.op_describe(i).kind for i in range(len(sched))]
    sums = 0
    for rg, ops in _regions(sched).items():
        last = max(sched[i][1] for i in ops)
        for pos, a in enumerate(ops):
            la = sched[a][1]
            for b in ops[:pos]:
                if _conflicts(sched, a, b):
                    assert la > sched[b][1], f"{backbone} {dtype}: op {a} (level {la}) conflicts with op {b} (level {sched[b][1]})"
            # a fuse sum nothing in its region waits for goes out with the module's other sums, as one launch behind the layer's convs (early
            # sums on a stream of their own were measured slower: EXPERIMENTS R11.1)
            if kinds[a] == FUSE and not any(_conflicts(sched, c, a) for c in ops[pos + 1:]):
                assert la == last
                sums += 1
    if backbone != "cpn":
        assert sums == 2 + 4 * 3 + 2 * 4 + 1      # stage 2, stage 3, stage 4 (its last module keeps output 0)


@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_the_default_schedule_is_two_chains_from_batch_16_to_128(dtype):
    eng = _plan("hrnet_32", dtype)
    sched = eng.op_schedule()

    def expect(two):
        return [1 if two and rg >= 0 and ln in (1, 2) else 0 for rg, _, ln, _, _ in sched]

    for batch, two in ((1, False), (15, False), (16, True), (64, True), (128, True), (129, False), (256, False)):
        assert eng.op_stream_classes(batch) == expect(two), batch          # no set_lanes call: the handle's default
    eng.set_lanes(3)
    assert eng.op_stream_classes(64) == expect(True)
    assert 1 in expect(True)
    for mode in (0, 2):
        eng.set_lanes(mode)
        assert set(eng.op_stream_classes(64)) == {0}
    eng.set_lanes(1)                                                         # one side stream per lane
    assert eng.op_stream_classes(64) == [1 if rg >= 0 and ln > 0 else 0 for rg, _, ln, _, _ in sched]
