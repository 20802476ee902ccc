"""No GPU: the groups of tests/test_feed_many_streams.py still cross what they exist for.  Every GPU id asserts its switch
from its own inputs and results; here the same numbers come from the lengths and the reference's records alone (the
reference runs on the D distinct streams of a group, not on its hundreds), so an edit of the signals that empties an id
fails here, on the machine where it is made."""
import numpy as np
import pytest

from oracle import ref
from tests import feed_many_cases as mc

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref is not built (the reference's sources were not there at build time)")


def test_the_distinct_streams():
    assert mc.D <= 24 and mc.D % 2 == 1 and 64 % mc.D and 1024 % mc.D
    from tests.decode_cases import END_COUNTS_9000
    from tests.synth_host import SHORT_LENGTHS
    assert set(SHORT_LENGTHS) <= set(mc.SHORT) and set(END_COUNTS_9000) <= set(mc.SHORT)
    assert any(n % 4 for n in END_COUNTS_9000)
    for g in (mc.short_group(), mc.uniform_group(), mc.bench_group()):
        assert len(g.distinct) == mc.D and g.index == [s % mc.D for s in range(g.count)]
        assert len({x.tobytes() for x in g.distinct}) == mc.D
        assert g.neighbours_differ()
        for stride in (64, 1024):                       # a wave's lanes, a workgroup's threads: never a copy of the same stream
            assert all(g.index[s] != g.index[s + stride] for s in range(g.count - stride))
    assert set(mc.KINDS) == {"noise", "gated", "sine", "clicks", "silence"} == set(mc.UNIFORM_KINDS) == set(mc.LONG_KINDS)


@pytest.mark.parametrize("which", ["a", "e", "f", "h"])
def test_the_short_group_crosses_its_switches(which):
    c = mc.conditions_of(which)
    assert c["ns"] > 1024
    assert c["ingest"] > 8192 * 256
    assert c["pass1"] > 65536 and c["pass2"] > 65536 and c["pass2"] == c["ns"] * 96
    assert min(c["group"].frames) == 1 and max(c["group"].frames) <= 10000
    assert all(len(r) >= 2 and r[-1][3] == 1 for r in c["group"].rows())


def test_the_uniform_group_crosses_its_switches():
    c = mc.conditions_of("b")
    assert len(set(c["group"].frames)) == 1 and c["group"].frames[0] % 4
    assert c["steps1"] % 32 and c["steps1"] % 64
    assert c["ns"] > 1024 and c["ingest"] > 8192 * 256 and c["pass1"] > 65536 and c["pass2"] > 65536


def test_the_bench_group_crosses_its_switches():
    c = mc.conditions_of("c")
    assert c["pass1"] > 65536 and c["pass2"] <= 65536
    assert c["long"] > 2048 and c["short"] > 2048, (c["long"], c["short"])
    assert max(c["group"].frames) <= 47000


@pytest.mark.parametrize("which", sorted(mc.MANAGED_SETUPS))
def test_the_managed_groups_cross_their_switches(which):
    c = mc.conditions_of(which)
    assert c["slices"] >= 3 and c["most"] > 1024 and c["cut"], (c["slices"], c["most"], c["cut"])
    assert c["group"].neighbours_differ()
    assert max(c["group"].frames) <= 10000


def test_slices_of():
    # three streams of 3, 2048 and 5 packets in slices of 2048: the second is cut by the first edge, the third lies in slice 1
    assert mc.slices_of(np.array([0, 3, 2051, 2056]), 2048) == (2, 2, [1])
    assert mc.slices_of(np.array([0, 2048, 4096]), 2048) == (2, 1, [])
    assert mc.slices_of(np.array([0, 1] + list(range(3, 2051, 2))), 2048)[1] == 1025


@pytest.mark.parametrize("which", sorted(mc.MANAGED_SETUPS))
def test_the_owner_of_a_whole_slice(which):
    g = mc.owner_group(which)
    n = g.packets_of(mc.MANAGED_SETUPS[which][1])
    assert n[0] > 2048 and g.neighbours_differ()            # the first stream's packets fill slice 0 and go on behind its edge
    assert mc.slices_of(np.concatenate([[0], np.cumsum(n)]))[2] == [0]


@pytest.mark.parametrize("batch", [0, 1])
def test_the_live_cuts(batch):
    g = mc.live_group()
    frames = g.frames if batch == 0 else g.frames[::-1]
    cuts = mc.live_cuts(frames, batch)
    c = mc.live_conditions(frames, cuts)
    assert 3 <= c["rounds"] <= 4 and c["tiled"] > 65536
    assert c["fresh"] >= 1 and len(c["closing"]) >= 3 and c["empty"] and c["single"] and c["ragged"]
    assert g.neighbours_differ() and max(g.frames) <= 18000
    by_stream = {}
    for d, cut in zip(g.index if batch == 0 else g.index[::-1], cuts):      # the copies of one stream are cut differently
        by_stream.setdefault(d, set()).add(tuple(cut))
    assert all(len(v) >= 4 for d, v in by_stream.items() if len(g.distinct[d]) > 1), by_stream


def test_the_sweep_reaches_the_first_step_of_a_tile():
    g = mc.sweep_group()
    assert g.count * g.steps > 65536 and g.steps % 64                # a tiled launch, its last tile ragged
    assert all(a != b for a, b in zip(g.index, g.index[1:])) and len({o["pcm"].tobytes() for o in g.distinct}) == mc.D
    for d, o in enumerate(g.distinct):   # in every stream a burst begins, and one ends, on a tile's first step at the longest stretch
        begins, ends = mc.tile_starts_hit(o["marks"], o["steps"])
        assert begins and ends, (d, begins, ends)
