"""CPU suite: the live feed's sequence for one stream -- stream ends, the detector from its carried state, the walk resumed
from its carried WalkState and the rebase after each piece (k_blockout.h, k_lpc.h, k_envelope.h compiled for the host) --
against the reference's application loop fed write_frames at a time, for streams cut into pieces at random."""
import numpy as np
import pytest

from tests import live_host


@pytest.fixture(scope="module")
def walker():
    return live_host.LiveWalk(live_host.build(), (256, 2048))


def signal(kind, frames, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(frames)
    if kind == "gated":
        x = (rng.random((2, frames)) - 0.5) * 2 * np.where((t % 6000) < 500, 0.5, 0.0005)
    elif kind == "sine":
        x = 0.5 * np.sin(0.05 * t)[None, :] * np.ones((2, 1)) + (rng.random((2, frames)) - 0.5) * 1e-3
    else:
        x = rng.random((2, frames)) - 0.5
    return np.ascontiguousarray(x, dtype=np.float32)


def cuts_for(rng, frames):
    """random piece lengths summing to `frames`, a 1-frame piece and an empty one among them"""
    points = set(int(p) for p in rng.integers(1, frames - 1, size=frames // 3000 + 2))
    p = int(rng.integers(1, frames - 1))
    points |= {p, p + 1}
    edges = [0] + sorted(points) + [frames]
    cuts = [b - a for a, b in zip(edges, edges[1:])]
    cuts.insert(int(rng.integers(0, len(cuts))), 0)
    return cuts


@pytest.mark.parametrize("write_frames", [1024, 777, 4096])
@pytest.mark.parametrize("kind,frames", [("gated", 30000), ("noise", 9000), ("sine", 12000), ("gated", 2500)])
def test_live_sequence_on_the_host_matches_the_reference(walker, write_frames, kind, frames):
    from oracle import ref
    from tests.emul.emul import Emul
    import vorbis_amd
    if not ref.available():
        pytest.skip("needs the reference build")
    x = signal(kind, frames, frames + write_frames)
    want = ref.RefEncoder(2, 44100, 0.4).encode_stream(x, write_frames=write_frames)
    em = Emul(vorbis_amd.default_setup_blob("44k_stereo_q4"))
    rng = np.random.default_rng(frames * 7 + write_frames)
    got = live_host.live_stream(em, walker, x, cuts_for(rng, frames), write_frames)
    assert len(got) == len(want), (len(got), len(want))
    for k, (g, b) in enumerate(zip(got, want)):
        kd = g["kind"]
        assert (kd & 1, (kd >> 1) & 1, (kd >> 2) & 1, (kd >> 3) & 1) == (b["W"], b["lW"], b["nW"], b["blocktype"]), k
        assert (g["granulepos"], g["eos"]) == (b["granulepos"], b["eos"]), k
        assert np.array_equal(g["pcm"].view(np.uint32), b["pcm"].view(np.uint32)), "block %d of %d: samples differ" % (k, len(want))
    assert want[-1]["eos"] == 1


@pytest.mark.parametrize("kind,frames", [("gated", 30000), ("noise", 7000)])
def test_resumed_walk_from_a_fresh_state_is_the_whole_stream_walk(walker, kind, frames):
    """One piece that closes the stream: the live sequence is vamd_plan_streams_whole's (tests/emul's whole_stream)."""
    from tests.emul.emul import Emul
    import vorbis_amd
    x = signal(kind, frames, 3)
    em = Emul(vorbis_amd.default_setup_blob("44k_stereo_q4"))
    buf, kinds, begins = em.whole_stream(x)
    got = live_host.live_stream(em, walker, x, [frames], 1024)
    assert [g["kind"] for g in got] == [int(k) for k in kinds]
    assert [g["begin"] for g in got] == [int(b) for b in begins]
