"""GPU suite: the live feed (vamd_feed_create_live / vamd_feed_wrote_live, include/vorbis_amd.h) -- continuing streams fed
in pieces, their state kept on the device between groups -- against the reference's application loop over the same
samples written `write_frames` at a time and closed with vorbis_analysis_wrote(v, 0): every packet's bytes, granule
position, size class and end-of-stream flag, over all of a stream's groups."""
import numpy as np
import pytest

from tests import bitrate_host as bh
from tests import checker
from tests.feed_cases import diff, record_rows as reference, run_live, small_arena, spy_totals
from tests.signals import mixed_streams, random_cuts, s16_streams

pytestmark = pytest.mark.gpu

def _ref():
    from oracle import ref
    if not ref.available():
        pytest.skip("needs the reference build")
    return ref


@pytest.mark.parametrize("setup", ["44k_stereo_q4", "44k_stereo_q9", "44k_mono_q5"])
@pytest.mark.parametrize("fmt", ["s16", "f32"])
def test_random_cuts_match_the_reference(setup, fmt):
    import vorbis_amd
    ref = _ref()
    ch, rate, q = checker.SETUPS[setup]
    rng = np.random.default_rng(7 + ch)
    streams, cuts = mixed_streams(rng, ch)
    feed_in = streams if fmt == "s16" else [(x.astype(np.float32) / np.float32(32768.0)) for x in streams]
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob(setup), lanes_per_device=1, max_streams=8, max_frames=32000,
                           fmt=vorbis_amd.FEED_S16 if fmt == "s16" else vorbis_amd.FEED_F32, write_frames=1024)
    got = run_live(feed, feed_in, cuts)
    feed.close()
    bad = []
    for s, x in enumerate(streams):
        bad += diff(reference(ref.RefEncoder(ch, rate, q), x), got[s], s)
    assert not bad, "\n".join(bad)
    assert all(g[-1][3] == 1 for g in got)


def test_two_cuts_agree_and_equal_the_whole_stream_feed():
    import vorbis_amd
    rng = np.random.default_rng(11)
    streams = [s16_streams(rng, 2, n, [k])[0] for n, k in [(40000, "gated"), (12345, "noise"), (700, "sine")]]
    blob = vorbis_amd.default_setup_blob("44k_stereo_q4")
    feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=4, max_frames=40000, write_frames=1024)
    a = run_live(feed, streams, [random_cuts(rng, len(x)) for x in streams])
    b = run_live(feed, streams, [[len(x) // 3, 0, len(x) - len(x) // 3] for x in streams])
    feed.close()
    whole = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=4, max_frames=40000)
    w = whole.encode(list(streams))
    whole.close()
    assert a == b
    assert a == w


@pytest.mark.parametrize("write_frames", [777, 4096])
def test_cadence_matches_the_reference_at_that_cadence(write_frames):
    import vorbis_amd
    ref = _ref()
    rng = np.random.default_rng(write_frames)
    streams = [s16_streams(rng, 2, n, [k])[0] for n, k in [(20000, "gated"), (3000, "noise"), (4500, "clicks"), (9999, "sine")]]
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_stereo_q4"), lanes_per_device=1, max_streams=4, max_frames=20000,
                           write_frames=write_frames)
    n_head = (2048 // write_frames + 1) * write_frames
    got = run_live(feed, streams, [random_cuts(rng, len(x), [n_head]) for x in streams])
    feed.close()
    bad = []
    for s, x in enumerate(streams):
        bad += diff(reference(ref.RefEncoder(2, 44100, 0.4), x, write_frames), got[s], s)
    assert not bad, "\n".join(bad)


def test_cadence_over_the_lds_bound_is_refused():
    import vorbis_amd
    with pytest.raises(vorbis_amd.VamdError) as e:
        vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_stereo_q4"), lanes_per_device=1, max_streams=2, max_frames=4096,
                        write_frames=1 << 20)
    assert "write_frames" in str(e.value)


@pytest.mark.parametrize("slice_", [None, "5"])
@pytest.mark.parametrize("name,ch,rates,kind,lengths,arena",
                         [bh.CONFIGS[0] + ([26000, 9000, 2000], None), bh.CONFIGS[2] + ([26000, 9000, 2000], None),
                          bh.CONFIGS[3] + ([26000, 9000, 2000], None), bh.CONFIGS[0] + ([90000, 60000, 2000], "4096")],
                         ids=["abr", "cbr", "minmax", "abr-arena4096"])
def test_managed_in_pieces(name, ch, rates, kind, lengths, arena, slice_, monkeypatch):
    """arena: the lane's packet arena starts at 4096 bytes (VAMD_FEED_OUT_BYTES) and the streams are long enough for a
    group's packets to outgrow it (between its slices, where it has several)."""
    import vorbis_amd
    ref = _ref()
    if slice_:
        monkeypatch.setenv("VAMD_TEST_KNOBS", "1")
        monkeypatch.setenv("VAMD_FEED_SLICE", slice_)
    small_arena(monkeypatch, arena)
    rng = np.random.default_rng(3)
    streams = [np.clip(np.round(bh.signal(kind, ch, n, 40 + i).T * 32768.0), -32768, 32767).astype(np.int16)
               for i, n in enumerate(lengths)]
    feed = vorbis_amd.Feed(bh.managed_blob(ch, rates), lanes_per_device=1, max_streams=4, max_frames=max(lengths), write_frames=1024)
    totals = spy_totals(feed)
    got = run_live(feed, streams, [random_cuts(rng, len(x)) for x in streams])
    feed.close()
    assert not arena or max(totals) > 4096, totals
    bad = []
    for s, x in enumerate(streams):
        bad += diff(reference(ref.RefEncoder(ch, 44100, managed=rates), x), got[s], s)
    assert not bad, "\n".join(bad)


def test_past_the_whole_stream_cap():
    """A mono 44.1 kHz stream of 11 M frames (about 250 s, past the whole-stream feed's length cap) in 1 s pieces."""
    import vorbis_amd
    ref = _ref()
    frames, sec = 11_000_000, 44100
    rng = np.random.default_rng(250)
    t = np.arange(frames)
    x = (rng.random(frames) - 0.5) * np.where((t % 44100) < 9000, 0.6, 0.01) + 0.3 * np.sin(2 * np.pi * 220.0 / 44100.0 * t)
    x = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)[:, None]
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_mono_q5"), lanes_per_device=1, max_streams=1, max_frames=sec,
                           write_frames=1024)
    got = []
    for a in range(0, frames, sec):
        got += feed.encode_live([x[a:a + sec]], [a + sec >= frames])[0]
    feed.close()
    ch, rate, q = checker.SETUPS["44k_mono_q5"]
    bad = diff(reference(ref.RefEncoder(ch, rate, q), x), got)
    assert not bad, "\n".join(bad)
    assert len(got) > 10_000 and got[-1][3] == 1


def test_slot_reuse_and_lanes_over_a_device_named_twice():
    """After a close the slot's next piece is a fresh stream; three lanes per device entry with pieces of each lane's
    streams in flight together, over one GPU named twice."""
    import vorbis_amd
    ref = _ref()
    rng = np.random.default_rng(99)
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_stereo_q4"), devices=[0, 0], lanes_per_device=3, max_streams=2,
                           max_frames=6000, write_frames=1024)
    assert feed.lanes == 6
    # per lane: in stream slot 0 two streams one after the other (the second starts with the piece after the first's close),
    # in slot 1 one stream
    plan = {}
    for lane in range(6):
        a, b, c = (s16_streams(rng, 2, n, [k])[0] for n, k in [(9000, "gated"), (7000, "noise"), (15000, "sine")])
        plan[lane] = {"streams": [[a, b], [c]], "pos": [0, 0], "cur": [0, 0], "got": [[[], []], [[]]]}

    def collect(sl, cur):
        rows = vorbis_amd.Feed._rows(feed.packets(sl), 2)
        feed.release(sl)
        for s in range(2):
            if cur[s] < len(plan[sl]["streams"][s]):
                plan[sl]["got"][s][cur[s]] += rows[s]

    pending = []
    for _ in range(6 * 8):
        slot, buf = feed.buffer(2)
        P = plan[slot]
        frames, close, flat = [], [], []
        for s in range(2):
            seq = P["streams"][s]
            if P["cur"][s] >= len(seq):
                frames.append(0)
                close.append(0)
                continue
            x = seq[P["cur"][s]]
            n = min(int(rng.integers(0, 6001)), len(x) - P["pos"][s])
            flat.append(x[P["pos"][s]:P["pos"][s] + n].reshape(-1))
            P["pos"][s] += n
            frames.append(n)
            close.append(int(P["pos"][s] == len(x)))
        f = np.concatenate(flat) if flat else np.zeros(0, np.int16)
        buf[:f.size] = f
        feed.wrote_live(slot, frames, close)
        pending.append((slot, list(P["cur"])))
        for s in range(2):
            if close[s]:
                P["cur"][s] += 1
                P["pos"][s] = 0
        if len(pending) == 4:
            collect(*pending.pop(0))
    for sl, cur in pending:
        collect(sl, cur)
    feed.close()
    bad, done = [], 0
    for lane, P in plan.items():
        for s in range(2):
            for i, x in enumerate(P["streams"][s]):
                if i < P["cur"][s]:  # (the streams that were closed)
                    bad += diff(reference(ref.RefEncoder(2, 44100, 0.4), x), P["got"][s][i], 10 * lane + s)
                    done += 1
    assert not bad, "\n".join(bad)
    assert done >= 12


def test_non_finite_sample_ends_its_stream_only():
    import vorbis_amd
    ref = _ref()
    rng = np.random.default_rng(5)
    streams = [s16_streams(rng, 2, 30000, [k])[0].astype(np.float32) / np.float32(32768.0) for k in ["gated", "noise", "sine"]]
    nan_at = 17001
    poisoned = streams[1].copy()
    poisoned[nan_at, 1] = np.nan
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_stereo_q4"), lanes_per_device=1, max_streams=4, max_frames=8000,
                           fmt=vorbis_amd.FEED_F32, write_frames=1024)
    cuts = [5000, 6000, 7000, 8000, 4000]
    got = [[], [], []]  # (packet tuple, info)
    pos = 0
    for r, n in enumerate(cuts):
        slot, buf = feed.buffer(2)
        flat = np.concatenate([x[pos:pos + n].reshape(-1) for x in (streams[0], poisoned, streams[2])])
        buf[:flat.size] = flat
        feed.wrote_live(slot, [n] * 3, [r == len(cuts) - 1] * 3)
        res = feed.packets(slot)
        for s, row in enumerate(vorbis_amd.Feed._rows(res, 3)):
            k0 = int(res["stream_start"][s])
            got[s] += [(g, int(res["info"][k0 + j])) for j, g in enumerate(row)]
        feed.release(slot)
        pos += n
    # the lane's next streams are unaffected
    later = s16_streams(rng, 2, 8000, ["gated"])[0].astype(np.float32) / np.float32(32768.0)
    after = feed.encode_live([later, later, later], [1, 1, 1])
    feed.close()
    want = [reference(ref.RefEncoder(2, 44100, 0.4), x) for x in streams]
    for s in (0, 2):
        assert not diff(want[s], [g for g, _ in got[s]], s)
    head, sample = 1024, nan_at + 1024  # (positions with the head room: granulepos = centre - head on all but the last block)
    held = 0
    for k, (g, info) in enumerate(got[1]):
        half = (2048 if g[2] else 256) // 2
        if g[3]:
            assert g[0] is None
            continue
        end = g[1] + head + half
        if end + 2 * 2048 <= sample:
            assert g == want[1][k], "packet %d, well before the non-finite sample, differs from the reference's" % k
        if end > sample:
            assert g[0] is None and (info >> 2) & 3 == 2, "packet %d holds the non-finite sample or follows it" % k
            held += 1
    assert held > 5
    wl = reference(ref.RefEncoder(2, 44100, 0.4), later)
    assert all(not diff(wl, row) for row in after)


def test_argument_errors_leave_the_feed_usable():
    import vorbis_amd
    ref = _ref()
    blob = vorbis_amd.default_setup_blob("44k_stereo_q4")
    live = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=4096, write_frames=1024)
    whole = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=4096)
    slot, _ = live.buffer(2)
    for call in (lambda: live.wrote(slot, 1, 100), lambda: live.wrote(slot, 2, [100, 200]),
                 lambda: live.wrote_live(slot, [5000]), lambda: live.wrote_live(slot, [1, 1, 1]),
                 lambda: live.wrote_live(slot, [0, 10], [1, 0])):
        with pytest.raises(vorbis_amd.VamdError) as e:
            call()
        assert e.value.code == -131
    live.release(slot)
    wslot, _ = whole.buffer(2)
    with pytest.raises(vorbis_amd.VamdError):
        whole.wrote_live(wslot, [100])
    whole.release(wslot)
    whole.close()
    rng = np.random.default_rng(1)
    x = s16_streams(rng, 2, 4000, ["noise"])[0]
    got = live.encode_live([x], [1])[0]
    live.close()
    assert not diff(reference(ref.RefEncoder(2, 44100, 0.4), x), got)
