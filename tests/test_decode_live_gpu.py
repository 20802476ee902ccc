"""GPU: the live decoder (vamd_decode_live_*; Analyzer.live_decoder, LiveDecoder.write) -- continuing streams decoded in
pieces, the lap carried on the device between calls (k_decode_carry_out behind k_synth, k_decode_carry_in ahead of k_lap).
A stream's pieces laid end to end are held, bit for bit, against libvorbis' decoder over the WHOLE stream
(ref_host.reference_decode) and against decode_streams of the whole stream.  The cut lists and the flagged case are the
ones tests/test_decode_live_cpu.py takes through the same code on the host.  Every stream of every case is compared, or has
its flagged status asserted."""
import numpy as np
import pytest

from oracle import ref
from tests import decode_cases, decode_live_host as live, ref_host, synth_host
from tests.feed_cases import Q4, same_bits
from tests.signals import gated_streams as streams

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")]
EINVAL = -131
_rows = {}


def reference_rows(name, seconds, seed):
    """the reference encoder's packets of gated-noise streams -> (headers, per stream (packets, end granule, the reference
    decoder's samples)); once per process"""
    key = (name, tuple(seconds), seed)
    if key not in _rows:
        headers = ref_host.encoder_headers(ref_host.encoder(name))
        out = []
        for p in streams(name, seconds, seed):
            recs = ref_host.encoder(name).encode_stream(np.ascontiguousarray(p.T))
            packets, granules = [r["packet"] for r in recs], [r["granulepos"] for r in recs]
            want = ref_host.reference_decode(headers + packets, granules)
            assert want.shape == (p.shape[1], len(p))
            want.setflags(write=False)
            out.append((packets, granules[-1], want))
        _rows[key] = (headers, out)
    return _rows[key]


def analyzer(name):
    import vorbis_amd
    return vorbis_amd.Analyzer(ref_host.encoder(name).pack_setup())


def run_rounds(an, dec, packets, cut_lists, ends, slots=None):
    """live.rounds() through LiveDecoder.write -> per stream (status, samples on the host)"""
    calls, who = live.rounds(packets, cut_lists, ends, slots)
    res = []
    for slots_, pieces, close, granules in calls:
        got, status = dec.write(slots_, pieces, close, granules, with_status=True)
        assert len(got) == len(slots_) and all(t.is_cuda and t.device.index == an.device and t.shape[0] == an.channels for t in got)
        res.append([(int(status[i]), got[i].cpu().numpy()) for i in range(len(got))])
    return live.join(res, who, len(packets), an.channels)


def assert_equal(got, want, what):
    assert len(got) == len(want)
    for s, ((status, pcm), w) in enumerate(zip(got, want)):
        assert status == 0, (what, s, status)
        assert pcm.shape == w.shape, (what, s, pcm.shape, w.shape)
        assert same_bits(pcm, w), (what, s, int((pcm.view(np.uint32) != w.view(np.uint32)).sum()))


def whole(an, packets, ends):
    got, status = an.decode_streams(packets, ends, with_status=True)
    return [(int(status[s]), got[s].cpu().numpy()) for s in range(len(got))]


def test_one_packet_pieces_and_random_cuts():
    """four streams on four slots at once, a packet a call: they end at different calls, so later calls name fewer slots.
    Then a seeded cut list per stream, with empty pieces (none of them the closing piece: that one alone would leave the
    end granule unapplied)."""
    _, rows = reference_rows(Q4, (0.3, 0.7, 1.1, 1.5), 11)
    packets, ends, want = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    assert len(set(len(p) for p in packets)) == 4
    rng = np.random.default_rng(5)
    cuts = [[c for c in live.random_cuts(len(p), rng) if c < len(p)] for p in packets]
    assert all(any(a == b for a, b in zip([0] + c, c)) for c in cuts)
    an = analyzer(Q4)
    try:
        assert_equal(whole(an, packets, ends), want, "whole")
        dec = an.live_decoder(4)
        got = run_rounds(an, dec, packets, [list(range(1, len(p))) for p in packets], ends)
        assert_equal(got, want, "one packet a piece")
        assert [g[1].shape for g in got] == [(2, e) for e in ends]
        assert_equal(run_rounds(an, dec, packets, cuts, ends), want, ("cut lists", cuts))
    finally:
        an.close()


@pytest.mark.parametrize("name", synth_host.FEED_SETUPS + ("44k_stereo_q4_uncoupled",))
def test_setups(name):
    _, rows = reference_rows(name, (0.3, 0.5), 23)
    packets, ends, want = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    an = analyzer(name)
    try:
        assert_equal(whole(an, packets, ends), want, "whole")
        dec = an.live_decoder(2)
        assert_equal(run_rounds(an, dec, packets, [list(range(3, len(p), 3)) for p in packets], ends), want, name)
    finally:
        an.close()


def test_slots():
    """A opens on slot 0 in call 1; B opens on slot 5 in call 3; call 4 names slot 5 alone; A closes in call 5; C takes slot 0
    in call 6"""
    _, rows = reference_rows(Q4, (0.3, 0.5, 0.4), 31)
    (A, endA, wantA), (B, endB, wantB), (Cc, endC, wantC) = rows
    a = live.pieces_of(A, [len(A) // 4, len(A) // 2, 3 * len(A) // 4])   # calls 1, 2, 3, 5
    b = live.pieces_of(B, [len(B) // 3, 2 * len(B) // 3, len(B) - 1])    # calls 3, 4, 5, 6
    c = live.pieces_of(Cc, [len(Cc) // 2])                               # calls 6, 7
    calls = [([0], [a[0]], [], {}), ([0], [a[1]], [], {}), ([0, 5], [a[2], b[0]], [], {}), ([5], [b[1]], [], {}),
             ([5, 0], [b[2], a[3]], [0], {0: endA}), ([0, 5], [c[0], b[3]], [5], {5: endB}), ([0], [c[1]], [0], {0: endC})]
    who = [[0], [0], [0, 1], [1], [1, 0], [2, 1], [2]]
    an = analyzer(Q4)
    try:
        dec = an.live_decoder(6)
        res = []
        for slots, pieces, close, granules in calls:
            got, status = dec.write(slots, pieces, close, granules, with_status=True)
            res.append([(int(status[i]), got[i].cpu().numpy()) for i in range(len(got))])
        assert_equal(live.join(res, who, 3, 2), [wantA, wantB, wantC], "slots")
    finally:
        an.close()


def test_many_short_streams():
    """130 short streams in two pieces each in one decoder: more (stream, channel) pairs than the carry kernels have
    workgroups (they stride), more than two waves of k_unpack"""
    g = decode_cases.short_streams(130)
    cuts = [[len(p) // 2] for p in g.streams]
    assert all(0 < c[0] < len(p) for c, p in zip(cuts, g.streams)) and 130 * g.channels > 256
    an = analyzer(Q4)
    try:
        dec = an.live_decoder(130)
        got = run_rounds(an, dec, g.streams, cuts, g.ends)
    finally:
        an.close()
    decode_cases.check(g, got)


def test_flagged_stream_among_clean_ones():
    """tests/test_decode_live_cpu.py::test_flagged_packet on slot 2 of four: piece 1's samples stand, pieces 2 to 4 have
    no frames and carry STATUS_TRUNCATED; the clean streams and the slot's next stream equal the reference"""
    import vorbis_amd
    from tests.test_decode_live_cpu import flagged_case
    _, ch, packets, end, want, pieces, bad = flagged_case()
    n = len(packets)
    cuts = [n // 4, n // 2, 3 * n // 4]
    an = analyzer(Q4)
    try:
        dec = an.live_decoder(4)
        res = []
        for r in range(4):
            got, status = dec.write([0, 1, 2, 3], [pieces[r], pieces[r], bad[r], pieces[r]], close=[0, 1, 2, 3] if r == 3 else [],
                                    end_granules={s: end for s in range(4)}, with_status=True)
            res.append([(int(status[i]), got[i].cpu().numpy()) for i in range(4)])
        first = res[0][2][1]
        assert res[0][2][0] == 0 and first.shape[1] > 0 and same_bits(first, want[:, :first.shape[1]])
        for r in (1, 2, 3):
            assert res[r][2][0] == vorbis_amd.STATUS_TRUNCATED and res[r][2][1].shape == (ch, 0), (r, res[r][2][0], res[r][2][1].shape)
        clean = live.join([[row[0], row[1], row[3]] for row in res], [[0, 1, 2]] * 4, 3, ch)
        assert_equal(clean, [want] * 3, "the clean streams")
        assert_equal(run_rounds(an, dec, [packets], [cuts], [end], slots=[2]), [want], "the slot's next stream")
    finally:
        an.close()


def test_a_live_feeds_loop():
    """a live feed's consumer: each group's packets go to the decoder as the group comes out, close and the end granule
    with the closing group (the cuts of tests/test_decode_gpu.py::test_a_live_feeds_packets)"""
    import vorbis_amd
    parts = streams(Q4, (0.3, 0.5), 41)
    cuts = [[5000, 0, len(parts[0]) - 5000], [1, 9000, len(parts[1]) - 9001]]
    blob = ref_host.encoder(Q4).pack_setup()
    headers = ref_host.encoder_headers(ref_host.encoder(Q4))
    feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=32000, fmt=vorbis_amd.FEED_F32, write_frames=1024)
    an = vorbis_amd.Analyzer(blob)
    try:
        dec = an.live_decoder(2)
        pos, rows, out = [0, 0], [[], []], [[], []]
        for r in range(3):
            pieces = [x[pos[s]:pos[s] + cuts[s][r]] for s, x in enumerate(parts)]
            pos = [pos[s] + cuts[s][r] for s in range(2)]
            group = feed.encode_live(pieces, [r == 2] * 2)
            closing = [s for s in range(2) if group[s] and group[s][-1][3]]
            assert closing == ([0, 1] if r == 2 else [])
            got, status = dec.write([0, 1], [[p for p, _, _, _ in row] for row in group], close=closing,
                                    end_granules={s: group[s][-1][1] for s in closing}, with_status=True)
            assert not status.any()
            for s in range(2):
                rows[s] += group[s]
                out[s].append(got[s].cpu().numpy())
        for s in range(2):
            want = ref_host.reference_decode(headers + [p for p, _, _, _ in rows[s]], [g for _, g, _, _ in rows[s]])
            got = np.concatenate(out[s], axis=1)
            assert got.shape == (2, len(parts[s])) == want.shape and same_bits(got, want), (s, got.shape, want.shape)
    finally:
        an.close()
        feed.close()


def test_bad_calls():
    """a slot named twice, a slot equal to max_streams, more streams than slots: EINVAL, and the decoder goes on as if the
    call had not been made"""
    import vorbis_amd
    _, rows = reference_rows(Q4, (0.3, 0.5), 23)
    (A, endA, wantA), (B, endB, wantB) = rows
    a, b = live.pieces_of(A, [len(A) // 2]), live.pieces_of(B, [len(B) // 3])
    an = analyzer(Q4)
    try:
        dec = an.live_decoder(2)
        first, st = dec.write([0, 1], [a[0], b[0]], with_status=True)
        assert not st.any()
        for slots, pieces, reason in (([1, 1], [b[1], a[1]], "twice"), ([2, 0], [b[1], a[1]], "outside"), ([0, 1, 1], [a[1], b[1], []], "more streams")):
            with pytest.raises(vorbis_amd.VamdError) as e:
                dec.write(slots, pieces, close=slots, end_granules={0: endA, 1: endB})
            assert e.value.code == EINVAL and reason in str(e.value), str(e.value)
        last, st = dec.write([1, 0], [b[1], a[1]], close=[0, 1], end_granules={0: endA, 1: endB}, with_status=True)
        assert not st.any()
        got = [(0, np.concatenate([first[0].cpu().numpy(), last[1].cpu().numpy()], axis=1)),
               (0, np.concatenate([first[1].cpu().numpy(), last[0].cpu().numpy()], axis=1))]
        assert_equal(got, [wantA, wantB], "around the refused calls")
    finally:
        an.close()
