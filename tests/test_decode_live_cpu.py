"""CPU: the live decoder (vamd_decode_live_*) for one lane on the host -- tests/c/decode_live_host.cpp, a program of its own
built with -fsanitize=address,undefined and run as a child process: the shipped vamd_decode_live_plan.h, unpack_packet,
synth_block, the two carry bodies and lap_sample, piece by piece.  A stream's pieces laid end to end are held, bit for bit
(floats as bit patterns), against libvorbis' decoder over the WHOLE stream (ref_host.reference_decode), at every cut of
its packet list this file makes; and against the whole-stream decoder's host build (tests/unpack_host.py).  Every stream
of every case is compared, or has its flagged status asserted."""
import numpy as np
import pytest

from oracle import ref
from tests import decode_cases, decode_live_host as live, ref_host, synth_host, unpack_host
from tests.feed_cases import Q4, same_bits
from tests.signals import gated_noise

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")
_made = {}


@pytest.fixture(scope="module")
def exe():
    return live.build()


def made(name, seconds, seed):
    """gated-noise streams of `seconds` from the reference encoder -> (blob, ch, [packets], [end granule], [size classes],
    [the reference decoder's samples], [its samples with no granule position on any packet]); once per process, the
    samples read-only.  The second reference is for a cut list whose closing piece is empty: such a piece only frees the
    slot, its end granule comes too late to cut samples that have left (include/vorbis_amd.h)."""
    key = (name, tuple(seconds), seed)
    if key not in _made:
        headers = ref_host.encoder_headers(ref_host.encoder(name))
        rows = []
        for i, sec in enumerate(seconds):
            enc = ref_host.encoder(name)
            recs = enc.encode_stream(gated_noise(enc.channels, enc.rate, int(enc.rate * sec) + 7 * i, seed + i))
            packets, granules = [r["packet"] for r in recs], [r["granulepos"] for r in recs]
            want = ref_host.reference_decode(headers + packets, granules)
            assert want.shape == (enc.channels, granules[-1])
            uncut = ref_host.reference_decode(headers + packets, [-1] * len(packets))
            assert uncut.shape[1] >= want.shape[1] and same_bits(uncut[:, :want.shape[1]], want)
            want.setflags(write=False), uncut.setflags(write=False)
            rows.append((packets, granules[-1], [r["W"] for r in recs], want, uncut))
        enc = ref_host.encoder(name)
        _made[key] = (enc.pack_setup(), enc.channels) + tuple(list(col) for col in zip(*rows))
    return _made[key]


def q4():
    m = made(Q4, (0.3, 0.5), 21)
    # between them: long/long, long/short, short/long, short/short
    assert set().union(*(synth_host.lap_cases(Ws) for Ws in m[4])) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    return m


def decode(exe, tmp, blob, ch, jobs, max_streams):
    """jobs: [(streams, cut lists, ends)], each decoded side by side on slots 0 .. (live.rounds), job after job on ONE
    decoder -> per job, per stream (status, samples)"""
    calls, spans = [], []
    for streams, cuts, ends in jobs:
        c, who = live.rounds(streams, cuts, ends)
        spans.append((len(calls), who, len(streams)))
        calls += [live.call(*a) for a in c]
    res = live.run(exe, tmp, blob, max_streams, calls, ch)
    return [live.join(res[at:at + len(who)], who, n, ch) for at, who, n in spans]


def wanted(m, cut_lists, idx=None):
    """per stream the reference its cut list is held to (made())"""
    idx = range(len(m[2])) if idx is None else idx
    return [m[6][i] if live.closes_empty(m[2][i], c) else m[5][i] for i, c in zip(idx, cut_lists)]


def assert_equal(got, want, what):
    assert len(got) == len(want)
    for s, ((status, pcm), w) in enumerate(zip(got, want)):
        assert status == 0, (what, s, status)
        assert pcm.shape == w.shape, (what, s, pcm.shape, w.shape)
        assert same_bits(pcm, w), (what, s, int((pcm.view(np.uint32) != w.view(np.uint32)).sum()))


def test_pieces_of_one_packet(exe, tmp_path):
    m = q4()
    blob, ch, streams, ends, _, want, _ = m
    (got,) = decode(exe, tmp_path, blob, ch, [(streams, [list(range(1, len(p))) for p in streams], ends)], 2)
    assert_equal(got, want, "one packet a piece")
    # ... and the whole-stream decoder's host build gives the same
    whole = unpack_host.host_decode_streams(unpack_host.build(), tmp_path, blob, streams, ends, ch)
    assert_equal(whole, want, "whole")


def test_every_single_cut(exe, tmp_path):
    """two pieces, the cut at every position 0 .. npackets (at the ends: an empty piece in front or behind)"""
    m = q4()
    blob, ch, streams, ends, _, want, _ = m
    jobs, which = [], []
    for k in range(max(len(p) for p in streams) + 1):
        idx = [i for i, p in enumerate(streams) if k <= len(p)]
        jobs.append(([streams[i] for i in idx], [[k]] * len(idx), [ends[i] for i in idx]))
        which.append(idx)
    assert sum(len(i) for i in which) == sum(len(p) + 1 for p in streams)
    for k, (got, idx) in enumerate(zip(decode(exe, tmp_path, blob, ch, jobs, 2), which)):
        assert_equal(got, wanted(m, [[k]] * len(idx), idx), ("cut at", k))


def test_random_cut_lists(exe, tmp_path):
    m = q4()
    blob, ch, streams, ends, _, want, _ = m
    rng = np.random.default_rng(40)
    jobs = [(streams, [live.random_cuts(len(p), rng) for p in streams], ends) for _ in range(20)]  # 40 cut lists
    assert all(any(a == b for a, b in zip([0] + c, c + [len(p)])) for _, cuts, _ in jobs for c, p in zip(cuts, streams))  # empty pieces
    for n, got in enumerate(decode(exe, tmp_path, blob, ch, jobs, 2)):
        assert_equal(got, wanted(m, jobs[n][1]), ("cut list", n, jobs[n][1]))


def test_open_and_close_in_one_piece(exe, tmp_path):
    m = q4()
    blob, ch, streams, ends, _, want, _ = m
    (got,) = decode(exe, tmp_path, blob, ch, [(streams, [[], []], ends)], 2)
    assert_equal(got, want, "one piece")


@pytest.mark.parametrize("name", ["44k_51_q3", "8k_mono_q3"])
def test_other_setups(exe, tmp_path, name):
    blob, ch, streams, ends, Ws, want, _ = made(name, (0.3, 0.5), 23)
    (got,) = decode(exe, tmp_path, blob, ch, [(streams, [list(range(1, len(p))) for p in streams], ends)], 2)
    assert_equal(got, want, name)


def test_end_granules(exe, tmp_path):
    """decode_cases.end_granules(): the closing piece holds the last packet alone, and with it the granule position"""
    g = decode_cases.end_granules()
    n = len(g.streams)
    (got,) = decode(exe, tmp_path, g.blob, g.channels, [(g.streams, [[len(p) - 1] for p in g.streams], g.ends)], n)
    decode_cases.check(g, got)
    assert tuple(pcm.shape[1] for _, pcm in got[:10]) == decode_cases.END_COUNTS_9000


def flagged_case():
    """a stream of four pieces whose piece 2 holds a packet cut to 5 bytes -> (blob, ch, packets, end, want, pieces, bad)"""
    m = q4()
    blob, ch, streams, ends, _, want, _ = m
    packets, n = streams[0], len(streams[0])
    pieces = live.pieces_of(packets, [n // 4, n // 2, 3 * n // 4])
    k = n // 4 + 1
    assert n // 4 >= 2 and k < n // 2 and len(packets[k]) > 5
    bad = [list(p) for p in pieces]
    bad[1][1] = packets[k][:5]
    return blob, ch, packets, ends[0], want[0], pieces, bad


def test_flagged_packet(exe, tmp_path):
    blob, ch, packets, end, want, pieces, bad = flagged_case()
    calls = [live.call([0], [bad[r]], close=[0] if r == 3 else [], granules={0: end}) for r in range(4)]
    calls += [live.call([0], [pieces[r]], close=[0] if r == 3 else [], granules={0: end}) for r in range(4)]  # the slot's next stream
    res = live.run(exe, tmp_path, blob, 1, calls, ch)
    (st, first), = res[0]
    assert st == 0 and first.shape[1] > 0 and same_bits(first, want[:, :first.shape[1]])
    for r in (1, 2, 3):
        (st, pcm), = res[r]
        assert st == unpack_host.STATUS_TRUNCATED and pcm.shape == (ch, 0), (r, st, pcm.shape)
    assert_equal(live.join(res[4:], [[0]] * 4, 1, ch), [want], "the slot's next stream")


def test_bad_descriptors(exe, tmp_path):
    """each refused descriptor changes nothing: the good calls around them decode to the reference"""
    m = q4()
    blob, ch, streams, ends, _, want, _ = m
    A, B = streams
    a, b = live.pieces_of(A, [len(A) // 2]), live.pieces_of(B, [len(B) // 3])
    good1 = live.call([0, 1], [a[0], b[0]])
    good2 = live.call([1, 0], [b[1], a[1]], close=[0, 1], granules={0: ends[0], 1: ends[1]})
    np2 = len(a[1]) + len(b[1])
    off = good2["offset"]
    bad = [dict(null=live.NULL_SLOT), dict(null=live.NULL_BYTES), dict(null=live.NULL_OFFSET), dict(null=live.NULL_START),
           dict(nstreams=-1), dict(npackets=-1), dict(npackets=np2 + 1, offset=off + [off[-1] - 1]),
           dict(offset=off[:2] + [off[1] - 1] + off[3:]), dict(offset=[-1] + off[1:]),
           dict(stream_start=[0, np2 + 1, np2]), dict(stream_start=[0, len(b[1]), np2 + 1]), dict(stream_start=[-1, len(b[1]), np2]),
           dict(slot=[1, 2]), dict(slot=[-1, 0]), dict(slot=[1, 1]),
           dict(nstreams=3, slot=[1, 0, 0], stream_start=[0, len(b[1]), np2, np2], close=[1, 1, 0], end_granule=[-1, -1, -1]),
           dict(end_granule=[-2, ends[0]])]
    calls = [good1]
    for kw in bad:
        calls.append(dict(good2, **kw))
    calls.append(good2)
    res = live.run(exe, tmp_path, blob, 2, calls, ch)
    assert all(r is None for r in res[1:-1]), [i for i, r in enumerate(res) if r is None]
    got = live.join([res[0], res[-1]], [[0, 1], [1, 0]], 2, ch)
    assert_equal(got, want, "around the refused calls")
