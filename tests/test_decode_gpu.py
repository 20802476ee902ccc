"""GPU: the packet decoder (vamd_decode_plan / vamd_decode_streams; Analyzer.decode_streams) -- audio packets in host
memory to PCM on the device, k_unpack ahead of k_synth and k_lap -- against libvorbis' decoder over the same packets with
their granule positions (tests/ref_host.py), bit for bit.  The packets are the reference encoder's, a VBR decoded feed's, a
bitrate-managed feed's and a live feed's; the malformed cases are ones tests/test_unpack_cpu.py has taken through the same
code on the host."""
import numpy as np
import pytest

from oracle import ref
from tests import decode_cases, ref_host, synth_host, unpack_host
from tests.feed_cases import Q4, decoded_feed_of as feed_of, run_live, same_bits
from tests.signals import MANAGED_RATES, gated_noise, gated_streams as streams

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")]
EINVAL = -131


def analyzer(name):
    import vorbis_amd
    return vorbis_amd.Analyzer(ref_host.encoder(name).pack_setup())


def reference_streams(name, parts):
    """the reference encoder's packets of [frames, ch] streams -> per stream (packets, granules)"""
    out = []
    for p in parts:
        recs = ref_host.encoder(name).encode_stream(np.ascontiguousarray(p.T))
        out.append(([r["packet"] for r in recs], [r["granulepos"] for r in recs]))
    return out


def check(an, headers, rows, got, status, skip=()):
    assert len(got) == len(rows)
    for s, (packets, granules) in enumerate(rows):
        assert got[s].is_cuda and got[s].device.index == an.device
        if s in skip:
            continue
        want = ref_host.reference_decode(headers + packets, granules)
        g = got[s].cpu().numpy()
        assert status[s] == 0 and same_bits(g, want), "stream %d: %s against %s, %d samples differ" % (
            s, g.shape, want.shape, int((g.view(np.uint32) != want.view(np.uint32)).sum()) if g.shape == want.shape else -1)


@pytest.mark.parametrize("name", synth_host.FEED_SETUPS + ("44k_stereo_q4_uncoupled",))
def test_decode_equals_the_reference_decoder(name):
    parts = streams(name, (0.3, 0.7, 1.1, 1.5), 11)
    rows = reference_streams(name, parts)
    an = analyzer(name)
    try:
        got, status = an.decode_streams([p for p, _ in rows], [g[-1] for _, g in rows], with_status=True)
    finally:
        an.close()
    assert [tuple(g.shape) for g in got] == [(p.shape[1], len(p)) for p in parts]
    check(an, ref_host.encoder_headers(ref_host.encoder(name)), rows, got, status)


def test_short_streams():
    rng = np.random.default_rng(3)
    parts = [((rng.random((n, 2), dtype=np.float32) - 0.5) * 0.8).astype(np.float32) for n in synth_host.SHORT_LENGTHS]
    rows = reference_streams(Q4, parts)
    an = analyzer(Q4)
    try:
        got, status = an.decode_streams([p for p, _ in rows], [g[-1] for _, g in rows], with_status=True)
        assert [tuple(g.shape) for g in got] == [(2, n) for n in synth_host.SHORT_LENGTHS]
        check(an, ref_host.encoder_headers(ref_host.encoder(Q4)), rows, got, status)
        # no packets, one packet: no frames; without a granule position the last block is not cut
        none, st = an.decode_streams([[], rows[3][0][:1], rows[3][0]], with_status=True)
        assert [tuple(g.shape) for g in none[:2]] == [(2, 0), (2, 0)] and not st.any()
        assert none[2].shape[1] >= synth_host.SHORT_LENGTHS[3] and same_bits(none[2][:, :got[3].shape[1]].cpu().numpy(), got[3].cpu().numpy())
    finally:
        an.close()


def test_module_level_decode():
    import vorbis_amd
    parts = streams(Q4, (0.2,), 31)
    rows = reference_streams(Q4, parts)
    got = vorbis_amd.decode(ref_host.encoder(Q4).pack_setup(), [rows[0][0]], [rows[0][1][-1]])
    want = ref_host.reference_decode(ref_host.encoder_headers(ref_host.encoder(Q4)) + rows[0][0], rows[0][1])
    assert same_bits(got[0].cpu().numpy(), want)


def test_a_decoded_feeds_own_packets():
    """a VBR decoded feed's rows through decode_streams: the feed's `decoded` tensors, bit for bit"""
    import torch
    parts = streams(Q4, (0.3, 0.7, 1.1, 1.5), 11)
    x = np.zeros((len(parts), 2, max(len(p) for p in parts)), np.float32)
    for s, p in enumerate(parts):
        x[s, :, :len(p)] = p.T
    x = torch.from_numpy(x).cuda()
    feed = feed_of(Q4, parts)
    an = analyzer(Q4)
    try:
        rows, dec = feed.roundtrip_tensors([x[s, :, :len(p)] for s, p in enumerate(parts)])  # (views of one tensor: equal strides)
        got, status = an.decode_streams([[p for p, _, _, _ in row] for row in rows], [row[-1][1] for row in rows], with_status=True)
        assert not status.any() and all(len(r) > 5 for r in rows)
        for s in range(len(parts)):
            assert same_bits(got[s].cpu().numpy(), dec[s].cpu().numpy()), s
    finally:
        an.close()
        feed.close()


def test_a_managed_feeds_packets():
    """a bitrate-managed feed (ABR 128 kb/s, the setup test_feed_decoded.py::test_errors builds -- for which the feed itself
    has no decoded signal): its packets decode as the reference decodes them, except the streams in which the manager cut a
    packet, which are flagged as truncated -- at most half (tests/test_unpack_cpu.py::test_managed_streams: the reference's
    own managed encoder on these inputs stays under that)"""
    import vorbis_amd
    parts = streams(Q4, (0.3, 0.7, 1.1, 1.5), 11)
    blob = ref.RefEncoder(2, 44100, managed=MANAGED_RATES).pack_setup()
    feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=len(parts), max_frames=max(len(p) for p in parts), fmt=vorbis_amd.FEED_F32)
    an = vorbis_amd.Analyzer(blob)
    try:
        rows = feed.encode(parts)
        pairs = [([p for p, _, _, _ in row], [g for _, g, _, _ in row]) for row in rows]
        got, status = an.decode_streams([p for p, _ in pairs], [g[-1] for _, g in pairs], with_status=True)
        flagged = [s for s in range(len(parts)) if status[s]]
        assert all(status[s] == vorbis_amd.STATUS_TRUNCATED and got[s].shape == (2, 0) for s in flagged)
        assert 2 * len(flagged) <= len(parts), flagged
        check(an, ref_host.encoder_headers(ref.RefEncoder(2, 44100, managed=MANAGED_RATES)), pairs, got, status, skip=flagged)
    finally:
        an.close()
        feed.close()


def test_a_live_feeds_packets():
    """a live feed in pieces (for which the feed has no decoded signal either)"""
    import vorbis_amd
    parts = streams(Q4, (0.3, 0.5), 41)
    cuts = [[5000, 0, len(parts[0]) - 5000], [1, 9000, len(parts[1]) - 9001]]
    blob = ref_host.encoder(Q4).pack_setup()
    feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=32000, fmt=vorbis_amd.FEED_F32, write_frames=1024)
    an = vorbis_amd.Analyzer(blob)
    try:
        rows = run_live(feed, parts, cuts)
        pairs = [([p for p, _, _, _ in row], [g for _, g, _, _ in row]) for row in rows]
        got, status = an.decode_streams([p for p, _ in pairs], [g[-1] for _, g in pairs], with_status=True)
        assert [tuple(g.shape) for g in got] == [(2, len(p)) for p in parts]
        check(an, ref_host.encoder_headers(ref_host.encoder(Q4)), pairs, got, status)
    finally:
        an.close()
        feed.close()


@pytest.fixture(scope="module")
def exe():
    return unpack_host.build()


MUTATED_CASES, CLEAN = 192, 6  # some 3800 packets, 60 waves of k_unpack; the clean streams among the cases
_fresh = {}


def decode_group(an, g):
    """one decode_streams call over a decode_cases.Group -> per stream (status, pcm [ch][frames] on the host)"""
    got, status = an.decode_streams(g.streams, g.ends, with_status=True)
    assert len(got) == len(g.streams) and all(t.is_cuda and t.device.index == an.device for t in got)
    return [(int(status[s]), got[s].cpu().numpy()) for s in range(len(got))]


def fresh(key, g):
    """the group through a context of its own, with the environment as the suite has it; once per key"""
    import vorbis_amd
    if key not in _fresh:
        an = vorbis_amd.Analyzer(g.blob)
        try:
            _fresh[key] = decode_group(an, g)
        finally:
            an.close()
    return _fresh[key]


def assert_same_results(a, b):
    assert len(a) == len(b)
    for s, ((sa, pa), (sb, pb)) in enumerate(zip(a, b)):
        assert sa == sb and same_bits(pa, pb), (s, sa, sb, pa.shape, pb.shape)


def mutated_group(name, n=MUTATED_CASES, clean=CLEAN):
    return decode_cases.with_clean(decode_cases.cases(name, n), clean)


@pytest.mark.parametrize("name", list(synth_host.SETUPS))
def test_mutated_streams(exe, tmp_path, name):
    """tests/test_unpack_cpu.py::test_mutated_streams on the GPU, twice the cases and six clean streams among them in ONE
    call, so that mutated and clean packets share waves: lanes that leave early with a status beside lanes that go on,
    divergent serial decodes, the posts in LDS a wave's lanes apart.  Against the reference as on the host; and the
    statuses are the host build's.  Seen: 0, STATUS_TRUNCATED and, in four setups once each, STATUS_NOTAUDIO; never
    STATUS_BADCODE."""
    g = mutated_group(name)
    assert g.cls[-1] != "clean" and g.where[-1][1] == len(g.streams[-1]) - 1  # the group's final bytes are a mutated packet
    got = fresh((name, MUTATED_CASES), g)
    decode_cases.check(g, got)
    host = unpack_host.host_decode_streams(exe, tmp_path, g.blob, g.streams, g.ends, g.channels)
    assert [st for st, _ in got] == [st for st, _ in host]


@pytest.mark.parametrize("lanes", [1, 5, 63])
def test_packets_a_wave(lanes, monkeypatch):
    """the test knob VAMD_UNPACK_LANES -- k_unpack's grid, its LDS and the stride of a lane's posts: the same statuses and
    the same bits as with 64 packets a wave, which are the reference's"""
    import vorbis_amd
    for name in ("44k_stereo_q4", "44k_51_q3"):
        g = mutated_group(name, 48, 2)
        want = fresh((name, 48), g)  # (before the knob is set)
        decode_cases.check(g, want)
        with monkeypatch.context() as m:
            m.setenv("VAMD_TEST_KNOBS", "1")
            m.setenv("VAMD_UNPACK_LANES", str(lanes))
            an = vorbis_amd.Analyzer(g.blob)
            try:
                assert "VAMD_UNPACK_LANES=%d" % lanes in an.config_string().split()
                got = decode_group(an, g)
            finally:
                an.close()
        assert_same_results(got, want)


def test_end_granules():
    """tests/test_unpack_cpu.py::test_end_granules on the GPU: thirty streams in one group, the counts that are no multiple
    of four in the tail of k_lap's four-frames-a-thread loop"""
    g = decode_cases.end_granules()
    got = fresh("ends", g)
    decode_cases.check(g, got)
    assert tuple(pcm.shape[1] for _, pcm in got[:10]) == decode_cases.END_COUNTS_9000


def test_many_streams():
    """more streams than k_lap has rows (1024: it strides over the rest), through decode_run: every stream at its offset"""
    import vorbis_amd
    g = decode_cases.short_streams(1100)
    ch = g.channels
    an = vorbis_amd.Analyzer(g.blob)
    try:
        pcm, frames, off, status = an.decode_run(an.decode_prepare(g.streams, g.ends))
        h = pcm.cpu().numpy()
    finally:
        an.close()
    assert len(frames) == 1100 and not status.any()
    assert [int(f) for f in frames[:8]] == list(synth_host.SHORT_LENGTHS)
    for s in range(1100):
        want = g.want(s)
        got = h[int(off[s]):int(off[s]) + ch * int(frames[s])].reshape(ch, int(frames[s]))
        assert same_bits(got, want), (s, got.shape, want.shape)


def test_context_reuse():
    """one context over a large group, a group of one 20-frame stream (its bytes go where the large group's lay: the
    workspace is kept, and exactly the group's bytes are copied), the large group again: what contexts of their own give.
    Then decode_run into a caller's tensor: the planned floats, nothing behind them, and no tensor too small."""
    import torch
    import vorbis_amd
    big = mutated_group(Q4)
    want_big = fresh((Q4, MUTATED_CASES), big)
    decode_cases.check(big, want_big)
    short = decode_cases.short_streams(8)
    one = decode_cases.Group(Q4, short.blob, short.headers, short.channels)
    one.streams, one.ends, one.cls, one.where = short.streams[1:2], short.ends[1:2], ["clean"], [None]
    assert one.want(0).shape == (2, 20)
    want_one = fresh("one", one)
    decode_cases.check(one, want_one)
    an = vorbis_amd.Analyzer(big.blob)
    try:
        first = decode_group(an, big)
        small = decode_group(an, one)
        again = decode_group(an, big)
        assert_same_results(first, want_big)
        assert_same_results(small, want_one)
        assert_same_results(again, want_big)
        prep = an.decode_prepare(big.streams, big.ends)
        pcm, frames, off, status = an.decode_run(prep)
        total = int(frames.sum()) * big.channels
        assert total > 0 and pcm.numel() >= total
        sentinel = -12345.678
        t = torch.full((total + 64,), sentinel, dtype=torch.float32, device=pcm.device)
        pcm2, frames2, off2, status2 = an.decode_run(prep, pcm=t)
        assert pcm2.data_ptr() == t.data_ptr() and np.array_equal(frames, frames2) and np.array_equal(off, off2) and np.array_equal(status, status2)
        h = t.cpu().numpy()
        assert np.array_equal(h[:total].view(np.uint32), pcm[:total].cpu().numpy().view(np.uint32))
        assert np.array_equal(h[total:], np.full(64, sentinel, np.float32))
        with pytest.raises(ValueError):
            an.decode_run(prep, pcm=torch.empty(total - 1, dtype=torch.float32, device=pcm.device))
    finally:
        an.close()


def test_flagged_streams_and_bad_descriptors():
    """tests/test_unpack_cpu.py::test_flagged_streams on the GPU; then a descriptor whose offsets are not monotone: EINVAL,
    nothing launched, and the context decodes the next group as before"""
    import vorbis_amd
    x = np.ascontiguousarray(gated_noise(2, 44100, 20000, 3).T)
    (packets, granules), = reference_streams(Q4, [x])
    assert len(packets) > 4 and len(packets[2]) > 5
    cut = packets[:2] + [packets[2][:5]] + packets[3:]
    typed = packets[:1] + [bytes([packets[1][0] ^ 1]) + packets[1][1:]] + packets[2:]
    want = ref_host.reference_decode(ref_host.encoder_headers(ref_host.encoder(Q4)) + packets, granules)
    an = analyzer(Q4)
    try:
        got, status = an.decode_streams([packets, cut, typed, packets], [granules[-1]] * 4, with_status=True)
        assert list(status) == [0, vorbis_amd.STATUS_TRUNCATED, vorbis_amd.STATUS_NOTAUDIO, 0]
        assert got[1].shape == (2, 0) and got[2].shape == (2, 0)
        assert same_bits(got[0].cpu().numpy(), want) and same_bits(got[3].cpu().numpy(), want)
        with pytest.raises(ValueError):
            an.decode_streams([packets[:2] + [None] + packets[3:]])
        off = np.zeros(len(packets) + 1, np.int64)
        np.cumsum([len(p) for p in packets], out=off[1:])
        off[3], off[4] = off[4], off[3]
        with pytest.raises(vorbis_amd.VamdError) as e:
            an.decode_streams([packets], [granules[-1]], offset=off)
        assert e.value.code == EINVAL and "monotone" in str(e.value)
        with pytest.raises(vorbis_amd.VamdError) as e:
            an.decode_streams([packets], [granules[-1]], stream_start=[0, len(packets) + 1])
        assert e.value.code == EINVAL
        again = an.decode_streams([packets], [granules[-1]])
        assert same_bits(again[0].cpu().numpy(), want)
    finally:
        an.close()
