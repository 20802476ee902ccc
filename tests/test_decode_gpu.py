"""GPU: the packet decoder (vamd_decode_plan / vamd_decode_streams; Analyzer.decode_streams) -- audio packets in host
memory to PCM on the device, k_unpack ahead of k_synth and k_lap -- against libvorbis' decoder over the same packets with
their granule positions (tests/ogg_host.py), bit for bit.  The packets are the reference encoder's, a VBR decoded feed's, a
bitrate-managed feed's and a live feed's; the malformed cases are ones tests/test_unpack_cpu.py has taken through the same
code on the host."""
import numpy as np
import pytest

from oracle import ref
from tests import ogg_host, synth_host
from tests.test_feed_decoded import Q4, feed_of, same_bits, streams
from tests.test_unpack_cpu import MANAGED_RATES

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")]
EINVAL = -131


def analyzer(name):
    import vorbis_amd
    return vorbis_amd.Analyzer(synth_host.encoder(name).pack_setup())


def reference_streams(name, parts):
    """the reference encoder's packets of [frames, ch] streams -> per stream (packets, granules)"""
    out = []
    for p in parts:
        recs = synth_host.encoder(name).encode_stream(np.ascontiguousarray(p.T))
        out.append(([r["packet"] for r in recs], [r["granulepos"] for r in recs]))
    return out


def check(an, headers, rows, got, status, skip=()):
    assert len(got) == len(rows)
    for s, (packets, granules) in enumerate(rows):
        assert got[s].is_cuda and got[s].device.index == an.device
        if s in skip:
            continue
        want = ogg_host.reference_decode(headers + packets, granules)
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
    check(an, synth_host.encoder_headers(synth_host.encoder(name)), rows, got, status)


def test_short_streams():
    rng = np.random.default_rng(3)
    parts = [((rng.random((n, 2), dtype=np.float32) - 0.5) * 0.8).astype(np.float32) for n in synth_host.SHORT_LENGTHS]
    rows = reference_streams(Q4, parts)
    an = analyzer(Q4)
    try:
        got, status = an.decode_streams([p for p, _ in rows], [g[-1] for _, g in rows], with_status=True)
        assert [tuple(g.shape) for g in got] == [(2, n) for n in synth_host.SHORT_LENGTHS]
        check(an, synth_host.encoder_headers(synth_host.encoder(Q4)), rows, got, status)
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
    got = vorbis_amd.decode(synth_host.encoder(Q4).pack_setup(), [rows[0][0]], [rows[0][1][-1]])
    want = ogg_host.reference_decode(synth_host.encoder_headers(synth_host.encoder(Q4)) + rows[0][0], rows[0][1])
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
        check(an, synth_host.encoder_headers(ref.RefEncoder(2, 44100, managed=MANAGED_RATES)), pairs, got, status, skip=flagged)
    finally:
        an.close()
        feed.close()


def test_a_live_feeds_packets():
    """a live feed in pieces (for which the feed has no decoded signal either)"""
    import vorbis_amd
    from tests.test_feed_live import run_live
    parts = streams(Q4, (0.3, 0.5), 41)
    cuts = [[5000, 0, len(parts[0]) - 5000], [1, 9000, len(parts[1]) - 9001]]
    blob = synth_host.encoder(Q4).pack_setup()
    feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=32000, fmt=vorbis_amd.FEED_F32, write_frames=1024)
    an = vorbis_amd.Analyzer(blob)
    try:
        rows = run_live(feed, parts, cuts)
        pairs = [([p for p, _, _, _ in row], [g for _, g, _, _ in row]) for row in rows]
        got, status = an.decode_streams([p for p, _ in pairs], [g[-1] for _, g in pairs], with_status=True)
        assert [tuple(g.shape) for g in got] == [(2, len(p)) for p in parts]
        check(an, synth_host.encoder_headers(synth_host.encoder(Q4)), pairs, got, status)
    finally:
        an.close()
        feed.close()


def test_flagged_streams_and_bad_descriptors():
    """tests/test_unpack_cpu.py::test_flagged_streams on the GPU; then a descriptor whose offsets are not monotone: EINVAL,
    nothing launched, and the context decodes the next group as before"""
    import vorbis_amd
    x = np.ascontiguousarray(synth_host.gated_noise(2, 44100, 20000, 3).T)
    (packets, granules), = reference_streams(Q4, [x])
    assert len(packets) > 4 and len(packets[2]) > 5
    cut = packets[:2] + [packets[2][:5]] + packets[3:]
    typed = packets[:1] + [bytes([packets[1][0] ^ 1]) + packets[1][1:]] + packets[2:]
    want = ogg_host.reference_decode(synth_host.encoder_headers(synth_host.encoder(Q4)) + packets, granules)
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
