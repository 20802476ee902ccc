"""GPU suite: the Ogg feed (vamd_feed_ogg_headers / vamd_feed_ogg, include/vorbis_amd.h) -- whole streams in from host
memory, one complete Ogg Vorbis I file per stream back, framed on the device (vorbis_amd/csrc/k_ogg.h).  Every file is
taken apart by a demuxer written from doc/framing.html alone (tests/ogg_framing.py; it checks every page's CRC with a
bit-serial routine) and must hold the reference's own header packets and packets, which must also be the packets the
same group's vamd_feed_packets reports; it must equal, byte for byte, what the shipped host mux makes of those packets
(one policy, two implementations); and the reference decoder must get exactly the stream's frame count out of it."""
import numpy as np
import pytest

from tests import bitrate_host as bh
from tests import checker
from tests import ogg_framing as fr
from tests import ogg_host as oh
from tests import ref_host as rh
from tests.feed_cases import check_file, reference_records, small_arena, spy_totals
from tests.signals import s16_streams

pytestmark = pytest.mark.gpu


def _ref():
    from oracle import ref
    if not ref.available():
        pytest.skip("needs the reference build")
    return ref


@pytest.fixture(scope="module")
def host():
    return oh.HostOgg()


def run_group(feed, parts, serials=None):
    """One group through an Ogg feed -> (files, packet rows as Feed.encode gives them, the ogg() record)"""
    parts = [np.ascontiguousarray(x, dtype=feed.dtype) for x in parts]
    ch = parts[0].shape[1]
    slot, buf = feed.buffer(ch)
    try:
        flat = np.concatenate([x.reshape(-1) for x in parts])
        buf[:flat.size] = flat
        if serials is not None:
            feed.ogg_serials(slot, serials)
        lengths = [x.shape[0] for x in parts]
        if len(set(lengths)) == 1:
            feed.wrote(slot, len(parts), lengths[0])
        else:
            feed.wrote(slot, len(parts), lengths)
        o = feed.ogg(slot)
        r = feed.packets(slot)
    finally:
        feed.release(slot)
    off = o["stream_offset"]
    assert o["nstreams"] == len(parts) and off[0] == 0 and off[-1] == o["total_bytes"]
    files = [bytes(o["bytes"][int(off[s]):int(off[s + 1])]) for s in range(len(parts))]
    return files, feed._rows(r, len(parts)), o


def check_group(host, ref, setup, headers, parts, files, rows, o, serials):
    ch, _, q = checker.SETUPS[setup]
    out = []
    for s, x in enumerate(parts):
        assert o["status"][s] == 0
        want = reference_records(ref, ch, q, x)
        out.append(check_file(host, headers, want, rows[s], files[s], x.shape[0], serials[s], int(o["npages"][s])))
    return out


@pytest.mark.parametrize("setup,arena", [pytest.param(s, None, id=s) for s in ("44k_stereo_q4", "44k_stereo_q9", "44k_mono_q5")] +
                         [pytest.param(s, "4096", id=s + "-arena4096") for s in ("44k_stereo_q4", "44k_stereo_q9", "44k_mono_q5")])
def test_files_of_whole_streams(host, setup, arena, monkeypatch):
    """arena: each lane's packet arena starts at 4096 bytes (VAMD_FEED_OUT_BYTES), so the group is laid out and paged a
    second time, the arena and its mirror grown in between."""
    import vorbis_amd
    ref = _ref()
    small_arena(monkeypatch, arena)
    ch, rate, q = checker.SETUPS[setup]
    headers = rh.reference_headers(ch, rate, q)
    rng = np.random.default_rng(2026)
    frames = 30000
    pcm = s16_streams(rng, ch, frames, ["noise", "gated", "sine", "clicks", "silence", "gated"])
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob(setup), lanes_per_device=2, max_streams=8, max_frames=frames, ogg_headers=headers)
    totals = spy_totals(feed)
    try:
        files, rows, o = run_group(feed, list(pcm))
        again = feed.encode_ogg(pcm, serials=range(6))     # (the other lane; encode_ogg's own path)
    finally:
        feed.close()
    assert again == files
    assert len(totals) == 1 and (not arena or totals[0] > 4096), totals
    check_group(host, ref, setup, headers, list(pcm), files, rows, o, list(range(6)))


@pytest.mark.parametrize("frames", [1, 33, 2049, 7777])
def test_short_streams(host, frames):
    import vorbis_amd
    ref = _ref()
    setup = "44k_stereo_q4"
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(frames)
    pcm = s16_streams(rng, 2, frames, ["noise", "gated", "sine"])
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob(setup), lanes_per_device=1, max_streams=4, max_frames=8192, ogg_headers=headers)
    try:
        files, rows, o = run_group(feed, list(pcm))
    finally:
        feed.close()
    check_group(host, ref, setup, headers, list(pcm), files, rows, o, [0, 1, 2])


def test_unequal_streams_and_their_place_in_the_group(host):
    """vamd_feed_wrote_v; and a stream's file depends neither on its place in the group nor on the lane."""
    import vorbis_amd
    ref = _ref()
    setup = "44k_stereo_q4"
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(31)
    lengths = [40000, 1, 33, 2049, 17000, 3072, 39999, 700, 25000, 4097, 12345]
    kinds = ["gated", "noise", "sine", "clicks", "noise", "gated", "sine", "gated", "clicks", "noise", "gated"]
    parts = [s16_streams(rng, 2, n, [k])[0] for n, k in zip(lengths, kinds)]
    serials = [100 + s for s in range(len(parts))]
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob(setup), lanes_per_device=2, max_streams=16, max_frames=40000, ogg_headers=headers)
    try:
        files, rows, o = run_group(feed, parts, serials)
        again, _, _ = run_group(feed, parts[::-1], serials[::-1])
    finally:
        feed.close()
    check_group(host, ref, setup, headers, parts, files, rows, o, serials)
    for s in range(len(parts)):
        assert again[::-1][s] == files[s], "stream %d's file depends on its place in the group" % s


def test_the_255_segment_rule(host):
    """A 400 000-frame silent stream: the reference makes 393 one-byte packets of it, so one page holds 255 of them."""
    import vorbis_amd
    ref = _ref()
    setup = "44k_stereo_q4"
    headers = rh.reference_headers(2, 44100, 0.4)
    x = np.zeros((400000, 2), np.int16)
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob(setup), lanes_per_device=1, max_streams=1, max_frames=400000, ogg_headers=headers)
    try:
        files, rows, o = run_group(feed, [x])
    finally:
        feed.close()
    pages = check_group(host, ref, setup, headers, [x], files, rows, o, [0])[0]
    assert any(p["nseg"] == 255 and p["done"] == 255 for p in pages)


def test_a_continued_page(host):
    """Silence, then noise from frame S on: with the reference's packets the policy cuts the first audio page at segment
    255 inside a packet -- for S = 249 968 (255 segments, 727 body bytes, 254 packets completed), then a page flagged
    0x01 | 0x04; for S = 241 776 the cut falls inside a later packet.  The expectation itself (the host mux of the reference's packets) is asserted to contain the continued
    page, so the case cannot stop being covered silently."""
    import vorbis_amd
    ref = _ref()
    setup = "44k_stereo_q4"
    headers = rh.reference_headers(2, 44100, 0.4)
    parts = []
    for S in (249968, 241776):
        rng = np.random.default_rng(7)
        x = np.zeros((S + 12000, 2))
        x[S:] = (rng.random((12000, 2)) - 0.5) * 0.8
        parts.append(np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16))
    for s, x in enumerate(parts):
        want = reference_records(ref, 2, 0.4, x)
        expect, _ = fr.demux(host.mux(headers, [w["packet"] for w in want], [w["granulepos"] for w in want], s))
        assert any(p["flags"] & 1 for p in expect), "the reference's packets of stream %d no longer give a continued page" % s
        assert expect[2]["nseg"] == 255 and expect[3]["flags"] & 1, "... nor cut their first audio page inside a packet"
        if s == 0:
            assert (expect[2]["nseg"], expect[2]["body"], expect[2]["done"]) == (255, 727, 254) and expect[3]["flags"] == 5
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob(setup), lanes_per_device=1, max_streams=2, max_frames=262144, ogg_headers=headers)
    try:
        files, rows, o = run_group(feed, parts)
    finally:
        feed.close()
    got = check_group(host, ref, setup, headers, parts, files, rows, o, [0, 1])
    assert (got[0][2]["nseg"], got[0][2]["body"], got[0][2]["done"]) == (255, 727, 254) and got[0][3]["flags"] == 5
    assert got[1][2]["nseg"] == 255 and got[1][3]["flags"] & 1


@pytest.mark.parametrize("arena", [None, "4096"])
def test_managed_and_its_slices(host, arena, monkeypatch):
    """An ABR setup; once with the default slice and once with slices of 7 blocks, so that pages straddle slices: the
    same files.  arena: in the sliced run the packet arena starts at 4096 bytes (VAMD_FEED_OUT_BYTES), so it and its
    mirror grow between slices, the earlier slices' packets kept."""
    import vorbis_amd
    ref = _ref()
    rates = (-1, 128000, -1)
    blob = bh.managed_blob(2, rates)
    headers = rh.reference_headers(2, 44100, managed=rates)
    parts = []
    for s, n in enumerate([66150, 20000, 700]):
        x = bh.signal("music", 2, n, 50 + s).T
        parts.append(np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16))

    def run():
        feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=4, max_frames=66150, ogg_headers=headers)
        totals.append(spy_totals(feed))
        try:
            return run_group(feed, parts, [7, 8, 9])
        finally:
            feed.close()
    totals = []
    files, rows, o = run()
    monkeypatch.setenv("VAMD_TEST_KNOBS", "1")
    monkeypatch.setenv("VAMD_FEED_SLICE", "7")
    if arena:
        monkeypatch.setenv("VAMD_FEED_OUT_BYTES", arena)
    files7, rows7, o7 = run()
    assert not arena or totals[1][0] > 4096, totals
    assert files7 == files and rows7 == rows
    assert len(rows[0]) >= 3 * 7, "the first stream must span several slices"
    for s, x in enumerate(parts):
        assert o["status"][s] == 0
        want = reference_records(ref, 2, 0.4, x, managed=rates)
        check_file(host, headers, want, rows[s], files[s], x.shape[0], 7 + s, int(o["npages"][s]))


def test_serial_numbers(host):
    """Given ones appear in every page of their stream; default ones are distinct across two groups."""
    import vorbis_amd
    setup = "44k_stereo_q4"
    _ref()
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(4)
    pcm = s16_streams(rng, 2, 9000, ["noise", "gated", "sine"])
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob(setup), lanes_per_device=2, max_streams=4, max_frames=9000, ogg_headers=headers)
    try:
        a, _, _ = run_group(feed, list(pcm))
        b, _, _ = run_group(feed, list(pcm))
        c, _, _ = run_group(feed, list(pcm), [0xdeadbeef, 5])     # (two given; the third takes the counter's)
    finally:
        feed.close()
    seen = []
    for files in (a, b):
        for f in files:
            pages, _ = fr.demux(f)
            assert len({p["serial"] for p in pages}) == 1
            seen.append(pages[0]["serial"])
    assert len(set(seen)) == 6
    given = [{p["serial"] for p in fr.demux(f)[0]} for f in c]
    assert given[0] == {0xdeadbeef} and given[1] == {5} and len(given[2]) == 1 and not given[2] & set(seen)


def test_a_stream_with_a_nan_gets_no_file(host):
    import vorbis_amd
    ref = _ref()
    setup = "44k_stereo_q4"
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(8)
    pcm = (s16_streams(rng, 2, 20000, ["noise", "gated", "sine"]).astype(np.float32) / np.float32(32768.0))
    pcm[1, 10000, 0] = np.nan
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob(setup), lanes_per_device=1, max_streams=4, max_frames=20000, fmt=vorbis_amd.FEED_F32,
                           ogg_headers=headers)
    try:
        files, rows, o = run_group(feed, list(pcm))
    finally:
        feed.close()
    assert files[1] == b"" and o["npages"][1] == 0 and o["status"][1] == vorbis_amd.api.STATUS_NONFINITE
    assert any(r[0] is None for r in rows[1])
    for s in (0, 2):
        assert o["status"][s] == 0
        want = reference_records(ref, 2, 0.4, pcm[s])
        check_file(host, headers, want, rows[s], files[s], 20000, s, int(o["npages"][s]))


def test_errors():
    import vorbis_amd
    _ref()
    blob = vorbis_amd.default_setup_blob("44k_stereo_q4")
    headers = rh.reference_headers(2, 44100, 0.4)
    mono = rh.reference_headers(1, 44100, 0.5)
    for bad in ((mono[0], headers[1], headers[2]), (headers[0][:29], headers[1], headers[2]), (headers[0], headers[2], headers[1])):
        with pytest.raises(vorbis_amd.VamdError) as e:
            vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=4096, ogg_headers=bad)
        assert e.value.code == vorbis_amd.api.VAMD_EINVAL and "Ogg headers" in str(e.value)
    feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=4096)
    try:
        slot, buf = feed.buffer(2)
        with pytest.raises(vorbis_amd.VamdError):
            feed.ogg_headers(*headers)                  # after the first vamd_feed_buffer
        buf[:8192] = 0
        feed.wrote(slot, 1, 4096)
        with pytest.raises(vorbis_amd.VamdError):
            feed.ogg(slot)                              # a feed without headers
        feed.packets(slot)
        feed.release(slot)
    finally:
        feed.close()
    live = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=4096, write_frames=1024)
    try:
        with pytest.raises(vorbis_amd.VamdError) as e:
            live.ogg_headers(*headers)
        assert e.value.code == vorbis_amd.api.VAMD_EIMPL
    finally:
        live.close()


def test_packets_of_an_ogg_feed_equal_a_plain_feeds():
    import vorbis_amd
    _ref()
    setup = "44k_stereo_q4"
    blob = vorbis_amd.default_setup_blob(setup)
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(12)
    parts = [s16_streams(rng, 2, n, [k])[0] for n, k in [(20000, "gated"), (5000, "noise"), (12345, "clicks")]]
    res = []
    for hdr in (None, headers):
        feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=4, max_frames=20000, ogg_headers=hdr)
        try:
            slot, buf = feed.buffer(2)
            flat = np.concatenate([x.reshape(-1) for x in parts])
            buf[:flat.size] = flat
            feed.wrote(slot, 3, [x.shape[0] for x in parts])
            res.append(feed.packets(slot))
            feed.release(slot)
        finally:
            feed.close()
    for k in ("nstreams", "nblocks", "total_bytes"):
        assert res[0][k] == res[1][k]
    for k in ("stream_start", "offset", "bits", "granulepos", "info", "bytes"):
        assert np.array_equal(res[0][k], res[1][k]), k
