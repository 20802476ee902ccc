"""GPU suite: the live Ogg feed (vamd_feed_ogg_headers_live, include/vorbis_amd.h "the live Ogg feed") -- continuing streams
fed in pieces, per group and stream the next bytes of the stream's Ogg file back, paged on the device with the open page's
packets carried between groups (vorbis_amd/csrc/k_ogg.h).  A stream's pieces laid end to end must be the file: the
reference's headers and packets (tests/feed_cases.py's check_file: spec demuxer, host mux byte for byte, policy,
reference decoder), the whole-stream Ogg feed's file for the same serial number, the same under every cut -- and every
piece a whole number of pages on its own."""
import numpy as np
import pytest

from tests import bitrate_host as bh
from tests import checker
from tests import ogg_framing as fr
from tests import ogg_host as oh
from tests import ref_host as rh
from tests.feed_cases import check_file, records, rows_of, small_arena, spy_totals, whole_file
from tests.signals import managed_s16_streams as managed_streams, mixed_streams, random_cuts, s16_streams

pytestmark = pytest.mark.gpu


def _ref():
    from oracle import ref
    if not ref.available():
        pytest.skip("needs the reference build")
    return ref


@pytest.fixture(scope="module")
def host():
    return oh.HostOgg()


@pytest.fixture(scope="module")
def live_host():
    return oh.HostOgg()


def run_live_ogg(feed, streams, cuts, serials=None):
    """Feed streams [frames_s, ch] to a one-lane live Ogg feed in rounds, as tests/feed_cases.py's run_live does: in round
    r stream s gets cuts[s][r] frames and is closed with its last piece.  serials: given to every round (they count where a
    stream begins).  -> per stream a list over the rounds of dict(bytes, npages, status, rows, close)."""
    got = [[] for _ in streams]
    pos = [0] * len(streams)
    ch = streams[0].shape[1]
    for r in range(max(len(c) for c in cuts)):
        frames, close, flat = [], [], []
        for s, x in enumerate(streams):
            n = cuts[s][r] if r < len(cuts[s]) else 0
            flat.append(np.ascontiguousarray(x[pos[s]:pos[s] + n], dtype=feed.dtype).reshape(-1))
            pos[s] += n
            frames.append(n)
            close.append(r == len(cuts[s]) - 1)
        slot, buf = feed.buffer(ch)
        try:
            f = np.concatenate(flat)
            buf[:f.size] = f
            if serials is not None:
                feed.ogg_serials(slot, serials)
            feed.wrote_live(slot, frames, close)
            o = feed.ogg(slot)
            p = feed.packets(slot)
        finally:
            feed.release(slot)
        off = o["stream_offset"]
        assert o["nstreams"] == len(streams) and off[0] == 0 and off[-1] == o["total_bytes"]
        rows = feed._rows(p, len(streams))
        for s in range(len(streams)):
            got[s].append(dict(bytes=bytes(o["bytes"][int(off[s]):int(off[s + 1])]), npages=int(o["npages"][s]), status=int(o["status"][s]),
                               rows=rows[s], close=close[s]))
    assert pos == [len(x) for x in streams]
    return got


@pytest.mark.parametrize("setup", ["44k_stereo_q4", "44k_stereo_q9", "44k_mono_q5"])
def test_random_cuts_give_the_whole_stream_feeds_files(host, setup):
    import vorbis_amd
    ref = _ref()
    ch, rate, q = checker.SETUPS[setup]
    headers = rh.reference_headers(ch, rate, q)
    rng = np.random.default_rng(7 + ch)
    streams, cuts = mixed_streams(rng, ch)
    serials = [100 + s for s in range(len(streams))]
    blob = vorbis_amd.default_setup_blob(setup)
    feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=8, max_frames=32000, write_frames=1024, ogg_headers=headers)
    try:
        a = run_live_ogg(feed, streams, cuts, serials)
        b = run_live_ogg(feed, streams, [[len(x) // 3, 0, len(x) - len(x) // 3] if len(x) > 2 else [len(x)] for x in streams], serials)
    finally:
        feed.close()
    whole = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=8, max_frames=32000, ogg_headers=headers)
    try:
        files = whole.encode_ogg(list(streams), serials=serials)
    finally:
        whole.close()
    for s, x in enumerate(streams):
        assert all(g["status"] == 0 for g in a[s])
        f = whole_file(a[s])
        want = records(ref.RefEncoder(ch, rate, q), x)
        pages = check_file(host, headers, want, rows_of(a[s]), f, x.shape[0], serials[s], sum(g["npages"] for g in a[s]))
        assert len(pages) == sum(g["npages"] for g in a[s])
        assert f == files[s], "stream %d: the pieces are not the whole-stream Ogg feed's file" % s
        assert whole_file(b[s]) == f, "stream %d: another cut gives another file" % s
        assert all(g["bytes"] == b"" for g in a[s][len(cuts[s]):]), "a closed stream went on returning bytes"


def test_pieces_of_700_frames(host):
    """Most groups complete no page: their ranges are empty and the carry grows."""
    import vorbis_amd
    ref = _ref()
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(70)
    x = s16_streams(rng, 2, 30000, ["gated"])[0]
    y = s16_streams(rng, 2, 9100, ["noise"])[0]
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_stereo_q4"), lanes_per_device=1, max_streams=2, max_frames=700, write_frames=1024,
                           ogg_headers=headers)
    try:
        got = run_live_ogg(feed, [x, y], [[700] * 42 + [600], [700] * 13], [5, 6])
    finally:
        feed.close()
    assert sum(g["bytes"] == b"" and not g["close"] for g in got[0][1:43]) > 20
    for s, z in enumerate((x, y)):
        want = records(ref.RefEncoder(2, 44100, 0.4), z)
        check_file(host, headers, want, rows_of(got[s]), whole_file(got[s]), z.shape[0], 5 + s, sum(g["npages"] for g in got[s]))


def test_the_255_segment_rule_and_a_continued_page_across_groups(host, live_host):
    """tests/test_feed_ogg.py's test_a_continued_page stream (silence, noise from frame S = 249 968 on: the first audio page
    is cut at segment 255 inside a packet), eight copies in one lane, their piece ends staggered in steps of 1000 frames
    from S - 3000 to S + 8000, through the first noise blocks.  What each boundary leaves behind is computed on the host,
    from the packet counts the feed reports per group and the shipped walk in pieces: some group must return pages without
    closing its stream and leave an open page whose first packet is continued, and some one that carries >= 200 packets."""
    import vorbis_amd
    ref = _ref()
    headers = rh.reference_headers(2, 44100, 0.4)
    S = 249968
    rng = np.random.default_rng(7)
    x = np.zeros((S + 12000, 2))
    x[S:] = (rng.random((12000, 2)) - 0.5) * 0.8
    x = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    want = records(ref.RefEncoder(2, 44100, 0.4), x)
    expect, _ = fr.demux(host.mux(headers, [w["packet"] for w in want], [w["granulepos"] for w in want], 0))
    assert (expect[2]["nseg"], expect[2]["body"], expect[2]["done"]) == (255, 727, 254) and expect[3]["flags"] == 5, \
        "the reference's packets no longer cut the first audio page inside a packet"
    cuts = []
    for i in range(8):
        first = S - 3000 + 1000 * i
        cuts.append([first, 1000, 1000, 1000, 1000, len(x) - first - 4000])
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_stereo_q4"), lanes_per_device=1, max_streams=8, max_frames=262144,
                           write_frames=1024, ogg_headers=headers)
    try:
        got = run_live_ogg(feed, [x] * 8, cuts, list(range(8)))
    finally:
        feed.close()
    continued = carried = 0
    for s in range(8):
        f = whole_file(got[s])
        pages = check_file(host, headers, want, rows_of(got[s]), f, x.shape[0], s, sum(g["npages"] for g in got[s]))
        assert (pages[2]["nseg"], pages[2]["body"], pages[2]["done"]) == (255, 727, 254) and pages[3]["flags"] == 5
        st = live_host.stream(headers, s)
        for g in got[s]:
            piece = st.piece([r[0] for r in g["rows"]], [r[1] for r in g["rows"]], g["close"])
            assert piece == g["bytes"], "stream %d: a group's bytes are not the host mux's for that group" % s
            if g["npages"] and not g["close"]:
                continued += st.open_page["byte0"] > 0
                carried += st.open_page["npackets"] >= 200
    assert continued > 0 and carried > 0, (continued, carried)


def test_managed_and_its_slices(host, monkeypatch):
    """ABR 128 kb/s in random pieces, with the default slice and with slices of 5 blocks: the same bytes, the host mux of
    the reference's managed packets."""
    import vorbis_amd
    ref = _ref()
    rates = (-1, 128000, -1)
    blob = bh.managed_blob(2, rates)
    headers = rh.reference_headers(2, 44100, managed=rates)
    streams = managed_streams([26000, 9000, 2000])
    rng = np.random.default_rng(3)
    cuts = [random_cuts(rng, len(x)) for x in streams]

    def run():
        feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=4, max_frames=26000, write_frames=1024, ogg_headers=headers)
        try:
            return run_live_ogg(feed, streams, cuts, [7, 8, 9])
        finally:
            feed.close()
    a = run()
    monkeypatch.setenv("VAMD_TEST_KNOBS", "1")
    monkeypatch.setenv("VAMD_FEED_SLICE", "5")
    b = run()
    for s, x in enumerate(streams):
        f = whole_file(a[s])
        assert [g["bytes"] for g in b[s]] == [g["bytes"] for g in a[s]], "stream %d: the slice size changes the bytes" % s
        want = records(ref.RefEncoder(2, 44100, managed=rates), x)
        check_file(host, headers, want, rows_of(a[s]), f, x.shape[0], 7 + s, sum(g["npages"] for g in a[s]))


@pytest.mark.parametrize("kind", ["vbr", "abr"])
def test_a_group_laid_out_twice_advances_its_streams_once(kind, monkeypatch):
    """The lane's packet arena starts at 4096 bytes, so a group outgrows it: a VBR group is laid out and paged a second
    time, a managed one grows it between slices.  The same bytes as without the knob."""
    import vorbis_amd
    _ref()
    if kind == "vbr":
        blob = vorbis_amd.default_setup_blob("44k_stereo_q4")
        headers = rh.reference_headers(2, 44100, 0.4)
        rng = np.random.default_rng(44)
        streams = [s16_streams(rng, 2, n, [k])[0] for n, k in [(40000, "noise"), (20000, "gated")]]
    else:
        rates = (-1, 128000, -1)
        blob = bh.managed_blob(2, rates)
        headers = rh.reference_headers(2, 44100, managed=rates)
        streams = managed_streams([90000, 60000, 2000])
    rng = np.random.default_rng(45)
    cuts = [random_cuts(rng, len(x)) for x in streams]

    def run():
        feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=4, max_frames=max(len(x) for x in streams), write_frames=1024,
                               ogg_headers=headers)
        totals = spy_totals(feed)
        try:
            return run_live_ogg(feed, streams, cuts), totals
        finally:
            feed.close()
    a, _ = run()
    small_arena(monkeypatch, "4096")
    b, totals = run()
    assert max(totals) > 4096, totals
    for s in range(len(streams)):
        assert [g["bytes"] for g in b[s]] == [g["bytes"] for g in a[s]], "stream %d" % s
        fr.demux(whole_file(b[s]))


def test_a_non_finite_sample_ends_its_streams_file_only(host, live_host):
    """The inputs of tests/test_feed_live.py's test_non_finite_sample_ends_its_stream_only."""
    import vorbis_amd
    ref = _ref()
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(5)
    streams = [s16_streams(rng, 2, 30000, [k])[0].astype(np.float32) / np.float32(32768.0) for k in ["gated", "noise", "sine"]]
    poisoned = streams[1].copy()
    poisoned[17001, 1] = np.nan
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_stereo_q4"), lanes_per_device=1, max_streams=4, max_frames=8000,
                           fmt=vorbis_amd.FEED_F32, write_frames=1024, ogg_headers=headers)
    try:
        got = run_live_ogg(feed, [streams[0], poisoned, streams[2]], [[5000, 6000, 7000, 8000, 4000]] * 3, [10, 11, 12])
        later = s16_streams(rng, 2, 8000, ["gated"])[0].astype(np.float32) / np.float32(32768.0)
        after = run_live_ogg(feed, [later] * 3, [[8000]] * 3)
    finally:
        feed.close()
    want = [records(ref.RefEncoder(2, 44100, 0.4), x) for x in streams]
    for s in (0, 2):
        assert all(g["status"] == 0 for g in got[s])
        check_file(host, headers, want[s], rows_of(got[s]), whole_file(got[s]), 30000, 10 + s, sum(g["npages"] for g in got[s]))
    hit = next(r for r, g in enumerate(got[1]) if any(row[0] is None for row in g["rows"]))
    assert 0 < hit < 4
    for g in got[1][:hit]:
        assert g["status"] == 0
    for g in got[1][hit:]:
        assert g["bytes"] == b"" and g["npages"] == 0 and g["status"] == vorbis_amd.api.STATUS_NONFINITE
    prefix = fr.pages_of(whole_file(got[1][:hit]))              # a valid Ogg prefix: whole pages, no end-of-stream page
    assert len(prefix) >= 2 and [p["seq"] for p in prefix] == list(range(len(prefix))) and not any(p["flags"] & 4 for p in prefix)
    assert prefix[0]["flags"] == 2 and all(p["serial"] == 11 for p in prefix)
    held = fr.packets_of(prefix)
    assert held[:3] == list(headers)
    assert held[3:] == [w["packet"] for w in want[1][:len(held) - 3]]
    st = live_host.stream(headers, 11)                            # ... and group by group what the host mux in pieces hands out
    for g in got[1][:hit]:
        assert st.piece([r[0] for r in g["rows"]], [r[1] for r in g["rows"]], False) == g["bytes"]
    wl = records(ref.RefEncoder(2, 44100, 0.4), later)
    serials = set()
    for s in range(3):
        assert after[s][0]["status"] == 0
        pages = check_file(host, headers, wl, after[s][0]["rows"], after[s][0]["bytes"], 8000, fr.demux(after[s][0]["bytes"])[0][0]["serial"],
                           after[s][0]["npages"])
        serials.add(pages[0]["serial"])
    assert len(serials) == 3


def test_slot_reuse_and_serial_numbers(host):
    """Two streams one after the other in a slot: two files, each with a bos page at sequence 0.  A serial number belongs
    to a stream: a given one applies where the stream begins and is ignored for an open one; default ones are distinct."""
    import vorbis_amd
    ref = _ref()
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(99)
    a, b, c = (s16_streams(rng, 2, n, [k])[0] for n, k in [(9000, "gated"), (7000, "noise"), (15000, "sine")])
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_stereo_q4"), lanes_per_device=1, max_streams=2, max_frames=6000,
                           write_frames=1024, ogg_headers=headers)
    files = {"a": b"", "b": b"", "c": b""}
    try:
        # (slot 0's piece, its close, slot 1's piece, its close, the serials given)
        steps = [(("a", a[:5000]), 0, ("c", c[:6000]), 0, [11, 22]),
                 (("a", a[5000:]), 1, ("c", c[6000:12000]), 0, [33, 44]),      # both open: 33 and 44 are ignored
                 (("b", b[:3000]), 0, ("c", c[12000:]), 1, None),              # b begins: the counter's
                 (("b", b[3000:]), 1, ("c", c[:0]), 0, [55, 66])]              # b open, slot 1 has no stream: ignored
        for (n0, p0), c0, (n1, p1), c1, serials in steps:
            out = feed.encode_live_ogg([p0, p1], [c0, c1], serials)
            files[n0] += out[0]
            files[n1] += out[1]
        d = feed.encode_live_ogg([a[:6000], c[:0]], [1, 0])[0]                         # a third stream in slot 0: the counter's next
    finally:
        feed.close()
    seen = {}
    for name, x in (("a", a), ("b", b), ("c", c)):
        pages, got = fr.demux(files[name])
        assert got[:3] == list(headers)
        assert got[3:] == [w["packet"] for w in records(ref.RefEncoder(2, 44100, 0.4), x)]
        assert pages[0]["flags"] == 2 and [p["seq"] for p in pages] == list(range(len(pages))) and pages[-1]["flags"] & 4
        assert len({p["serial"] for p in pages}) == 1
        seen[name] = pages[0]["serial"]
    assert seen["a"] == 11 and seen["c"] == 22
    dp, _ = fr.demux(d)
    assert dp[0]["flags"] == 2 and dp[0]["seq"] == 0
    assert len({seen["a"], seen["b"], seen["c"], dp[0]["serial"]}) == 4 and dp[0]["serial"] == seen["b"] + 1
    assert d[:58] != files["a"][:58] and d[58:] != b""


def test_packets_of_a_live_ogg_feed_equal_a_plain_live_feeds():
    import vorbis_amd
    _ref()
    blob = vorbis_amd.default_setup_blob("44k_stereo_q4")
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(12)
    parts = [s16_streams(rng, 2, n, [k])[0] for n, k in [(20000, "gated"), (5000, "noise"), (12345, "clicks")]]
    cuts = [[7000, 6000, 7000], [5000], [1, 0, 12344]]
    res = []
    for hdr in (None, headers):
        feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=4, max_frames=12500, write_frames=1024, ogg_headers=hdr)
        rounds, pos = [], [0, 0, 0]
        try:
            for r in range(3):
                slot, buf = feed.buffer(2)
                frames = [c[r] if r < len(c) else 0 for c in cuts]
                flat = np.concatenate([x[p:p + n].reshape(-1) for x, p, n in zip(parts, pos, frames)])
                buf[:flat.size] = flat
                pos = [p + n for p, n in zip(pos, frames)]
                feed.wrote_live(slot, frames, [r == len(c) - 1 for c in cuts])
                rounds.append(feed.packets(slot))
                feed.release(slot)
        finally:
            feed.close()
        res.append(rounds)
    for p, o in zip(*res):
        for k in ("nstreams", "nblocks", "total_bytes"):
            assert p[k] == o[k]
        for k in ("stream_start", "offset", "bits", "granulepos", "info", "bytes"):
            assert np.array_equal(p[k], o[k]), k


def test_errors():
    import vorbis_amd
    _ref()
    EINVAL = vorbis_amd.api.VAMD_EINVAL
    blob = vorbis_amd.default_setup_blob("44k_stereo_q4")
    headers = rh.reference_headers(2, 44100, 0.4)
    mono = rh.reference_headers(1, 44100, 0.5)
    whole = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=4096)
    try:
        with pytest.raises(vorbis_amd.VamdError) as e:
            whole.ogg_headers_live(*headers)                  # a whole-stream feed
        assert e.value.code == EINVAL and "live feed" in str(e.value)
    finally:
        whole.close()
    for bad in ((mono[0], headers[1], headers[2]), (headers[0][:29], headers[1], headers[2]), (headers[0], headers[2], headers[1])):
        with pytest.raises(vorbis_amd.VamdError) as e:
            vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=4096, write_frames=1024, ogg_headers=bad)
        assert e.value.code == EINVAL and "Ogg headers" in str(e.value)
    live = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=4096, write_frames=1024)
    try:
        slot, buf = live.buffer(2)
        with pytest.raises(vorbis_amd.VamdError) as e:
            live.ogg_headers_live(*headers)                   # after the first vamd_feed_buffer
        assert e.value.code == EINVAL and "before the first vamd_feed_buffer" in str(e.value)
        buf[:8192] = 0
        live.wrote_live(slot, [4096], [1])
        with pytest.raises(vorbis_amd.VamdError):
            live.ogg(slot)                                    # a live feed without headers
        live.packets(slot)
        live.release(slot)
    finally:
        live.close()
