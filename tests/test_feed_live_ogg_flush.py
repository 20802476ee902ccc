"""GPU suite: the live Ogg feed's flush per write (vamd_feed_ogg_flush, include/vorbis_amd.h "a flush per write") -- a group
names the streams whose open page leaves with it.  The device's bytes are held, group by group, against the shipped host
mux in pieces with the same flush points (tests/ogg_host.py); behind every flushing group the pieces so far hold
exactly the packets vamd_feed_packets has reported; the whole file holds the reference encoder's packets and decodes to
the samples the unflushed file decodes to; and a feed that flushes nothing returns what it returned before the call
existed.  Shapes and inputs are tests/test_feed_live_ogg.py's."""
import numpy as np
import pytest

from tests import bitrate_host as bh
from tests import checker
from tests import ogg_framing as fr
from tests import ogg_host as oh
from tests import ref_host as rh
from tests.feed_cases import records, rows_of, small_arena, spy_totals, whole_file
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
def flush_host():
    return oh.HostOgg()


def run_flushed(feed, streams, cuts, serials, flush_of, comments=None):
    """tests/test_feed_live_ogg.py's run_live_ogg with a flush per round: flush_of(r) -> what ogg_flush takes for round r
    (a list of flags, True for every stream), or None for no call.  -> per stream a list over the rounds of
    dict(bytes, npages, status, rows, close, flush, frames)."""
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
        mask = flush_of(r)
        slot, buf = feed.buffer(ch)
        try:
            f = np.concatenate(flat)
            buf[:f.size] = f
            if serials is not None:
                feed.ogg_serials(slot, serials)
            if comments is not None:
                feed.ogg_comments(slot, comments)
            if mask is not None:
                feed.ogg_flush(slot, mask)
            feed.wrote_live(slot, frames, close)
            o = feed.ogg(slot)
            p = feed.packets(slot)
        finally:
            feed.release(slot)
        off = o["stream_offset"]
        assert o["nstreams"] == len(streams) and off[0] == 0 and off[-1] == o["total_bytes"]
        rows = feed._rows(p, len(streams))
        for s in range(len(streams)):
            flushed = mask is True or (isinstance(mask, (list, tuple)) and s < len(mask) and bool(mask[s]))
            got[s].append(dict(bytes=bytes(o["bytes"][int(off[s]):int(off[s + 1])]), npages=int(o["npages"][s]), status=int(o["status"][s]),
                               rows=rows[s], close=close[s], flush=flushed, frames=frames[s]))
    assert pos == [len(x) for x in streams]
    return got


def random_masks(rng, rounds, ns):
    """per round: no call at all, a list of flags (sometimes shorter than the group), or every stream"""
    out = []
    for _ in range(rounds):
        kind = int(rng.integers(0, 5))
        out.append(None if kind == 0 else True if kind == 1 else [bool(v) for v in rng.integers(0, 2, int(rng.integers(1, ns + 1)))])
    return out


def hold_against_the_host_mux(flush_host, headers, serial, groups):
    """One stream's groups against the shipped mux in pieces with the same flushes, byte for byte; behind every flushing
    group of the open stream the pieces so far hold exactly the packets reported so far, whole, and nothing is open.
    -> the pages of all groups, the flushed ones marked"""
    st = flush_host.stream(headers, serial)
    got, pages, given, begun = fr.Reassembler(), [], [], False
    for r, g in enumerate(groups):
        if not begun and not g["frames"]:                              # not yet begun, or behind its end: untouched, flushed or not
            assert g["bytes"] == b"" and g["npages"] == 0 and not g["rows"]
            continue
        plain = st.twin()                                              # (the same group unflushed: one page fewer where the flush closed one)
        plain.piece([w[0] for w in g["rows"]], [w[1] for w in g["rows"]], g["close"], False)
        want = st.piece([w[0] for w in g["rows"]], [w[1] for w in g["rows"]], g["close"], g["flush"])
        assert g["bytes"] == want, "round %d: the device's bytes are not the host mux's with the same flush" % r
        begun = not g["close"]
        mine = fr.pages_of(g["bytes"])
        assert len(mine) == g["npages"]
        for p in mine:
            p["flushed"] = False
        assert st.npages - plain.npages == (1 if g["flush"] and not g["close"] and plain.open_page["nseg"] > 0 else 0)
        if st.npages > plain.npages:
            mine[-1]["flushed"] = True
        got.take(mine)
        pages += mine
        given += [w[0] for w in g["rows"]]
        if g["flush"] and not g["close"]:
            assert st.ncarry == 0 and not got.is_open
            assert got.packets == list(headers) + given, "round %d: the pieces so far do not hold the packets reported so far" % r
    return pages


def check_flushed_file(host, headers, want, groups, pages, frames, serial):
    """The whole flushed file: the reference's packets and granule positions, an e_o_s page with the frame count, and
    the reference decoder gives what it gives for the unflushed file of the same packets."""
    f = whole_file(groups)
    rows = rows_of(groups)
    fp, got = fr.demux(f)                                             # (every CRC bit-serially, the continued flags)
    assert got[:3] == list(headers)
    assert got[3:] == [w["packet"] for w in want] and got[3:] == [r[0] for r in rows]
    assert [r[1] for r in rows] == [w["granulepos"] for w in want]
    assert len(fp) == len(pages) and [p["seq"] for p in fp] == list(range(len(fp))) and all(p["serial"] == serial for p in fp)
    assert fp[0]["bytes"] == 58 and fp[0]["flags"] == 2 and fp[0]["granule"] == 0
    assert fp[-1]["flags"] & 4 and fp[-1]["granule"] == frames and sum(bool(p["flags"] & 4) for p in fp) == 1
    first_audio = next(i for i, p in enumerate(fp) if sum(q["done"] for q in fp[:i + 1]) == 3) + 1
    for i, p in enumerate(fp[first_audio:-1], first_audio):           # the policy, or a flush
        assert (p["body"] > fr.FILL and p["done"] >= fr.MIN_PACKETS) or p["nseg"] == 255 or pages[i]["flushed"], (i, p)
        if pages[i]["flushed"]:
            assert pages[i]["lacing"][-1] < 255 and p["granule"] != -1 and not p["flags"] & 4
    plain = host.mux(headers, [r[0] for r in rows], [r[1] for r in rows], serial)
    pp, _ = fr.demux(plain)
    nflushed = sum(p["flushed"] for p in pages)
    assert len(f) - len(plain) == 27 * (len(fp) - len(pp)) and (nflushed > 0 or f == plain)
    a = rh.reference_decode(got, fr.page_granules(fp, len(want)))
    b = rh.reference_decode(got, fr.page_granules(pp, len(want)))
    assert a.shape[1] == frames and np.array_equal(a, b), "the flushed file does not decode to the unflushed file's samples"
    return fp


@pytest.mark.parametrize("setup", ["44k_stereo_q4", "44k_mono_q5"])
def test_random_flushes(host, flush_host, setup):
    import vorbis_amd
    ref = _ref()
    ch, rate, q = checker.SETUPS[setup]
    headers = rh.reference_headers(ch, rate, q)
    rng = np.random.default_rng(7 + ch)
    streams, cuts = mixed_streams(rng, ch)
    serials = [100 + s for s in range(len(streams))]
    masks = random_masks(np.random.default_rng(70 + ch), max(len(c) for c in cuts), len(streams))
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob(setup), lanes_per_device=1, max_streams=8, max_frames=32000, write_frames=1024,
                           ogg_headers=headers)
    try:
        got = run_flushed(feed, streams, cuts, serials, lambda r: masks[r])
    finally:
        feed.close()
    nflushed = 0
    for s, x in enumerate(streams):
        assert all(g["status"] == 0 for g in got[s])
        pages = hold_against_the_host_mux(flush_host, headers, serials[s], got[s])
        want = records(ref.RefEncoder(ch, rate, q), x)
        check_flushed_file(host, headers, want, got[s], pages, x.shape[0], serials[s])
        assert all(g["bytes"] == b"" for g in got[s][len(cuts[s]):]), "a closed stream went on returning bytes"
        nflushed += sum(p["flushed"] for p in pages)
    assert nflushed >= 3, nflushed


def test_no_flush_is_the_feed_as_it_was(flush_host):
    """All zeros, an empty call and no call at all give the same bytes; a flush named for one group does not reach the
    slot's next group."""
    import vorbis_amd
    _ref()
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(21)
    streams = [s16_streams(rng, 2, n, [k])[0] for n, k in [(21000, "noise"), (16000, "gated")]]
    cuts = [[6000, 5000, 0, 6000, 4000], [8000, 4000, 4000]]

    def run(flush_of):
        feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_stereo_q4"), lanes_per_device=1, max_streams=4, max_frames=8000,
                               write_frames=1024, ogg_headers=headers)
        try:
            return run_flushed(feed, streams, cuts, [5, 6], flush_of)
        finally:
            feed.close()
    never = run(lambda r: None)
    zeros = run(lambda r: [[0, 0], [], False, [0], [0, 0, 0, 0]][r])
    once = run(lambda r: True if r == 0 else None)
    for s in range(2):
        assert [g["bytes"] for g in zeros[s]] == [g["bytes"] for g in never[s]], "stream %d: a flush of no stream changes the bytes" % s
        assert [g["rows"] for g in once[s]] == [g["rows"] for g in never[s]]
        assert once[s][0]["flush"] and not any(g["flush"] for g in once[s][1:])
        pages = hold_against_the_host_mux(flush_host, headers, 5 + s, once[s])      # (flushed behind round 0 and nowhere else)
        assert sum(p["flushed"] for p in pages) == 1 and len(once[s][0]["bytes"]) > len(never[s][0]["bytes"])
        hold_against_the_host_mux(flush_host, headers, 5 + s, never[s])


def test_pieces_of_700_frames(host, flush_host):
    """Most groups complete no page.  A flushed piece without frames returns one page, the carried packets'; a second
    one returns nothing."""
    import vorbis_amd
    ref = _ref()
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(70)
    x = s16_streams(rng, 2, 14600, ["gated"])[0]
    y = s16_streams(rng, 2, 9100, ["noise"])[0]
    cuts = [[700] * 10 + [0, 0] + [700] * 10 + [600], [700] * 13]
    flush = {10: True, 11: True, 15: [1, 0], 16: [0, 1]}
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_stereo_q4"), lanes_per_device=1, max_streams=2, max_frames=700, write_frames=1024,
                           ogg_headers=headers)
    try:
        got = run_flushed(feed, [x, y], cuts, [5, 6], lambda r: flush.get(r))
    finally:
        feed.close()
    assert sum(g["bytes"] == b"" for g in got[0][1:10]) >= 5 and sum(len(g["rows"]) for g in got[0][:10]) > 0
    assert got[0][10]["npages"] == 1 and not got[0][10]["rows"], "a flushed piece without frames returns the carried packets' page"
    page = fr.pages_of(got[0][10]["bytes"])[0]
    held = [r[0] for g in got[0][:10] for r in g["rows"]]
    done = sum(p["done"] for g in got[0][:10] for p in fr.pages_of(g["bytes"])) - 3
    assert page["done"] == len(held) - done > 0 and page["granule"] == [r[1] for g in got[0][:10] for r in g["rows"]][-1]
    assert got[0][11]["npages"] == 0 and got[0][11]["bytes"] == b"", "a second flush finds the open page empty"
    for s, z in enumerate((x, y)):
        pages = hold_against_the_host_mux(flush_host, headers, 5 + s, got[s])
        want = records(ref.RefEncoder(2, 44100, 0.4), z)
        check_flushed_file(host, headers, want, got[s], pages, z.shape[0], 5 + s)


def test_the_255_segment_stream_flushed_where_the_open_page_is_continued_or_full_of_packets(host, flush_host):
    """tests/test_feed_live_ogg.py's 255-segment stream (silence, noise from frame 249 968 on), eight copies with staggered
    cuts.  A first pass, unflushed, tells on the host after which group each copy's open page begins inside a packet and
    after which it carries at least 200 packets; the second pass flushes exactly there (a copy with both: the even ones
    where the page carries the packets, the odd ones where it is continued -- one flush changes what the other would
    find).  The bytes are the host mux's; some flushed page has flag 0x01, some holds at least 200 packets."""
    import vorbis_amd
    ref = _ref()
    headers = rh.reference_headers(2, 44100, 0.4)
    S = 249968
    rng = np.random.default_rng(7)
    x = np.zeros((S + 12000, 2))
    x[S:] = (rng.random((12000, 2)) - 0.5) * 0.8
    x = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    cuts = []
    for i in range(8):
        first = S - 3000 + 1000 * i
        cuts.append([first, 1000, 1000, 1000, 1000, len(x) - first - 4000])
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_stereo_q4"), lanes_per_device=1, max_streams=8, max_frames=262144,
                           write_frames=1024, ogg_headers=headers)
    try:
        first_pass = run_flushed(feed, [x] * 8, cuts, list(range(8)), lambda r: None)
        where = {}
        for s in range(8):
            st = flush_host.stream(headers, s)
            continued = carried = None
            for r, g in enumerate(first_pass[s]):
                assert st.piece([w[0] for w in g["rows"]], [w[1] for w in g["rows"]], g["close"]) == g["bytes"]
                if not g["close"]:
                    if continued is None and st.open_page["byte0"] > 0:
                        continued = r
                    if carried is None and st.open_page["npackets"] >= 200:
                        carried = r
            picks = [carried, continued] if s % 2 == 0 else [continued, carried]
            where[s] = next((r for r in picks if r is not None), None)
        assert any(where[s] is not None for s in range(8)), "the first pass leaves no such open page"
        got = run_flushed(feed, [x] * 8, cuts, list(range(8, 16)), lambda r: [where[s] == r for s in range(8)])
    finally:
        feed.close()
    want = records(ref.RefEncoder(2, 44100, 0.4), x)
    flagged = many = 0
    for s in range(8):
        pages = hold_against_the_host_mux(flush_host, headers, 8 + s, got[s])
        flagged += sum(p["flushed"] and bool(p["flags"] & 1) for p in pages)
        many += sum(p["flushed"] and p["done"] >= 200 for p in pages)
        if s < 2:
            check_flushed_file(host, headers, want, got[s], pages, x.shape[0], 8 + s)
        else:
            assert fr.demux(whole_file(got[s]))[1] == list(headers) + [w["packet"] for w in want]
    assert flagged > 0 and many > 0, (flagged, many, where)


def test_managed_and_its_slices(flush_host, monkeypatch):
    """ABR 128 kb/s in random pieces with random flushes, with the default slice and with slices of 5 blocks: a group in
    slices is flushed once, behind its last slice -- the same bytes, the host mux's."""
    import vorbis_amd
    _ref()
    rates = (-1, 128000, -1)
    blob = bh.managed_blob(2, rates)
    headers = rh.reference_headers(2, 44100, managed=rates)
    streams = managed_streams([26000, 9000, 2000])
    rng = np.random.default_rng(3)
    cuts = [random_cuts(rng, len(x)) for x in streams]
    masks = random_masks(rng, max(len(c) for c in cuts), 3)

    def run():
        feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=4, max_frames=26000, write_frames=1024, ogg_headers=headers)
        try:
            return run_flushed(feed, streams, cuts, [7, 8, 9], lambda r: masks[r])
        finally:
            feed.close()
    a = run()
    monkeypatch.setenv("VAMD_TEST_KNOBS", "1")
    monkeypatch.setenv("VAMD_FEED_SLICE", "5")
    b = run()
    nflushed = 0
    for s in range(3):
        assert [g["bytes"] for g in b[s]] == [g["bytes"] for g in a[s]], "stream %d: the slice size changes the bytes" % s
        nflushed += sum(p["flushed"] for p in hold_against_the_host_mux(flush_host, headers, 7 + s, a[s]))
        assert fr.demux(whole_file(a[s]))[0][-1]["flags"] & 4
    assert nflushed > 0


def test_a_vbr_group_laid_out_twice_is_flushed_once(flush_host, monkeypatch):
    """The lane's packet arena starts at 4096 bytes, so a group outgrows it and is laid out and paged a second time: the
    state and the carry are double-buffered, the flush happens once.  The same bytes as without the knob."""
    import vorbis_amd
    _ref()
    blob = vorbis_amd.default_setup_blob("44k_stereo_q4")
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(44)
    streams = [s16_streams(rng, 2, n, [k])[0] for n, k in [(40000, "noise"), (20000, "gated")]]
    rng = np.random.default_rng(45)
    cuts = [random_cuts(rng, len(x)) for x in streams]
    masks = random_masks(rng, max(len(c) for c in cuts), 2)

    def run():
        feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=4, max_frames=40000, write_frames=1024, ogg_headers=headers)
        totals = spy_totals(feed)
        try:
            return run_flushed(feed, streams, cuts, [1, 2], lambda r: masks[r]), totals
        finally:
            feed.close()
    a, _ = run()
    small_arena(monkeypatch, "4096")
    b, totals = run()
    assert max(totals) > 4096, totals
    nflushed = 0
    for s in range(2):
        assert [g["bytes"] for g in b[s]] == [g["bytes"] for g in a[s]], "stream %d" % s
        nflushed += sum(p["flushed"] for p in hold_against_the_host_mux(flush_host, headers, 1 + s, b[s]))
        fr.demux(whole_file(b[s]))
    assert nflushed > 0


def test_a_flushed_stream_with_a_non_finite_sample(flush_host):
    """tests/test_feed_live_ogg.py's poisoned stream, every stream flushed in every group: the dead stream returns nothing
    and keeps its status; its neighbours' flushed bytes are the host mux's."""
    import vorbis_amd
    _ref()
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(5)
    streams = [s16_streams(rng, 2, 30000, [k])[0].astype(np.float32) / np.float32(32768.0) for k in ["gated", "noise", "sine"]]
    poisoned = streams[1].copy()
    poisoned[17001, 1] = np.nan
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_stereo_q4"), lanes_per_device=1, max_streams=4, max_frames=8000,
                           fmt=vorbis_amd.FEED_F32, write_frames=1024, ogg_headers=headers)
    try:
        got = run_flushed(feed, [streams[0], poisoned, streams[2]], [[5000, 6000, 7000, 8000, 4000]] * 3, [10, 11, 12], lambda r: True)
    finally:
        feed.close()
    for s in (0, 2):
        assert all(g["status"] == 0 for g in got[s])
        pages = hold_against_the_host_mux(flush_host, headers, 10 + s, got[s])
        assert sum(p["flushed"] for p in pages) == 4 and pages[-1]["flags"] & 4
    hit = next(r for r, g in enumerate(got[1]) if any(row[0] is None for row in g["rows"]))
    assert 0 < hit < 4
    for g in got[1][hit:]:
        assert g["bytes"] == b"" and g["npages"] == 0 and g["status"] == vorbis_amd.api.STATUS_NONFINITE
    st = flush_host.stream(headers, 11)
    for g in got[1][:hit]:
        assert g["status"] == 0 and st.piece([r[0] for r in g["rows"]], [r[1] for r in g["rows"]], False, True) == g["bytes"]


def test_streams_that_begin_with_a_flushed_group(flush_host):
    """A stream that begins with a flushed group and has a comment header of its own: header pages, audio pages and the
    flushed page in one range.  One that begins with a piece too short for any packet: its header pages alone."""
    import vorbis_amd
    _ref()
    headers = rh.reference_headers(2, 44100, 0.4)
    own = vorbis_amd.comment_packet([("TITLE", "flushed"), ("COMMENT", "x" * 700)], "vorbis_amd tests")
    rng = np.random.default_rng(31)
    a = s16_streams(rng, 2, 24000, ["noise"])[0]
    b = s16_streams(rng, 2, 6000, ["gated"])[0]
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_stereo_q4"), lanes_per_device=1, max_streams=2, max_frames=24000,
                           write_frames=1024, ogg_headers=headers)
    try:
        got = run_flushed(feed, [a, b], [[20000, 4000], [100, 5900]], [41, 42], lambda r: True, comments=[own, None])
    finally:
        feed.close()
    first = fr.pages_of(got[0][0]["bytes"])
    assert len(got[0][0]["rows"]) > 4 and first[0]["flags"] == 2 and first[-1]["lacing"][-1] < 255 and first[-1]["granule"] == got[0][0]["rows"][-1][1]
    pages = hold_against_the_host_mux(flush_host, [headers[0], own, headers[2]], 41, got[0])
    assert pages[len(first) - 1]["flushed"] and fr.packets_of(first)[:3] == [headers[0], own, headers[2]]
    assert not got[1][0]["rows"], "100 frames gave a packet: the case needs a shorter piece"
    only = fr.pages_of(got[1][0]["bytes"])
    assert got[1][0]["npages"] == len(only) and fr.packets_of(only) == list(headers) and [p["granule"] for p in only] == [0] * len(only)
    assert not any(p["flushed"] for p in hold_against_the_host_mux(flush_host, headers, 42, got[1])[:len(only)])


def test_errors():
    import vorbis_amd
    _ref()
    EINVAL = vorbis_amd.api.VAMD_EINVAL
    blob = vorbis_amd.default_setup_blob("44k_stereo_q4")
    headers = rh.reference_headers(2, 44100, 0.4)
    y = s16_streams(np.random.default_rng(8), 2, 8192, ["noise"])[0]
    x = y[:4096]

    def refused(feed, slot, flags, n, text):
        a = np.ascontiguousarray(flags, dtype=np.uint8)
        r = feed.L.vamd_feed_ogg_flush(feed.h, slot, a.ctypes.data, n)
        assert r == EINVAL and text in feed.L.vamd_feed_last_error(feed.h).decode(), (r, feed.L.vamd_feed_last_error(feed.h))

    whole = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=4096, ogg_headers=headers)
    try:
        slot, buf = whole.buffer(2)
        refused(whole, slot, [1, 1], 2, "live")                          # a whole-stream feed
        with pytest.raises(vorbis_amd.VamdError) as e:
            whole.ogg_flush(slot, [1])
        assert e.value.code == EINVAL
        whole.release(slot)
        assert len(whole.encode_ogg([x])[0]) > 58                         # ... which goes on working
    finally:
        whole.close()
    bare = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=4096, write_frames=1024)
    try:
        slot, buf = bare.buffer(2)
        refused(bare, slot, [1, 1], 2, "no Ogg headers")                  # a live feed without Ogg headers
        bare.release(slot)
        assert len(bare.encode_live([x], [1])[0]) > 0
    finally:
        bare.close()
    live = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=8192, write_frames=1024, ogg_headers=headers)
    try:
        refused(live, 0, [1, 1], 2, "between vamd_feed_buffer and vamd_feed_wrote_live")     # before buffer()
        slot, buf = live.buffer(2)
        refused(live, slot, [1, 1], -1, "max_streams")                    # n < 0
        refused(live, slot, [1, 1, 1], 3, "max_streams")                  # n > max_streams
        assert live.L.vamd_feed_ogg_flush(live.h, 7, None, 1) == EINVAL   # no such slot
        flat = y.reshape(-1)
        buf[:flat.size] = flat
        live.ogg_flush(slot, [1, 1])
        live.ogg_flush(slot, [])                                          # a later call replaces an earlier one: no flush
        live.wrote_live(slot, [8192], [0])
        refused(live, slot, [1], 1, "between vamd_feed_buffer and vamd_feed_wrote_live")     # after wrote
        o = live.ogg(slot)
        assert fr.packets_of(fr.pages_of(bytes(o["bytes"][:int(o["total_bytes"])])))[:3] == list(headers)
        refused(live, slot, [1], 1, "between vamd_feed_buffer and vamd_feed_wrote_live")
        live.release(slot)
        out = live.encode_live_ogg([x[:0]], [0], flush=True)              # the feed is usable: the open page, flushed
        assert len(fr.pages_of(out[0])) == 1 and not fr.pages_of(out[0])[0]["flags"] & 4
        assert live.encode_live_ogg([x[:2000]], [1])[0][-1:] != b""
    finally:
        live.close()
