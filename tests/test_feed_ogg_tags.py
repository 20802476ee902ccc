"""GPU suite: a comment header of its own per stream of an Ogg feed (vamd_feed_ogg_comments, include/vorbis_amd.h) -- the
comment goes to the device with its group and is paged there (vorbis_amd/csrc/k_ogg.h).  The oracle for every file is the
shipped host mux given that stream's own three headers; every file is also taken apart by the independent demuxer
(tests/ogg_framing.py), which must return the stream's comment as packet 1 and the reference encoder's packets behind the
headers, decoded by the reference, and its three headers read by the reference's vorbis_synthesis_headerin, whose
vorbis_comment_query must hand the tags back."""
import numpy as np
import pytest

from tests import ogg_framing as fr
from tests import ogg_host as oh
from tests import ref_host as rh
from tests.feed_cases import check_file, planar, reference_records, small_arena, spy_totals
from tests.signals import s16_streams, sized_comment

pytestmark = pytest.mark.gpu

SETUP = "44k_stereo_q4"
KINDS = ["noise", "gated", "sine", "clicks", "silence", "gated", "noise"]
FRAMES = [2049, 7777, 3000, 4097, 5555, 6001, 2500]
SHARED_TAGS = [("ENCODER", "vorbis_amd feed")]          # (tests/ref_host.py, reference_headers' default)


def _ref():
    from oracle import ref
    if not ref.available():
        pytest.skip("needs the reference build")
    return ref


@pytest.fixture(scope="module")
def host():
    return oh.HostOgg()


class World:
    """The seven streams, the reference's packets of each (computed once), the feed's three headers and the seven comments
    of the first case: None (the shared one), the smallest a comment header can be, 255 bytes, the length whose segments
    fill page 1 to exactly 255 together with the setup header's, one segment more, 65 026 bytes (255 segments and one:
    continued onto a second page) and 200 000 bytes."""

    def __init__(self, ref):
        import vorbis_amd
        self.ref = ref
        self.headers = rh.reference_headers(2, 44100, 0.4)
        self.vendor = vorbis_amd.comment_fields(self.headers[1])[0]
        rng = np.random.default_rng(1311)
        self.streams = [s16_streams(rng, 2, n, [k])[0] for n, k in zip(FRAMES, KINDS)]
        self.want = [reference_records(ref, 2, 0.4, x) for x in self.streams]
        self.serials = [1000 + s for s in range(len(self.streams))]
        setup_segs = len(self.headers[2]) // 255 + 1
        self.fill = (254 - setup_segs) * 255 + 100           # its 255 - setup_segs segments and the setup's make 255
        self.smallest = (vorbis_amd.comment_packet([], ""), "", [])
        self.comments = [None, self.smallest] + [self.sized(n, "stream %d" % (2 + i)) for i, n in
                                                 enumerate((255, self.fill, self.fill + 255, 65026, 200000))]

    def sized(self, nbytes, title):
        packet, tags = sized_comment(nbytes, title, self.vendor)
        return packet, self.vendor, tags

    @staticmethod
    def packet(c):
        return None if c is None else c[0]

    def check(self, host, s, c, f, rows, status, npages, want=None):
        """stream s's file f, made with comment c (None: the shared one)"""
        packet, vendor, tags = (self.headers[1], self.vendor, SHARED_TAGS) if c is None else c
        headers = [self.headers[0], packet, self.headers[2]]
        assert status == 0
        pages = check_file(host, headers, self.want[s] if want is None else want, rows, f, self.streams[s].shape[0], self.serials[s], npages)
        got_vendor, count, values = rh.reference_tags(fr.demux(f)[1][:3], sorted({k for k, _ in tags}))
        assert got_vendor == vendor.encode() and count == len(tags)
        for k in values:
            assert values[k] == [v.encode() for kk, v in tags if kk == k], "stream %d: vorbis_comment_query(%s)" % (s, k)
        return pages


@pytest.fixture(scope="module")
def world():
    return World(_ref())


def run_group(feed, parts, serials, comments=None):
    """One group through an Ogg feed -> (files, packet rows, the ogg() record, the slot it went through)"""
    parts = [np.ascontiguousarray(x, dtype=feed.dtype) for x in parts]
    slot, buf = feed.buffer(parts[0].shape[1])
    try:
        flat = np.concatenate([x.reshape(-1) for x in parts])
        buf[:flat.size] = flat
        feed.ogg_serials(slot, serials)
        if comments is not None:
            feed.ogg_comments(slot, comments)
        feed.wrote(slot, len(parts), [x.shape[0] for x in parts])
        o = feed.ogg(slot)
        r = feed.packets(slot)
    finally:
        feed.release(slot)
    off = o["stream_offset"]
    assert o["nstreams"] == len(parts) and off[0] == 0 and off[-1] == o["total_bytes"]
    return [bytes(o["bytes"][int(off[s]):int(off[s + 1])]) for s in range(len(parts))], feed._rows(r, len(parts)), o, slot


def make_feed(world, **kw):
    import vorbis_amd
    args = dict(lanes_per_device=2, max_streams=8, max_frames=max(FRAMES), ogg_headers=world.headers)
    args.update(kw)
    return vorbis_amd.Feed(vorbis_amd.default_setup_blob(SETUP), **args)


@pytest.fixture(scope="module")
def groups(world):
    """Four groups through one feed of two lanes: the seven streams with the seven comments; the same triples in reverse
    order (the other lane); the streams again WITHOUT the call (the first lane again); and with comments for the first
    three streams only."""
    packets = [World.packet(c) for c in world.comments]
    feed = make_feed(world)
    try:
        a = run_group(feed, world.streams, world.serials, packets)
        b = run_group(feed, world.streams[::-1], world.serials[::-1], packets[::-1])
        c = run_group(feed, world.streams, world.serials)
        d = run_group(feed, world.streams, world.serials, [packets[6], packets[5], packets[2]])
    finally:
        feed.close()
    return a, b, c, d


def test_sizes_where_lacing_and_continuation_can_go_wrong(host, world, groups):
    files, rows, o, _ = groups[0]
    pages = [world.check(host, s, world.comments[s], files[s], rows[s], o["status"][s], int(o["npages"][s])) for s in range(7)]
    for p in pages:
        assert p[0]["bytes"] == 58 and p[0]["done"] == 1          # page 0 stays the identification page
    assert len(world.smallest[0]) == 16 and len(world.comments[2][0]) == 255
    header_pages = [next(i for i in range(len(p)) if sum(q["done"] for q in p[:i + 1]) == 3) + 1 for p in pages]
    assert header_pages == [2, 2, 2, 2, 3, 3, 5]
    assert pages[0][1]["done"] == 2 and pages[1][1]["done"] == 2 and pages[2][1]["done"] == 2
    # comment + setup fill page 1 to exactly 255 segments: it is closed there, complete, and the audio starts on page 2
    assert (pages[3][1]["nseg"], pages[3][1]["done"], pages[3][2]["flags"] & 1) == (255, 2, 0)
    # one segment more: page 1 is cut at 255 segments inside the setup header, whose last segment is page 2, continued
    assert (pages[4][1]["nseg"], pages[4][1]["done"]) == (255, 1) and (pages[4][2]["flags"], pages[4][2]["nseg"], pages[4][2]["done"]) == (1, 1, 1)
    # 65 026 bytes are 256 segments: page 1 is all comment and completes nothing, page 2 continues it
    assert (pages[5][1]["nseg"], pages[5][1]["done"], pages[5][1]["granule"], pages[5][1]["body"]) == (255, 0, -1, 65025)
    assert pages[5][2]["flags"] == 1 and pages[5][2]["done"] == 2
    # 200 000 bytes are 785 segments: three full pages and the rest with the setup header
    assert [(p["nseg"], p["done"]) for p in pages[6][1:4]] == [(255, 0)] * 3 and [p["flags"] for p in pages[6][2:5]] == [1, 1, 1]
    assert pages[6][4]["done"] == 2


def test_a_file_depends_neither_on_its_place_in_the_group_nor_on_the_lane(world, groups):
    (files, _, _, slot_a), (again, _, _, slot_b) = groups[0], groups[1]
    assert slot_a != slot_b
    for s in range(7):
        assert again[::-1][s] == files[s], "stream %d's file depends on its place in the group or on the lane" % s


def test_a_group_paged_twice(world, groups, monkeypatch):
    """The packet arena starts at 4096 bytes, so the group is laid out and paged a second time, the arena and its mirror
    grown in between: the comments are still there for the second paging."""
    small_arena(monkeypatch, "4096")
    feed = make_feed(world, lanes_per_device=1)
    totals = spy_totals(feed)
    try:
        files, _, o, _ = run_group(feed, world.streams, world.serials, [World.packet(c) for c in world.comments])
    finally:
        feed.close()
    assert len(totals) == 1 and totals[0] > 4096, totals
    assert all(int(v) == 0 for v in o["status"])
    assert files == groups[0][0]


def test_comments_do_not_stick(host, world, groups):
    a, _, c, d = groups
    assert c[3] == a[3], "the third group must go through the lane the first one took"
    for s in range(7):                                             # made without the call: the shared comment in every file
        world.check(host, s, None, c[0][s], c[1][s], c[2]["status"][s], int(c[2]["npages"][s]))
    assert c[0][0] == a[0][0] and all(c[0][s] != a[0][s] for s in range(1, 7))
    given = [world.comments[6], world.comments[5], world.comments[2]]
    for s in range(7):                                             # n = 3 of 7 streams: streams 3 .. carry the shared one
        world.check(host, s, given[s] if s < 3 else None, d[0][s], d[1][s], d[2]["status"][s], int(d[2]["npages"][s]))
    assert d[0][3:] == c[0][3:]


def test_live(host, world):
    """Three lane slots in 1 024-frame pieces.  Slot 0's stream begins in round 0, slot 1's in round 1 (with the 65 026-byte
    comment), slot 2's in round 2; slot 1's is closed in round 3 and the slot begun again in round 5 with another stream
    and another comment.  In every round every slot is handed a comment: it counts where a stream begins, and is a decoy
    (the 200 000-byte one) for a stream already open."""
    ref = world.ref
    decoy = World.packet(world.comments[6])
    # (slot, first round, stream, comment)
    plan = [(0, 0, 1, world.comments[2]), (1, 1, 2, world.comments[5]), (2, 2, 3, world.comments[3]), (1, 5, 0, world.sized(300, "begun again"))]
    pieces_of = lambda s: -(-FRAMES[s] // 1024)
    assert plan[1][1] + pieces_of(2) <= plan[3][1], "slot 1's first stream must be closed before its second begins"
    rounds = max(r0 + pieces_of(s) for _, r0, s, _ in plan)
    got = {i: dict(bytes=[], rows=[], npages=0) for i in range(len(plan))}
    feed = make_feed(world, lanes_per_device=1, max_streams=4, max_frames=1024, write_frames=1024)
    try:
        for r in range(rounds):
            frames, close, flat, comments, serials, who = [0] * 3, [0] * 3, [np.zeros(0, np.int16)] * 3, [decoy] * 3, [0] * 3, [None] * 3
            for i, (slot, r0, s, c) in enumerate(plan):
                k = r - r0
                if 0 <= k < pieces_of(s):
                    x = world.streams[s][1024 * k:1024 * (k + 1)]
                    frames[slot], close[slot], flat[slot], who[slot], serials[slot] = x.shape[0], k == pieces_of(s) - 1, x.reshape(-1), i, world.serials[s]
                    if k == 0:
                        comments[slot] = World.packet(c)
            slot, buf = feed.buffer(2)
            try:
                f = np.concatenate(flat)
                buf[:f.size] = f
                feed.ogg_serials(slot, serials)
                feed.ogg_comments(slot, comments)
                feed.wrote_live(slot, frames, close)
                o = feed.ogg(slot)
                p = feed.packets(slot)
            finally:
                feed.release(slot)
            off, rows = o["stream_offset"], feed._rows(p, 3)
            assert o["nstreams"] == 3 and off[-1] == o["total_bytes"]
            for t in range(3):
                piece = bytes(o["bytes"][int(off[t]):int(off[t + 1])])
                assert len(fr.pages_of(piece)) == int(o["npages"][t]) and o["status"][t] == 0
                if who[t] is None:
                    assert piece == b"" and not rows[t]
                else:
                    got[who[t]]["bytes"].append(piece)
                    got[who[t]]["rows"] += rows[t]
                    got[who[t]]["npages"] += int(o["npages"][t])
    finally:
        feed.close()
    whole = make_feed(world, lanes_per_device=1)
    try:
        files = whole.encode_ogg([world.streams[s] for _, _, s, _ in plan], serials=[world.serials[s] for _, _, s, _ in plan],
                                 comments=[World.packet(c) for _, _, _, c in plan])
    finally:
        whole.close()
    for i, (slot, r0, s, c) in enumerate(plan):
        f = b"".join(got[i]["bytes"])
        want = ref.RefEncoder(2, 44100, 0.4).encode_stream(planar(world.streams[s]), write_frames=1024)
        pages = world.check(host, s, c, f, got[i]["rows"], 0, got[i]["npages"], want=want)
        assert f == files[i], "stream %d: the pieces are not the whole-stream Ogg feed's file" % s
        if s == 2:                                                   # the 65 026-byte comment: continued onto a second page
            assert (pages[1]["nseg"], pages[1]["done"]) == (255, 0) and pages[2]["flags"] == 1
        # all header pages leave with the group that begins the stream
        first = fr.pages_of(got[i]["bytes"][0])
        assert sum(p["done"] for p in first) >= 3 and first[0]["flags"] == 2


def test_a_stream_with_a_nan_and_a_comment_of_its_own(host, world):
    import vorbis_amd
    pcm = [x.astype(np.float32) / np.float32(32768.0) for x in world.streams[:3]]
    pcm[1] = pcm[1].copy()
    pcm[1][4000, 0] = np.nan
    comments = [world.comments[3], world.comments[5], world.comments[2]]
    feed = make_feed(world, lanes_per_device=1, fmt=vorbis_amd.FEED_F32)
    try:
        files, rows, o, _ = run_group(feed, pcm, world.serials[:3], [World.packet(c) for c in comments])
    finally:
        feed.close()
    assert files[1] == b"" and o["npages"][1] == 0 and o["status"][1] == vorbis_amd.api.STATUS_NONFINITE
    assert any(r[0] is None for r in rows[1])
    for s in (0, 2):
        world.check(host, s, comments[s], files[s], rows[s], o["status"][s], int(o["npages"][s]))


def test_errors(host, world):
    import vorbis_amd
    EINVAL = vorbis_amd.api.VAMD_EINVAL
    good = World.packet(world.comments[2])

    def refused(feed, slot, comments):
        with pytest.raises(vorbis_amd.VamdError) as e:
            feed.ogg_comments(slot, comments)
        assert e.value.code == EINVAL
        text = str(e.value).split(": ", 1)[1]
        assert "vamd_feed_ogg_comments" in text
        return text
    plain = make_feed(world, lanes_per_device=1, ogg_headers=None)
    try:
        slot, _ = plain.buffer(2)
        assert "Ogg" in refused(plain, slot, [good])                 # a plain packet feed
        plain.release(slot)
    finally:
        plain.close()
    feed = make_feed(world, lanes_per_device=1, max_streams=4)
    try:
        refused(feed, 0, [good])                                     # before buffer
        slot, buf = feed.buffer(2)
        refused(feed, slot, [good] * 5)                              # n > max_streams
        text = refused(feed, slot, [good, None, good[:-3], good[:5]])  # a truncated packet at index 2
        assert "stream 2" in text and "stream 3" not in text
        parts = world.streams[:3]
        flat = np.concatenate([x.reshape(-1) for x in parts])
        buf[:flat.size] = flat
        feed.ogg_serials(slot, world.serials[:3])
        feed.wrote(slot, 3, [x.shape[0] for x in parts])
        refused(feed, slot, [good])                                  # after wrote
        o, r = feed.ogg(slot), feed.packets(slot)
        refused(feed, slot, [good])                                  # ... and after the group is done
        feed.release(slot)
    finally:
        feed.close()
    # nothing of the malformed call was kept: the group, written without comments, carries the shared one everywhere
    off, rows = o["stream_offset"], feed._rows(r, 3)
    for s in range(3):
        world.check(host, s, None, bytes(o["bytes"][int(off[s]):int(off[s + 1])]), rows[s], o["status"][s], int(o["npages"][s]))
