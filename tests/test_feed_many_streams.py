"""GPU suite: the feed with groups of hundreds of streams, against the reference encoder (and decoder, and the host mux).

Several parts of the feed change their road with the number of streams in a group, and the other feed tests stay at 16
streams or fewer.  One test per road; each first asserts, from its own inputs and results, that the switch it exists
for is crossed -- against literals (tests/feed_many_cases.py names the source line each mirrors), with no test knob set
-- and then holds every stream's packets (bytes, granule position, size class, end-of-stream flag) to the reference bit
for bit, files byte for byte to the host mux, the decoded signal to the reference decoder.

  a  ~1000 streams of 1 to 9024 frames, 16-bit from host memory, two lanes: k_feed_ingest's second grid trip, both
     detector passes tiled with count_of / first_of, k_feed_scan with two streams a thread
  b  the same count at one length, float input (vamd_feed_wrote): the detector and the ingest without their lists
  c  the benchmark's shape in miniature: first detector pass tiled, second not; more than 2048 blocks of either class
     through vamd_analyze_streams_mixed with per-stream ampmax chains
  d  bitrate-managed: a slice of 2048 blocks that holds 1025 streams, streams cut by slice edges, four slices; and a
     second group whose first stream owns a whole slice
  e  group a as Ogg files: the pager's grids, serial lists and comment tables at ns > 1024
  f  group a through the decoded feed: k_lap beyond its 1024 rows
  h  group a from device memory, one dtype a call (a device-fed group has one frame stride: 1, 2, 3 and 2 over the calls)
  g  299 continuing streams on one live lane, every copy of a stream cut differently, a second batch through the same
     slots; once for packets, once as a live Ogg feed with a flush per write on every fifth stream
  i  the tiled detector on its own (vamd_envelope_search_batch): its flags against the reference's marks, over bursts
     that begin and end on the first step of every tile

A group is D = 23 distinct streams dealt round; the reference runs once per distinct stream and module.

What each id was seen to catch (four value-only mutations of the kernels): profiles/r27_feed_many_streams.txt, section 3."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref
from tests import bitrate_host as bh
from tests import feed_many_cases as mc
from tests import feed_source_host as fs
from tests import ogg_host as oh
from tests.feed_cases import check_file, diff, same_bits
from tests.test_feed_device import to_device
from tests.test_feed_ogg_tags import run_group as run_ogg_group

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref.available(), reason="oracle/_ref is not built (the reference's sources were not there at build time)")]


@pytest.fixture(autouse=True)
def no_test_knobs(monkeypatch):
    """nothing here is forced by a knob, whatever the caller's environment holds (as tests/test_batch_roads.py)"""
    monkeypatch.delenv("VAMD_TEST_KNOBS", raising=False)


def hold(g, got, want, what=""):
    """got: the feed's rows per stream; want: the reference's rows per DISTINCT stream.  Names the stream and the packet."""
    assert len(got) == g.count
    bad = []
    for s, d in enumerate(g.index):
        if got[s] != want[d]:
            bad += ["%s(a copy of distinct stream %d, %d frames) %s" % (what, d, g.frames[s], m) for m in diff(want[d], got[s], s)]
    assert not bad, "%d of %d streams differ\n" % (len(bad), g.count) + "\n".join(bad[:20])


def crossed_by_the_short_group(ns, longest):
    """what ids a, e, f and h assert of their group ahead of everything else"""
    s1, s2 = mc.steps_of(longest)
    assert ns > 1024                                   # k_feed_scan: per = ceil(ns / 1024) >= 2; k_lap's rows
    assert mc.ingest_items(ns, longest) > 2097152      # launch_ingest: 8192 workgroups x 256 threads
    assert ns * s1 > 65536 and ns * s2 > 65536 and s2 == 96   # envelope_search_batch: both passes tiled
    return s1, s2


def vbr_feed(g, **kw):
    import vorbis_amd
    kw.setdefault("lanes_per_device", 1)
    return vorbis_amd.Feed(vorbis_amd.default_setup_blob(g.name), max_streams=g.count, max_frames=max(g.frames), **kw)


# ---- a ----
def test_a_many_short_streams_of_unequal_length_s16():
    g = mc.short_group()
    parts = g.parts()
    crossed_by_the_short_group(len(parts), max(len(p) for p in parts))
    feed = vbr_feed(g, lanes_per_device=2)
    try:
        got = feed.encode(parts)
        again = feed.encode(parts[::-1])[::-1]        # (the same streams in another order, on the other lane)
    finally:
        feed.close()
    hold(g, got, g.rows())
    for s in range(g.count):
        assert again[s] == got[s], "stream %d depends on its place in the group" % s


# ---- b ----
def test_b_many_streams_of_one_length_float():
    import vorbis_amd
    g = mc.uniform_group()
    parts = g.parts(np.float32)
    ns, frames = len(parts), len(parts[0])
    s1, s2 = mc.steps_of(frames)
    assert all(len(p) == frames for p in parts) and frames % 4 != 0
    assert s1 % 32 != 0 and s1 % 64 != 0 and s2 % 64 != 0            # the last detector tile of either pass is ragged
    assert ns > 1024 and mc.ingest_items(ns, frames) > 2097152
    assert ns * s1 > 65536 and ns * s2 > 65536
    feed = vbr_feed(g, fmt=vorbis_amd.FEED_F32)
    try:
        slot, buf = feed.buffer(g.ch)
        try:
            flat = np.concatenate([p.reshape(-1) for p in parts])
            buf[:flat.size] = flat
            feed.wrote(slot, ns, frames)                             # one length: no frames_of, no count_of, no first_of
            got = feed._rows(feed.packets(slot), ns)
        finally:
            feed.release(slot)
    finally:
        feed.close()
    hold(g, got, g.rows())


# ---- c ----
def test_c_the_benchmarks_shape_in_miniature():
    g = mc.bench_group()
    parts = g.parts()
    ns, longest = len(parts), max(len(p) for p in parts)
    s1, s2 = mc.steps_of(longest)
    assert ns * s1 > 65536 and ns * s2 <= 65536 and s2 == 96         # the first pass tiled, the second not
    feed = vbr_feed(g)
    try:
        got = feed.encode(parts)
    finally:
        feed.close()
    nlong = sum(r[2] for row in got for r in row)
    nshort = sum(len(row) for row in got) - nlong
    assert nlong > 2048 and nshort > 2048, (nlong, nshort)           # res_team_max, pack_pair_max: both classes beyond them
    hold(g, got, g.rows())


# ---- d ----
def managed_run(g, rates):
    """one group through a managed feed of its own -> (the group's record, its rows)"""
    import vorbis_amd
    parts = g.parts()
    ns = len(parts)
    feed = vorbis_amd.Feed(bh.managed_blob(g.ch, rates), lanes_per_device=1, max_streams=ns, max_frames=max(g.frames))
    try:
        slot, buf = feed.buffer(g.ch)
        try:
            flat = np.concatenate([p.reshape(-1) for p in parts])
            buf[:flat.size] = flat
            feed.wrote(slot, ns, g.frames)
            r = feed.packets(slot)
            return r, feed._rows(r, ns)
        finally:
            feed.release(slot)
    finally:
        feed.close()


@pytest.mark.parametrize("which", sorted(mc.MANAGED_SETUPS))
def test_d_bitrate_managed(which):
    rates = mc.MANAGED_SETUPS[which][1]
    g = mc.managed_group(which)
    r, got = managed_run(g, rates)
    nslices, most, cut = mc.slices_of(r["stream_start"], 2048)      # feed_slice = 2048 blocks
    assert nslices >= 3, nslices
    assert most > 1024, most                                         # k_feed_scan per slice: two streams a thread
    assert cut, "no stream of three or more packets is cut by a slice edge"
    hold(g, got, g.rows(rates), which + " ")
    # a stream that owns a whole slice: it needs more than 2048 packets, so it comes in a small group of its own
    g = mc.owner_group(which)
    r, got = managed_run(g, rates)
    assert int(r["stream_start"][1]) > 2048                          # slice 0 is the first stream's alone, and its edge cuts it
    assert mc.slices_of(r["stream_start"], 2048)[2] == [0]
    hold(g, got, g.rows(rates), which + " (owner) ")


# ---- e ----
def test_e_ogg_files():
    import vorbis_amd
    g = mc.short_group()
    parts = g.parts()
    ns = len(parts)
    crossed_by_the_short_group(ns, max(len(p) for p in parts))
    headers = g.headers()
    vendor = vorbis_amd.comment_fields(headers[1])[0]
    serials = [(0x9e3779b1 * (s + 1)) & 0xffffffff for s in range(ns)]
    assert len(set(serials)) == ns and all(v != s for s, v in enumerate(serials))
    comments = [vorbis_amd.comment_packet([("TITLE", "stream %d" % s), ("PAD", "x" * (s % 300))], vendor) if s % 3 == 0 else None
                for s in range(ns)]
    feed = vbr_feed(g, ogg_headers=headers)
    try:
        files, rows, o, _ = run_ogg_group(feed, parts, serials, comments)
    finally:
        feed.close()
    hold(g, rows, g.rows())
    host, want = oh.HostOgg(), g.records()
    for s, d in enumerate(g.index):
        assert o["status"][s] == 0, s
        try:
            check_file(host, [headers[0], comments[s] or headers[1], headers[2]], want[d], rows[s], files[s], g.frames[s], serials[s],
                       int(o["npages"][s]))
        except AssertionError as e:
            raise AssertionError("stream %d (a copy of distinct stream %d, %d frames): %s" % (s, d, g.frames[s], e))


# ---- f ----
def test_f_decoded_feed():
    import torch
    import vorbis_amd
    from vorbis_amd.abi import _FeedDecodedResult
    from vorbis_amd.feed import _view
    g = mc.short_group()
    parts = g.parts(np.float32)
    ns = len(parts)
    crossed_by_the_short_group(ns, max(len(p) for p in parts))
    assert ns > 1024                                                 # k_lap strides over the streams beyond its 1024 rows
    assert any(n % 4 for n in g.frames)
    big = torch.from_numpy(np.ascontiguousarray(np.concatenate(parts).T)).cuda()       # [ch, all frames]
    at = np.concatenate([[0], np.cumsum(g.frames)])
    views = [big[:, int(at[s]):int(at[s + 1])] for s in range(ns)]
    feed = vbr_feed(g, fmt=vorbis_amd.FEED_F32, decoded=True)
    try:
        got, dec = feed.roundtrip_tensors(views)
        pcm = [d.cpu().numpy() for d in dec]
        # the record itself (statuses, frames, offsets) is not part of what roundtrip_tensors returns: the same group once more
        slot = feed.buffer()[0]
        try:
            feed.wrote_device(slot, views)
            r = _FeedDecodedResult()
            feed._check(feed.L.vamd_feed_decoded(feed.h, slot, C.byref(r)))
            frames, offset, status = _view(r.frames, C.c_int64, ns, True), _view(r.offset, C.c_int64, ns + 1, True), _view(r.status, C.c_uint8, ns, True)
            assert int(r.nstreams) == ns and int(r.channels) == g.ch and int(r.total_floats) == int(offset[-1])
        finally:
            feed.release(slot)
    finally:
        feed.close()
    hold(g, got, g.rows())
    assert not status.any(), np.flatnonzero(status)[:10]
    assert np.array_equal(frames, g.frames)
    assert np.array_equal(offset, g.ch * at)                         # as planned: back to back, ch * frames floats a stream
    want = g.decoded()
    for s, d in enumerate(g.index):
        mine = pcm[s]
        assert mine.shape == (g.ch, g.frames[s]), (s, mine.shape)
        assert same_bits(mine, want[d]), "stream %d (a copy of distinct stream %d, %d frames): %d samples differ from the reference decoder's" % (
            s, d, g.frames[s], int((mine.view(np.uint32) != want[d].view(np.uint32)).sum()))


# ---- h ----
def device_views(dtype, elems, frames, ch, fstride, rng):
    """Per-stream elements [ch, frames_s] as (ch, frames_s) views of ONE device tensor, at unequal offsets (a gap of 0 to 2
    elements between streams) and a frame stride of `fstride`; what lies between the samples is noise, not zeros."""
    import torch
    gaps = [s % 3 for s in range(len(frames))]
    at = np.concatenate([[0], np.cumsum([fstride * n + k for n, k in zip(frames, gaps)])]).astype(np.int64)
    total = int(at[-1])
    host = fs.from_float(dtype, (rng.random((ch, total)) - 0.5).astype(np.float32))
    for s, x in enumerate(elems):
        host[:, int(at[s]):int(at[s]) + fstride * frames[s]:fstride] = x
    flat = to_device(dtype, host)
    return [torch.as_strided(flat, (ch, frames[s]), (total, fstride), int(at[s])) for s in range(len(frames))]


@pytest.mark.parametrize("dtype,fstride", [(fs.SRC_S16, 1), (fs.SRC_F32, 2), (fs.SRC_F16, 3), (fs.SRC_BF16, 2)], ids=["s16", "f32", "f16", "bf16"])
def test_h_device_fed(dtype, fstride):
    g = mc.short_group()
    ns = g.count
    crossed_by_the_short_group(ns, max(g.frames))
    # the reference sees the values the source type holds (16-bit and float hold the same: x / 32768 is exact in float)
    half = dtype in (fs.SRC_F16, fs.SRC_BF16)
    quantise = ("src%d" % dtype, lambda x: fs.to_float(dtype, fs.from_float(dtype, x))) if half else None
    planar = [np.ascontiguousarray(fs.to_float(fs.SRC_S16, x).T) for x in g.distinct]
    distinct = [fs.from_float(dtype, x) for x in planar]
    views = device_views(dtype, [distinct[d] for d in g.index], g.frames, g.ch, fstride, np.random.default_rng(dtype))
    assert len({v.data_ptr() for v in views}) == ns
    feed = vbr_feed(g)
    try:
        got = feed.encode_tensors(views)
    finally:
        feed.close()
    hold(g, got, g.rows(quantise=quantise))


# ---- g ----
def crossed_by_the_live_cuts(frames, cuts):
    c = mc.live_conditions(frames, cuts)
    assert c["tiled"] > 65536, c                                     # envelope_search_batch: a round's launch is tiled
    assert c["fresh"] >= 1 and len(c["closing"]) >= 3 and c["empty"] and c["single"] and c["ragged"], c
    return c


def test_g_live_feed():
    import vorbis_amd
    from tests.feed_cases import run_live
    g = mc.live_group()
    want = g.rows()
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob(g.name), lanes_per_device=1, max_streams=g.count, max_frames=max(g.frames),
                           write_frames=mc.WRITE_FRAMES)
    try:
        for batch in (0, 1):             # the second batch: fresh streams through the slots the first batch's streams closed
            parts, index = (g.parts(), g.index) if batch == 0 else (g.parts()[::-1], g.index[::-1])
            cuts = mc.live_cuts([len(p) for p in parts], batch)
            crossed_by_the_live_cuts([len(p) for p in parts], cuts)
            got = run_live(feed, parts, cuts)
            bad = []
            for s, d in enumerate(index):
                if got[s] != want[d]:
                    bad += ["batch %d (a copy of distinct stream %d, cut %s) %s" % (batch, d, cuts[s], m) for m in diff(want[d], got[s], s)]
            assert not bad, "%d streams differ\n" % len(bad) + "\n".join(bad[:20])
    finally:
        feed.close()


def test_g_live_ogg_feed():
    import vorbis_amd
    from tests.feed_cases import whole_file
    from tests.test_feed_live_ogg_flush import check_flushed_file, hold_against_the_host_mux, run_flushed
    g = mc.live_group()
    headers, want, rows = g.headers(), g.records(), g.rows()
    ns = g.count
    mask = [s % 5 == 0 for s in range(ns)]                           # a flush per write on every fifth stream
    host, flush_host = oh.HostOgg(), oh.HostOgg()
    nflushed = 0
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob(g.name), lanes_per_device=1, max_streams=ns, max_frames=max(g.frames),
                           write_frames=mc.WRITE_FRAMES, ogg_headers=headers)
    try:
        for batch in (0, 1):             # the second batch: fresh streams, with serial numbers of their own, through the same slots
            parts, index = (g.parts(), g.index) if batch == 0 else (g.parts()[::-1], g.index[::-1])
            frames = [len(p) for p in parts]
            cuts = mc.live_cuts(frames, batch)
            crossed_by_the_live_cuts(frames, cuts)
            # ... some of the flushed streams stay open behind a write that has brought them to 8192 frames, four long blocks:
            # their open page holds packets
            assert sum(mask[s] and any(sum(c[:r + 1]) >= 8192 for r in range(len(c) - 1)) for s, c in enumerate(cuts)) >= 3
            serials = [(0x85ebca6b * (s + 1 + batch * ns)) & 0xffffffff for s in range(ns)]
            got = run_flushed(feed, parts, cuts, serials, lambda r: mask)
            for s, d in enumerate(index):
                try:
                    assert all(x["status"] == 0 for x in got[s])
                    assert [w for x in got[s] for w in x["rows"]] == rows[d], "the packets are not the reference's"
                    assert whole_file(got[s]) == host.mux(headers, [w[0] for w in rows[d]], [w[1] for w in rows[d]], serials[s]) or mask[s], \
                        "the pieces laid end to end are not the host mux of the reference's packets"
                    pages = hold_against_the_host_mux(flush_host, headers, serials[s], got[s])
                    check_flushed_file(host, headers, want[d], got[s], pages, frames[s], serials[s])
                    assert mask[s] or not any(p["flushed"] for p in pages)
                    nflushed += sum(p["flushed"] for p in pages)
                except AssertionError as e:
                    raise AssertionError("batch %d stream %d (a copy of distinct stream %d, cut %s): %s" % (batch, s, d, cuts[s], e))
    finally:
        feed.close()
    # (how many pages each flush closes is held group by group against the host mux above; here only that there were some)
    assert nflushed >= 1, nflushed


# ---- i ----
def test_i_tiled_detector_flags_against_the_references_marks():
    """vamd_envelope_search_batch over 46 streams x 4302 steps, a tiled launch, against the reference's own _ve_envelope_search
    over each stream (ve->mark[]): bursts that begin and end on the first step of a 64-step tile with the stretch at its
    longest, where the trigger reaches back to the oldest row of history k_env_bits_tiled stages."""
    import torch
    import vorbis_amd
    g = mc.sweep_group()
    ns, steps = g.count, g.steps
    assert ns * steps > 65536 and steps % 64 != 0                    # envelope_search_batch: tiled, the last tile ragged
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(g.name), 0)
    need = (steps - 1) * 64 + 128
    pcm = torch.from_numpy(np.stack([g.distinct[d]["pcm"][:, :need] for d in g.index])).cuda()
    flags, _ = an.envelope_search_batch(pcm, steps)
    flags = flags.cpu().numpy()
    for d, o in enumerate(g.distinct):                               # (the reference's marks: what the flags are held to below)
        begins, ends = mc.tile_starts_hit(o["marks"], steps)
        assert begins and ends, "distinct stream %d: no burst begins / ends on a tile's first step" % d
    for s, d in enumerate(g.index):
        marks = vorbis_amd.envelope_marks(flags[s])[:steps + 2]
        want = g.distinct[d]["marks"]
        bad = np.flatnonzero(marks != want)
        assert not bad.size, "stream %d (a copy of distinct stream %d): %d marks differ from the reference's, the first at step %d (step %d of its tile)" % (
            s, d, bad.size, bad[0], bad[0] % 64)
