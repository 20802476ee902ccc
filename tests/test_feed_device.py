"""GPU suite: device-fed groups of the feed (vamd_feed_wrote_device / _wrote_live_device / _source_done / _buffer_on,
VAMD_FEED_NO_ARENA; include/vorbis_amd.h, "device-fed groups") -- streams that already lie in device memory as torch tensors
of any strides, int16 / float32 / float16 / bfloat16 -- against the reference encoder over the float value of every sample
(after rounding to the source type), and against the host-fed feed of the same samples.  Everything is exact equality."""
import hashlib

import numpy as np
import pytest

from tests import bitrate_host as bh
from tests import checker
from tests import feed_source_host as fs
from tests import ref_host as rh
from tests.feed_cases import Q4, diff
from tests.signals import N_HEAD, mixed_streams, random_cuts, s16_streams

pytestmark = pytest.mark.gpu

EINVAL = -131


def _ref():
    from oracle import ref
    if not ref.available():
        pytest.skip("needs the reference build")
    return ref


_WANT = {}


def want_of(setup, planar, managed=None):
    """the reference's packets of one stream, planar float32 [ch, frames]: (bytes, granulepos, W, e_o_s) each; computed once"""
    ref = _ref()
    planar = np.ascontiguousarray(planar, dtype=np.float32)
    key = (setup, managed, planar.shape, hashlib.sha1(planar.tobytes()).hexdigest())
    if key not in _WANT:
        ch, rate, q = checker.SETUPS[setup]
        enc = ref.RefEncoder(ch, rate, managed=managed) if managed else ref.RefEncoder(ch, rate, q)
        _WANT[key] = [(w["packet"], w["granulepos"], w["W"], w["eos"]) for w in enc.encode_stream(planar)]
    return _WANT[key]


def check(setup, floats, got):
    """floats [ns][ch, frames] float32, got: the feed's rows"""
    assert len(got) == len(floats)
    bad = []
    for s, x in enumerate(floats):
        bad += diff(want_of(setup, x), got[s], s)
    assert not bad, "\n".join(bad)


def signals(seed, ch, frames, kinds):
    """-> float32 [ns, ch, frames] in +-1 (the signals of tests/test_feed.py, planar)"""
    x = s16_streams(np.random.default_rng(seed), ch, frames, kinds)
    return np.ascontiguousarray((x.astype(np.float32) / np.float32(32768.0)).transpose(0, 2, 1))


def to_device(dtype, elems):
    """source elements (tests/feed_source_host.py: bf16 as its uint16 bits) -> a torch tensor of the source type on the GPU"""
    import torch
    a = np.ascontiguousarray(elems)
    if dtype == fs.SRC_BF16:
        return torch.from_numpy(a.view(np.int16)).cuda().view(torch.bfloat16)
    return torch.from_numpy(a).cuda()


def feed_of(setup=Q4, **kw):
    import vorbis_amd
    kw.setdefault("lanes_per_device", 1)
    kw.setdefault("max_streams", 8)
    kw.setdefault("max_frames", 30000)
    blob = kw.pop("blob", None)
    return vorbis_amd.Feed(vorbis_amd.default_setup_blob(setup) if blob is None else blob, **kw)


# ---- 1. every dtype against the reference, whole streams ----
@pytest.mark.parametrize("setup", [Q4, "44k_mono_q5"])
@pytest.mark.parametrize("dtype", [fs.SRC_S16, fs.SRC_F32, fs.SRC_F16, fs.SRC_BF16], ids=["s16", "f32", "f16", "bf16"])
def test_every_dtype_matches_the_reference(setup, dtype):
    import vorbis_amd
    ch = checker.SETUPS[setup][0]
    x = signals(2026, ch, 30000, ["noise", "gated", "sine", "clicks", "silence", "gated"])
    elems = fs.from_float(dtype, x)
    floats = fs.to_float(dtype, elems)
    feed = feed_of(setup)
    try:
        got = feed.encode_tensors(to_device(dtype, elems))
    finally:
        feed.close()
    assert all(len(g) > 20 for g in got)
    check(setup, floats, got)
    if dtype in (fs.SRC_S16, fs.SRC_F32):  # ... and what the host-fed feed makes of the same samples
        host = feed_of(setup, fmt=vorbis_amd.FEED_S16 if dtype == fs.SRC_S16 else vorbis_amd.FEED_F32)
        try:
            assert host.encode(np.ascontiguousarray(elems.transpose(0, 2, 1))) == got
        finally:
            host.close()


# ---- 2. small shapes and views ----
@pytest.mark.parametrize("dtype", [fs.SRC_F32, fs.SRC_F16], ids=["f32", "f16"])
@pytest.mark.parametrize("frames", fs.FRAMES)
def test_small_shapes_and_views(frames, dtype):
    """Every layout of tests/feed_source_host.py at every element offset of the base, each one group of three streams: a
    view of one flat device buffer (torch.as_strided: the wrapper reads its strides), the negative frame stride hand-built
    (torch has no negative strides)."""
    import torch
    import vorbis_amd
    rng = np.random.default_rng(frames)
    ns, ch = 3, 2
    x = signals(frames, ch, frames, ["noise", "gated", "sine"])
    elems = fs.from_float(dtype, x)
    floats = fs.to_float(dtype, elems)
    feed = feed_of(max_streams=4, max_frames=8192)
    try:
        for name in fs.LAYOUTS:
            for offset in fs.OFFSETS:
                lay = fs.layout(name, frames, offset, ns, ch)
                host = fs.from_float(dtype, (rng.random(lay["elems"]) - 0.5).astype(np.float32))  # (between the rows: not zeros)
                fs.scatter(host, lay, elems[:, :lay["rows"]])
                flat = to_device(dtype, host)
                if lay["fstride"] >= 0:
                    src = torch.as_strided(flat, (ns, ch, frames), (lay["stream"], lay["cstride"], lay["fstride"]), offset)
                    got = feed.encode_tensors(src)
                else:
                    src = vorbis_amd.DeviceSource([flat.data_ptr() + b * flat.element_size() for b in lay["base"]], dtype, lay["cstride"],
                                                  lay["fstride"], keep=flat)
                    got = feed.encode_tensors(src, frames=[frames] * ns)
                want = floats if lay["rows"] == ch else np.repeat(floats[:, :1], ch, axis=1)
                try:
                    check(Q4, want, got)
                except AssertionError as e:
                    raise AssertionError("layout %s, offset %d: %s" % (name, offset, e))
    finally:
        feed.close()


def test_interleaved_tensor_with_layout_sfc():
    """(streams, frames, channels), as a decoder leaves it: layout="sfc"; frames shorter than the tensor"""
    x = signals(77, 2, 5000, ["gated", "noise"])
    feed = feed_of(max_frames=8192)
    try:
        t = to_device(fs.SRC_F32, np.ascontiguousarray(x.transpose(0, 2, 1)))
        got = feed.encode_tensors(t, frames=[5000, 3001], layout="sfc")
    finally:
        feed.close()
    check(Q4, [x[0], x[1][:, :3001]], got)


# ---- 3. a ragged list of separate allocations ----
def test_ragged_list_of_separate_allocations():
    import torch
    rng = np.random.default_rng(31)
    lengths = [30000, 1, 2049, 17000, 700]
    parts = [s16_streams(rng, 2, n, [k])[0] for n, k in zip(lengths, ["gated", "noise", "sine", "clicks", "noise"])]
    feed = feed_of()
    try:
        want = feed.encode(parts)                                           # (vamd_feed_wrote_v)
        tensors = [torch.from_numpy(p).cuda() for p in parts]               # [frames_s, 2] each, its own allocation
        assert len(set(t.data_ptr() for t in tensors)) == len(tensors)
        got = feed.encode_tensors(tensors, layout="sfc")
        again = feed.encode_tensors([t.T for t in tensors])                 # the same memory as (channels, frames_s) views
        with pytest.raises(ValueError):
            feed.encode_tensors([tensors[0].T, tensors[2].T.contiguous()])  # strides that disagree
        with pytest.raises(ValueError):
            feed.encode_tensors([tensors[0], tensors[2].float()], layout="sfc")
    finally:
        feed.close()
    assert got == want and again == want


# ---- 4. live ----
def f16_streams(rng, ch):
    """tests/signals.py's mixed streams and cuts, their samples rounded to float16: -> (float16 [frames_s, ch] each, cuts)"""
    streams, cuts = mixed_streams(rng, ch)
    return [(x.astype(np.float32) / np.float32(32768.0)).astype(np.float16) for x in streams], cuts


def run_live_mixed(feed, streams16, cuts):
    """Round r of the cuts: even rounds host-fed (float32 through the arena), odd rounds device-fed -- float16 tensors and
    float32 tensors in turn -- on the same streams.  -> per stream its packets over all rounds"""
    got = [[] for _ in streams16]
    pos = [0] * len(streams16)
    for r in range(max(len(c) for c in cuts)):
        pieces, close = [], []
        for s, x in enumerate(streams16):
            n = cuts[s][r] if r < len(cuts[s]) else 0
            pieces.append(x[pos[s]:pos[s] + n])
            pos[s] += n
            close.append(r == len(cuts[s]) - 1)
        if r % 2 == 0:
            rows = feed.encode_live([p.astype(np.float32) for p in pieces], close)
        else:
            dt = fs.SRC_F16 if r % 4 == 1 else fs.SRC_F32
            rows = feed.encode_live_tensors([to_device(dt, p if dt == fs.SRC_F16 else p.astype(np.float32)) for p in pieces], close=close,
                                            layout="sfc")
        for s, row in enumerate(rows):
            got[s] += row
    assert pos == [len(x) for x in streams16]
    return got


def test_live_pieces_from_the_arena_and_from_tensors():
    import vorbis_amd
    ref = _ref()
    rng = np.random.default_rng(9)
    streams16, cuts = f16_streams(rng, 2)
    feed = feed_of(max_frames=32000, fmt=vorbis_amd.FEED_F32, write_frames=1024)
    try:
        got = run_live_mixed(feed, streams16, cuts)
        again = run_live_mixed(feed, streams16, [random_cuts(rng, len(x), [N_HEAD]) for x in streams16])
    finally:
        feed.close()
    bad = []
    for s, x in enumerate(streams16):
        want = [(w["packet"], w["granulepos"], w["W"], w["eos"])
                for w in ref.RefEncoder(2, 44100, 0.4).encode_stream(np.ascontiguousarray(x.astype(np.float32).T), write_frames=1024)]
        bad += diff(want, got[s], s)
    assert not bad, "\n".join(bad)
    assert again == got


# ---- 5. a non-finite float16 sample in a live stream ----
def test_non_finite_f16_sample_ends_its_stream_only():
    """tests/test_feed_live.py::test_non_finite_sample_ends_its_stream_only, the pieces float16 tensors and the sample inf"""
    import vorbis_amd
    rng = np.random.default_rng(5)
    streams = [(s16_streams(rng, 2, 30000, [k])[0].astype(np.float32) / np.float32(32768.0)).astype(np.float16) for k in ["gated", "noise", "sine"]]
    nan_at = 17001
    poisoned = streams[1].copy()
    poisoned[nan_at, 1] = np.inf
    feed = feed_of(max_streams=4, max_frames=8000, fmt=vorbis_amd.FEED_F32, write_frames=1024)
    cuts = [5000, 6000, 7000, 8000, 4000]
    got = [[], [], []]  # (packet tuple, info)
    pos = 0
    try:
        for r, n in enumerate(cuts):
            slot, _ = feed.buffer()
            feed.wrote_live_device(slot, [to_device(fs.SRC_F16, x[pos:pos + n]) for x in (streams[0], poisoned, streams[2])],
                                   close=[r == len(cuts) - 1] * 3, layout="sfc")
            res = feed.packets(slot)
            for s, row in enumerate(vorbis_amd.Feed._rows(res, 3)):
                k0 = int(res["stream_start"][s])
                got[s] += [(g, int(res["info"][k0 + j])) for j, g in enumerate(row)]
            feed.release(slot)
            pos += n
        # the lane's next streams are unaffected
        later = (s16_streams(rng, 2, 8000, ["gated"])[0].astype(np.float32) / np.float32(32768.0)).astype(np.float16)
        after = feed.encode_live_tensors([to_device(fs.SRC_F16, later)] * 3, close=[1, 1, 1], layout="sfc")
    finally:
        feed.close()
    want = [want_of(Q4, x.astype(np.float32).T) for x in streams]
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
    wl = want_of(Q4, later.astype(np.float32).T)
    assert all(not diff(wl, row) for row in after)


# ---- 6. Ogg ----
def test_ogg_files_equal_the_host_fed_groups():
    import torch
    import vorbis_amd
    _ref()
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(61)
    lengths = [30000, 2049, 12000, 1]
    parts = [s16_streams(rng, 2, n, [k])[0] for n, k in zip(lengths, ["gated", "noise", "sine", "clicks"])]
    serials = [70, 7, 700, 7000]
    comments = [vorbis_amd.comment_packet([("TITLE", "one")], "vorbis_amd feed"), None, vorbis_amd.comment_packet([("TITLE", "three"), ("ARTIST", "x" * 300)], "v")]
    feed = feed_of(ogg_headers=headers)
    try:
        want = feed.encode_ogg(parts, serials=serials, comments=comments)
        got = feed.encode_ogg_tensors([torch.from_numpy(p).cuda() for p in parts], serials=serials, comments=comments, layout="sfc")
    finally:
        feed.close()
    assert all(len(f) > 100 for f in want)
    assert got == want


def test_live_ogg_pieces_with_random_flushes_equal_the_host_fed_feeds():
    import vorbis_amd
    _ref()
    headers = rh.reference_headers(2, 44100, 0.4)
    rng = np.random.default_rng(62)
    streams, cuts = mixed_streams(rng, 2)
    rounds = max(len(c) for c in cuts)
    masks = [[bool(rng.integers(0, 3) == 0) for _ in streams] for _ in range(rounds)]
    serials = [11, 22, 33, 44, 55, 66]

    def run(device_fed):
        feed = feed_of(max_frames=32000, write_frames=1024, ogg_headers=headers)
        out, pos = [], [0] * len(streams)
        try:
            for r in range(rounds):
                pieces, close = [], []
                for s, x in enumerate(streams):
                    n = cuts[s][r] if r < len(cuts[s]) else 0
                    pieces.append(x[pos[s]:pos[s] + n])
                    pos[s] += n
                    close.append(r == len(cuts[s]) - 1)
                if device_fed:
                    out.append(feed.encode_live_ogg_tensors([to_device(fs.SRC_S16, p) for p in pieces], close=close, serials=serials,
                                                            flush=masks[r], layout="sfc"))
                else:
                    out.append(feed.encode_live_ogg(pieces, close, serials=serials, flush=masks[r]))
        finally:
            feed.close()
        return out
    want, got = run(False), run(True)
    assert sum(len(b) for row in want for b in row) > 50000
    assert got == want


# ---- 7. managed ----
@pytest.mark.parametrize("slice_", [None, "7"])
def test_managed_group_equals_the_host_fed_one(slice_, monkeypatch):
    """ABR 128 (tests/bitrate_host.py's blob): bytes and choices of the device-fed group are the host-fed group's; the
    reference's packets besides"""
    import torch
    _ref()
    if slice_:
        monkeypatch.setenv("VAMD_TEST_KNOBS", "1")
        monkeypatch.setenv("VAMD_FEED_SLICE", slice_)
    rates = (-1, 128000, -1)
    parts = [np.ascontiguousarray(np.clip(np.round(bh.signal("music", 2, n, 50 + s).T * 32768.0), -32768, 32767).astype(np.int16))
             for s, n in enumerate([30000, 9000, 700])]   # [frames_s, 2], interleaved
    feed = feed_of(blob=bh.managed_blob(2, rates), max_streams=4)
    res = []
    try:
        for device_fed in (False, True):
            slot, buf = feed.buffer(2)
            if device_fed:
                feed.wrote_device(slot, [torch.from_numpy(p).cuda() for p in parts], layout="sfc")
            else:
                flat = np.concatenate([p.reshape(-1) for p in parts])
                buf[:flat.size] = flat
                feed.wrote(slot, len(parts), [len(p) for p in parts])
            res.append(feed.packets(slot))
            feed.release(slot)
    finally:
        feed.close()
    host, dev = res
    for k in ("nstreams", "nblocks", "total_bytes"):
        assert host[k] == dev[k], k
    for k in ("stream_start", "offset", "bits", "granulepos", "info", "choice", "bytes"):
        assert np.array_equal(host[k], dev[k]), k
    assert len(set(dev["choice"].tolist())) > 1 and dev["nblocks"] > 3 * 7
    assert dev["upload_ms"] == 0
    import vorbis_amd
    rows = vorbis_amd.Feed._rows(dev, len(parts))
    bad = []
    for s, p in enumerate(parts):
        bad += diff(want_of(Q4, (p.astype(np.float32) / np.float32(32768.0)).T, managed=rates), rows[s], s)
    assert not bad, "\n".join(bad)


# ---- 8. ordering against the producer ----
def busy(n=16):
    """enough work on torch's current stream that what is enqueued behind it has not started when the host moves on"""
    import torch
    a = torch.ones((8192, 8192), device="cuda")
    for _ in range(n):
        a = (a @ a) * (1.0 / 8192)
    return a


@pytest.mark.parametrize("which", ["side", "default"])
def test_the_ingest_waits_for_the_producer(which):
    import torch
    x = signals(88, 2, 20000, ["gated", "noise", "sine"])
    vals = torch.from_numpy(x).cuda()
    src = torch.zeros_like(vals)
    busy(1)
    torch.cuda.synchronize()
    feed = feed_of()
    side = torch.cuda.Stream()
    filled = torch.cuda.Event()
    try:
        slot, _ = feed.buffer()
        with torch.cuda.stream(side if which == "side" else torch.cuda.default_stream()):
            keep = busy()
            src.copy_(vals)
            filled.record()
        feed.wrote_device(slot, src, stream=side.cuda_stream if which == "side" else 0)
        started = filled.query()
        got = vorbis_amd_rows(feed, slot, 3)
    finally:
        feed.close()
    assert not started, "the source was filled before wrote_device returned: the test shows nothing"
    check(Q4, x, got)
    del keep


def vorbis_amd_rows(feed, slot, ns):
    import vorbis_amd
    try:
        return vorbis_amd.Feed._rows(feed.packets(slot), ns)
    finally:
        feed.release(slot)


# ---- 9. source_done ----
@pytest.mark.parametrize("how", ["host_wait", "consumer_stream"])
def test_source_done_lets_the_source_be_overwritten(how):
    import torch
    import vorbis_amd
    x = signals(99, 2, 20000, ["gated", "noise", "sine"])
    src = torch.from_numpy(x).cuda()
    torch.cuda.synchronize()
    feed = feed_of()
    side = torch.cuda.Stream()
    try:
        slot, _ = feed.buffer()
        feed.wrote_device(slot, src)
        if how == "host_wait":
            feed.source_done(slot, wait=True)
            src.zero_()
            torch.cuda.synchronize()
        else:
            feed.source_done(slot, stream=side.cuda_stream)
            with torch.cuda.stream(side):
                src.zero_()
        got = vorbis_amd_rows(feed, slot, 3)
        torch.cuda.synchronize()
        assert not src.any()
        # a host-fed group has no source to be done with
        slot, buf = feed.buffer(2)
        buf[:8] = 0
        feed.wrote(slot, 1, 4)
        with pytest.raises(vorbis_amd.VamdError) as e:
            feed.source_done(slot)
        assert e.value.code == EINVAL
        feed.packets(slot)
        feed.release(slot)
    finally:
        feed.close()
    check(Q4, x, got)


# ---- 10. a feed without an arena ----
def test_feed_without_arena():
    import vorbis_amd
    x = signals(10, 2, 9000, ["gated", "sine"])
    feed = feed_of(fmt=vorbis_amd.FEED_S16 | vorbis_amd.FEED_NO_ARENA)
    try:
        slot, buf = feed.buffer(2)
        assert buf is None
        for call in (lambda: feed.wrote(slot, 2, 9000), lambda: feed.wrote(slot, 2, [9000, 100])):
            with pytest.raises(vorbis_amd.VamdError) as e:
                call()
            assert e.value.code == EINVAL
        feed.wrote_device(slot, to_device(fs.SRC_F32, x))
        got = vorbis_amd_rows(feed, slot, 2)
    finally:
        feed.close()
    live = feed_of(fmt=vorbis_amd.FEED_F32 | vorbis_amd.FEED_NO_ARENA, write_frames=1024, max_frames=9000)
    try:
        slot, buf = live.buffer(2)
        assert buf is None
        with pytest.raises(vorbis_amd.VamdError) as e:
            live.wrote_live(slot, [100, 100])
        assert e.value.code == EINVAL
        live.release(slot)
        got_live = live.encode_live_tensors(to_device(fs.SRC_F32, x), close=[1, 1])
    finally:
        live.close()
    check(Q4, x, got)
    check(Q4, x, got_live)


# ---- 11. refusals leave the feed usable ----
def test_refusals_leave_the_feed_usable():
    import re
    import torch
    import vorbis_amd
    x = signals(11, 2, 6000, ["gated", "noise"])
    good = torch.from_numpy(x).cuda()
    host_array = np.ascontiguousarray(x)
    pinned = torch.from_numpy(x).pin_memory()
    feed = feed_of(max_frames=8192)
    live = feed_of(max_frames=8192, write_frames=1024)
    S = vorbis_amd.DeviceSource
    p0 = good.data_ptr()
    planar = lambda base, cs=6000, fs_=1, dt=fs.SRC_F32: S([base, base + 2 * 6000 * 4], dt, cs, fs_)

    def refused(f, call):
        with pytest.raises(vorbis_amd.VamdError) as e:
            call()
        assert e.value.code == EINVAL, e.value
        why = f.L.vamd_feed_last_error(f.h).decode()
        assert why, "no reason given"
        return why
    try:
        slot, _ = feed.buffer()
        n = [6000, 6000]
        refused(feed, lambda: feed.wrote_device(slot, planar(host_array.ctypes.data), frames=n))               # host memory
        refused(feed, lambda: feed.wrote_device(slot, planar(pinned.data_ptr()), frames=n))                    # pinned host memory
        refused(feed, lambda: feed.wrote_device(slot, planar(p0, cs=1 << 40), frames=n))                       # a stride out of this world
        refused(feed, lambda: feed.wrote_device(slot, planar(p0, fs_=-(1 << 40)), frames=n))
        refused(feed, lambda: feed.wrote_device(slot, planar(p0, dt=7), frames=n))                             # an unknown dtype
        refused(feed, lambda: feed.wrote_device(slot, planar(p0 + 2), frames=n))                               # half an element
        refused(feed, lambda: feed.wrote_device(slot, S([p0, 0], fs.SRC_F32, 6000, 1), frames=n))              # frames without a pointer
        refused(feed, lambda: feed.wrote_device(slot, planar(p0), frames=[6000, 9000]))                        # longer than the feed holds
        # one element past the allocation: its size from the library's own words
        why = refused(feed, lambda: feed.wrote_device(slot, planar(p0, cs=1 << 40), frames=n))
        m = re.search(r"lies (\d+) bytes into an allocation of (\d+) bytes", why)
        assert m, why
        off, size = int(m.group(1)), int(m.group(2))
        room = (size - off) // 4                      # elements from the first stream's base to the allocation's end
        one = S([p0], fs.SRC_F32, room - 6000 + 1, 1)  # channel 1's row then ends one element past it
        why = refused(feed, lambda: feed.wrote_device(slot, one, frames=[6000]))
        assert "out of range" in why
        refused(feed, lambda: feed.wrote_live_device(slot, good))                                              # a live call on a whole feed
        lslot, _ = live.buffer()
        refused(live, lambda: live.wrote_device(lslot, good))                                                  # ... and the reverse
        refused(live, lambda: live.wrote_live_device(lslot, planar(host_array.ctypes.data), frames=n))
        refused(feed, lambda: feed.buffer_on(torch.cuda.device_count() + 3))                                   # no lane there
        # ... and the slots are still being filled: good groups on the same feeds
        feed.wrote_device(slot, good)
        got = vorbis_amd_rows(feed, slot, 2)
        live.wrote_live_device(lslot, good, close=[1, 1])
        got_live = vorbis_amd_rows(live, lslot, 2)
    finally:
        feed.close()
        live.close()
    check(Q4, x, got)
    check(Q4, x, got_live)


# ---- 12. a lane on the tensor's device ----
def test_buffer_on_the_current_device():
    import torch
    dev = torch.cuda.current_device()
    x = signals(12, 2, 5000, ["noise"])
    feed = feed_of(lanes_per_device=2, max_frames=8192)
    try:
        slot, buf = feed.buffer_on(dev, 2)
        assert feed.device(slot) == dev and buf is not None
        other, _ = feed.buffer_on(dev)
        assert other != slot and feed.device(other) == dev
        feed.release(other)
        feed.wrote_device(slot, to_device(fs.SRC_BF16, fs.from_float(fs.SRC_BF16, x)))
        got = vorbis_amd_rows(feed, slot, 1)
    finally:
        feed.close()
    check(Q4, fs.to_float(fs.SRC_BF16, fs.from_float(fs.SRC_BF16, x)), got)
