"""GPU: windows of streams and of Ogg files (vamd_decode_window; vamd_ogg_index_create, vamd_decode_ogg_window;
Analyzer.decode_window, Analyzer.ogg_index, OggIndex.decode / .crops) -- a seek index on the host, then per window only
its own pages up, k_ogg_depage over them, k_unpack, k_synth and k_lap_window -- against libvorbis' decoder over the WHOLE
stream, sliced, bit for bit.  The windows are tests/decode_window_cases.py's edge list; the same windows have been through
the same code on the host in tests/test_decode_window_cpu.py.  Every window of every call is compared."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref
from tests import decode_cases, decode_window_cases as wc, ogg_demux_cases as cases, ref_host
from tests.feed_cases import Q4, same_bits

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")]
EINVAL = -131


def blocksizes(name):
    enc = ref_host.encoder(name)
    return enc.blocksize(0), enc.blocksize(1)


def columns(windows):
    return [w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows]


def check(got, status, windows, wants, what):
    assert len(got) == len(windows) == len(status)
    for w, ((s, start, count), t) in enumerate(zip(windows, got)):
        a, b = wc.cut(start, count, wants[s].shape[1])
        assert t.is_cuda and status[w] == 0 and tuple(t.shape) == (wants[s].shape[0], b - a), (what, w, s, start, count, int(status[w]), tuple(t.shape))
        assert same_bits(t.cpu().numpy(), wants[s][:, a:b]), (what, w, s, start, count)


def edge_list(streams, bs, Ts):
    return [(s, start, count) for s in range(len(streams)) for start, count in wc.edge_windows(streams[s], bs, Ts[s])]


@pytest.mark.parametrize("name", ["44k_stereo_q4", "44k_51_q3"])
def test_edge_windows_of_files(name):
    """the edge windows of the 24 files of a setup, one call through OggIndex.decode"""
    import vorbis_amd
    bs = blocksizes(name)
    blob, headers, _ = cases.base_files(name, "feed")
    files = [f for policy in cases.POLICIES for f in cases.base_files(name, policy)[2]]
    exp = [cases.expected(f) for f in files]
    streams, wants = [e[0] for e in exp], [e[2] for e in exp]
    Ts = [w.shape[1] for w in wants]
    windows = edge_list(streams, bs, Ts)
    an = vorbis_amd.Analyzer(blob)
    try:
        x = an.ogg_index(files, headers[2])
        assert [int(v) for v in x.frames] == Ts and not x.status.any()
        got, status = x.decode(*columns(windows), with_status=True)
        x.close()
    finally:
        an.close()
    check(got, status, windows, wants, name)


def test_edge_windows_of_packets():
    """the same list through Analyzer.decode_window on decode_cases.base_streams"""
    import vorbis_amd
    blob, headers, bs, base = decode_cases.base_streams(Q4, 1)
    streams, ends = [p for p, _ in base], [end for _, end in base]
    wants = [ref_host.reference_decode(headers + p, [-1] * (len(p) - 1) + [end]) for p, end in base]
    windows = edge_list(streams, bs, ends)
    an = vorbis_amd.Analyzer(blob)
    try:
        got, status = an.decode_window(streams, ends, *columns(windows), with_status=True)
        frames, nblocks = np.zeros(len(windows), np.int64), np.zeros(2, np.int64)
        prep = an.decode_prepare(streams, ends)
        cols = [np.array(c, np.int64) for c in columns(windows)]
        vp = C.c_void_p
        assert an.L.vamd_decode_window_plan(an.h, C.byref(prep["desc"]), len(windows), *(vp(c.ctypes.data) for c in cols), vp(frames.ctypes.data),
                                            vp(nblocks.ctypes.data)) == 0
    finally:
        an.close()
    check(got, status, windows, wants, "packets")
    assert [int(n) for n in nblocks] == wc.nblocks_of(streams, bs, ends, windows)
    assert [int(f) for f in frames] == [wc.cut(a, n, ends[s])[1] - wc.cut(a, n, ends[s])[0] for s, a, n in windows]


def test_crops():
    """crops of one length, some cut short by the file's end: the valid part bit-equal, the rest exactly zero, the lengths right"""
    import vorbis_amd
    blob, headers, files = cases.base_files(Q4, "seeded")
    wants = [cases.expected(f)[2] for f in files]
    Ts = [w.shape[1] for w in wants]
    length = 1500
    stream = [0, 1, 2, 3, 0, 1, 2]
    start = [0, Ts[1] - 1500, Ts[2] - 1499, Ts[3] - 1, 4321, Ts[1], Ts[2] + 9]
    an = vorbis_amd.Analyzer(blob)
    try:
        x = an.ogg_index(files, headers[2])
        pcm, valid = x.crops(stream, start, length)
    finally:
        an.close()
    assert tuple(pcm.shape) == (len(stream), wants[0].shape[0], length) and pcm.is_cuda
    assert [int(v) for v in valid] == [1500, 1500, 1499, 1, 1500, 0, 0]
    got = pcm.cpu().numpy()
    for w, (s, a) in enumerate(zip(stream, start)):
        n = int(valid[w])
        assert same_bits(got[w][:, :n], wants[s][:, a:a + n]), w
        assert not got[w][:, n:].view(np.uint32).any(), w


def test_multiple_windows_of_a_stream():
    """ten windows a file in one call, seeded, overlapping and out of order; the module-level entry"""
    import vorbis_amd
    blob, headers, files = cases.base_files(Q4, "shared")
    wants = [cases.expected(f)[2] for f in files]
    rng = np.random.default_rng(30)
    windows = [(s, int(rng.integers(0, wants[s].shape[1])), int(rng.integers(1, 3000))) for _ in range(10) for s in (3, 1, 0, 2)]
    x = vorbis_amd.ogg_index(blob, files, setup_header=headers[2])
    try:
        got, status = x.decode(*columns(windows), with_status=True)
    finally:
        x.close()
    check(got, status, windows, wants, "ten a file")


@pytest.mark.parametrize("name", ["44k_stereo_q4", "44k_51_q3"])
def test_damage(name):
    """tests/test_decode_window_cpu.py::test_damage on the GPU: a window over the page with the flipped bit is BADPAGE and has
    no frames; the windows beside it -- in the same call, of the same file -- are clean"""
    import vorbis_amd
    blob, header, files, want, want1, over, beside = wc.damage_case(name)
    other = (1, 100, 3000)
    an = vorbis_amd.Analyzer(blob)
    try:
        x = an.ogg_index(files, header)
        assert not x.status.any()
        got, status = x.decode(*columns([beside, other]), with_status=True)
        check(got, status, [beside, other], [want, want1], (name, "beside"))
        windows = [beside, over, other, beside]
        got, status = x.decode(*columns(windows), with_status=True)
        whole, whole_status = an.decode_ogg(files, header, with_status=True)
    finally:
        an.close()
    assert status[1] & cases.STATUS_BADPAGE and tuple(got[1].shape) == (want.shape[0], 0)
    keep = [0, 2, 3]
    check([got[i] for i in keep], status[keep], [windows[i] for i in keep], [want, want1], (name, "neighbours"))
    assert whole_status[0] & cases.STATUS_BADPAGE and whole_status[1] == 0  # (what the window beside the page does not see)


def test_context_reuse():
    """a window call, a whole decode_ogg, a larger window call, an empty one and decode_streams in turn on one context: each
    equals the reference, and the whole-file calls what they give on a fresh context"""
    import vorbis_amd
    bs = blocksizes(Q4)
    blob, headers, small = cases.base_files(Q4, "seeded")
    large = [f for policy in cases.POLICIES for f in cases.base_files(Q4, policy)[2]]
    packets = decode_cases.base_streams(Q4, 1)[3]
    exp = [cases.expected(f) for f in large]
    wants = [e[2] for e in exp]
    fresh = vorbis_amd.Analyzer(blob)
    try:
        fresh_ogg = [t.cpu().numpy() for t in fresh.decode_ogg(large)]
    finally:
        fresh.close()
    fresh = vorbis_amd.Analyzer(blob)
    try:
        fresh_packets = [t.cpu().numpy() for t in fresh.decode_streams([p for p, _ in packets], [end for _, end in packets])]
    finally:
        fresh.close()
    an = vorbis_amd.Analyzer(blob)
    try:
        x = an.ogg_index(large, headers[2])
        first = [(0, 1000, 700), (5, 10, 10)]
        check(*x.decode(*columns(first), with_status=True), first, wants, "first")
        whole, st = an.decode_ogg(large, with_status=True)
        assert not st.any() and all(same_bits(t.cpu().numpy(), w) and same_bits(t.cpu().numpy(), f) for t, w, f in zip(whole, wants, fresh_ogg))
        larger = edge_list([e[0] for e in exp], bs, [w.shape[1] for w in wants])
        check(*x.decode(*columns(larger), with_status=True), larger, wants, "larger")
        got, st = x.decode([], [], [], with_status=True)
        assert got == [] and len(st) == 0
        nothing = [(2, 50, 0), (3, 1 << 40, 5)]
        check(*x.decode(*columns(nothing), with_status=True), nothing, wants, "no frames")
        via = an.decode_streams([p for p, _ in packets], [end for _, end in packets])
        assert all(same_bits(t.cpu().numpy(), cases.expected(f)[2]) and same_bits(t.cpu().numpy(), f2) for t, f, f2 in zip(via, small, fresh_packets))
        check(*x.decode(*columns(first), with_status=True), first, wants, "again")
    finally:
        an.close()


def test_changed_file_and_bad_descriptors():
    """an index used with a file of another length is EINVAL; with a flipped body byte of equal length, BADPAGE and no fault;
    with another context's index, EINVAL; the refusals of the window list; and the call after each is correct"""
    import vorbis_amd
    blob, headers, files = cases.base_files(Q4, "one_packet")
    wants = [cases.expected(f)[2] for f in files]
    good = [(0, 100, 500), (3, 4000, 1000), (0, 300, 500)]
    an, other = vorbis_amd.Analyzer(blob), vorbis_amd.Analyzer(blob)
    try:
        x, y = an.ogg_index(files, headers[2]), other.ogg_index(files, headers[2])

        def refused(why, *a, **kw):
            with pytest.raises(vorbis_amd.VamdError) as e:
                x.decode(*a, **kw)
            assert e.value.code == EINVAL and why in str(e.value), str(e.value)
            check(*x.decode(*columns(good), with_status=True), good, wants, ("after", why))

        refused("length", *columns(good), files=[files[0] + b"\0"] + files[1:])
        sizes = np.cumsum([0] + [len(f) for f in files])
        refused("monotone", *columns(good), file_offset=sizes[[0, 2, 1, 3, 4]])
        refused("out of range", [0, 4, 0], [1, 1, 1], [1, 1, 1])
        refused("out of range", [0, -1, 0], [1, 1, 1], [1, 1, 1])
        refused("start", [0, 1, 0], [1, -1, 1], [1, 1, 1])
        refused("count", [0, 1, 0], [1, 1, 1], [1, 1, (1 << 62) + 1])
        # the raw entry: null pointers, a negative count, another context's index
        vp = C.c_void_p
        cols = [np.array(c, np.int64) for c in columns(good)]
        data = np.frombuffer(b"".join(files) + b"\0" * 8, np.uint8)
        frames, status, staged = np.zeros(3, np.int64), np.zeros(3, np.uint8), np.zeros(2, np.int64)
        from vorbis_amd.abi import _OggWindowDesc
        d = _OggWindowDesc(3, *(vp(c.ctypes.data) for c in cols), vp(data.ctypes.data), vp(sizes.astype(np.int64).ctypes.data), None)
        keep = sizes.astype(np.int64)
        d.file_offset = vp(keep.ctypes.data)
        plan = lambda ctx, idx, desc: an.L.vamd_decode_ogg_window_plan(ctx, idx, desc, vp(frames.ctypes.data), None, vp(staged.ctypes.data))
        run = lambda ctx, idx, desc: an.L.vamd_decode_ogg_window(ctx, idx, desc, None, None, vp(status.ctypes.data))
        assert plan(an.h, x.h, C.byref(d)) == 0 and [int(f) for f in frames] == [500, 1000, 500]
        streams = [cases.expected(f)[0] for f in files]
        assert tuple(int(v) for v in staged) == wc.staged_bytes(files, streams, blocksizes(Q4), [w.shape[1] for w in wants], good)
        for call in (plan, run):
            assert call(an.h, x.h, None) == EINVAL and call(an.h, None, C.byref(d)) == EINVAL
            assert call(an.h, y.h, C.byref(d)) == EINVAL and "another context" in an.L.vamd_last_error(an.h).decode()
            for field in ("stream", "start", "count", "bytes", "file_offset"):
                was = getattr(d, field)
                setattr(d, field, None)
                assert call(an.h, x.h, C.byref(d)) == EINVAL, field
                setattr(d, field, was)
            d.nwindows = -1
            assert call(an.h, x.h, C.byref(d)) == EINVAL
            d.nwindows = 3
        assert run(an.h, x.h, C.byref(d)) == EINVAL  # (frames to decode, nowhere to put them)
        out = vp()
        assert an.L.vamd_ogg_index_create(an.h, None, C.byref(out)) == EINVAL and an.L.vamd_ogg_index_create(an.h, C.byref(an.decode_ogg_prepare(files)["desc"]), None) == EINVAL
        check(*x.decode(*columns(good), with_status=True), good, wants, "after the raw refusals")
        # a byte of a page body flipped, the length as it was: the window over that page is flagged, the others are clean
        pages = wc.ogg_framing.demux(files[0])[0]
        where = wc.packet_pages(pages)
        bs = blocksizes(Q4)
        span = wc.blocks_of(cases.expected(files[0])[0], bs, wants[0].shape[1], 100, 500)
        p = pages[where[span[0] + 1][0]]
        at = p["offset"] + 27 + p["nseg"] + p["body"] // 2
        changed = [files[0][:at] + bytes([files[0][at] ^ 0x20]) + files[0][at + 1:]] + files[1:]
        got, st = x.decode(*columns(good), with_status=True, files=changed)
        assert st[0] & cases.STATUS_BADPAGE and tuple(got[0].shape) == (wants[0].shape[0], 0)
        check(got[1:2], st[1:2], good[1:2], wants, "beside the changed page")
        check(*x.decode(*columns(good), with_status=True), good, wants, "the files as they were")
    finally:
        an.close()
        other.close()
