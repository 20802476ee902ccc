"""CPU: the window decoder (vamd_decode_window, vamd_ogg_index_create, vamd_decode_ogg_window) for one lane on the host --
tests/c/decode_window_host.cpp, a program of its own built with -fsanitize=address,undefined and run as a child process:
the shipped scan, seek index, window plan and staging layout, the staging gather, k_ogg_depage's body, unpack_packet,
synth_block and the window's lap body.  Every window is held, bit for bit (floats as bit patterns), against libvorbis'
decoder over the WHOLE stream, sliced (ogg_demux_cases.expected(f)[2][:, a:b]; Group.want() for packet groups); the blocks
taken and the bytes staged against what tests/decode_window_cases.py works out from the mode bits and the pages."""
import numpy as np
import pytest

from oracle import ref
from tests import decode_cases, decode_window_cases as wc, ogg_demux_cases as cases, ogg_framing, ref_host, synth_host
from tests.feed_cases import Q4, same_bits
from tests.signals import gated_noise

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")
SETUPS = ["44k_stereo_q4", "44k_51_q3"]
_made = []


@pytest.fixture(scope="module")
def exe():
    return wc.build()


def blocksizes(name):
    enc = ref_host.encoder(name)
    return enc.blocksize(0), enc.blocksize(1)


def check_windows(res, windows, wants, what):
    """every window of a call that ran: clean, and the whole decode's frames [a, b)"""
    assert res is not None and len(res["windows"]) == len(windows), what
    for w, ((s, start, count), (status, pcm)) in enumerate(zip(windows, res["windows"])):
        a, b = wc.cut(start, count, wants[s].shape[1])
        assert status == 0 and pcm.shape == (wants[s].shape[0], b - a), (what, w, s, start, count, status, pcm.shape)
        assert same_bits(pcm, wants[s][:, a:b]), (what, w, s, start, count, int((pcm.view(np.uint32) != wants[s][:, a:b].view(np.uint32)).sum()))


@pytest.mark.parametrize("name", SETUPS)
def test_edge_windows_of_files(exe, tmp_path, name):
    """the four base files under the six policies behind one index, a call per policy with every file's edge windows"""
    bs, ch = blocksizes(name), synth_host.SETUPS[name][0]
    blob, headers, _ = cases.base_files(name, "feed")
    files = [f for policy in cases.POLICIES for f in cases.base_files(name, policy)[2]]
    exp = [cases.expected(f) for f in files]
    streams, wants = [e[0] for e in exp], [e[2] for e in exp]
    Ts = [w.shape[1] for w in wants]
    calls = []
    for g in range(len(cases.POLICIES)):
        calls.append([(s, start, count) for s in range(4 * g, 4 * g + 4) for start, count in wc.edge_windows(streams[s], bs, Ts[s])])
    assert all(any(wc.blocks_of(streams[s], bs, Ts[s], a, n) is None for s, a, n in c) and (c[0][0], 0, Ts[c[0][0]]) in c for c in calls)
    info, res = wc.run_ogg(exe, tmp_path, blob, files, headers[2], [wc.call(c) for c in calls], [len(c) for c in calls], ch)
    assert info == [(0, T) for T in Ts]
    for g, (c, r) in enumerate(zip(calls, res)):
        check_windows(r, c, wants, (name, cases.POLICIES[g]))
        assert r["nblocks"] == wc.nblocks_of(streams, bs, Ts, c), (name, g)
        assert (r["staged"], r["rows"]) == wc.staged_bytes(files, streams, bs, Ts, c), (name, g)


def all_transitions():
    """two gated-noise streams of 0.3 and 0.5 s that have, between them, long/long, long/short, short/long and short/short
    -> (blob, headers, bs, [packets], [end granule], [the reference's samples])"""
    if not _made:
        headers = ref_host.encoder_headers(ref_host.encoder(Q4))
        rows = []
        for i, sec in enumerate((0.3, 0.5)):
            enc = ref_host.encoder(Q4)
            recs = enc.encode_stream(gated_noise(enc.channels, enc.rate, int(enc.rate * sec) + 7 * i, 21 + i))
            packets, granules = [r["packet"] for r in recs], [r["granulepos"] for r in recs]
            want = ref_host.reference_decode(headers + packets, granules)
            want.setflags(write=False)
            rows.append((packets, granules[-1], want))
        bs = blocksizes(Q4)
        assert set().union(*(wc.transitions(r[0], bs) for r in rows)) == {(0, 0), (0, 1), (1, 0), (1, 1)}
        _made.append((ref_host.encoder(Q4).pack_setup(), headers, bs) + tuple(list(col) for col in zip(*rows)))
    return _made[0]


def test_all_four_transitions(exe, tmp_path):
    """the edge windows at every size-class transition, through both entries (the base streams have three of the four)"""
    blob, headers, bs, streams, ends, wants = all_transitions()
    ch = wants[0].shape[0]
    Ts = [w.shape[1] for w in wants]
    windows = [(s, start, count) for s in range(2) for start, count in wc.edge_windows(streams[s], bs, Ts[s])]
    files = [cases.make(headers, p, end, bs, "seeded", s) for s, (p, end) in enumerate(zip(streams, ends))]
    info, (res,) = wc.run_ogg(exe, tmp_path, blob, files, headers[2], [wc.call(windows)], [len(windows)], ch)
    check_windows(res, windows, wants, "files")
    assert res["nblocks"] == wc.nblocks_of(streams, bs, Ts, windows)
    assert (res["staged"], res["rows"]) == wc.staged_bytes(files, streams, bs, Ts, windows)
    (pres,) = wc.run_packets(exe, tmp_path, blob, streams, ends, [wc.call(windows)], [len(windows)], ch)
    check_windows(pres, windows, wants, "packets")
    assert pres["nblocks"] == res["nblocks"]


@pytest.mark.parametrize("group", ["end_granules", "short_streams"])
def test_edge_windows_of_packets(exe, tmp_path, group):
    """decode_cases.end_granules() and short_streams(24) through the packet entry: the end granule's cut is the window's T"""
    g = decode_cases.end_granules() if group == "end_granules" else decode_cases.short_streams(24)
    bs = blocksizes(g.name)
    wants = [g.want(s) for s in range(len(g.streams))]
    Ts = [w.shape[1] for w in wants]
    windows = [(s, start, count) for s in range(len(g.streams)) for start, count in wc.edge_windows(g.streams[s], bs, Ts[s])]
    whole = [(s, 0, Ts[s]) for s in range(len(g.streams))]
    res = wc.run_packets(exe, tmp_path, g.blob, g.streams, g.ends, [wc.call(windows), wc.call(whole)], [len(windows), len(whole)], g.channels)
    check_windows(res[0], windows, wants, group)
    check_windows(res[1], whole, wants, group + " whole")
    assert res[0]["nblocks"] == wc.nblocks_of(g.streams, bs, Ts, windows)
    packed = sum(len(g.streams[s][k]) for s, a, n in windows for span in [wc.blocks_of(g.streams[s], bs, Ts[s], a, n)] if span
                 for k in range(span[0], span[1] + 1))
    assert res[0]["staged"] == packed


def test_short_files(exe, tmp_path):
    """short_streams(24) as files: one-frame streams, streams of two packets"""
    g = decode_cases.short_streams(24)
    bs = blocksizes(g.name)
    files = cases.group_files(g, "one_packet")
    exp = [cases.expected(f) for f in files]
    streams, wants = [e[0] for e in exp], [e[2] for e in exp]
    Ts = [w.shape[1] for w in wants]
    assert tuple(Ts[:8]) == tuple(synth_host.SHORT_LENGTHS)
    windows = [(s, start, count) for s in range(len(files)) for start, count in wc.edge_windows(streams[s], bs, Ts[s])]
    info, (res,) = wc.run_ogg(exe, tmp_path, g.blob, files, None, [wc.call(windows)], [len(windows)], g.channels)
    check_windows(res, windows, wants, "short files")
    assert res["nblocks"] == wc.nblocks_of(streams, bs, Ts, windows)
    assert (res["staged"], res["rows"]) == wc.staged_bytes(files, streams, bs, Ts, windows)


def test_streams_without_frames(exe, tmp_path):
    """the files the host's walk flags (ogg_demux_cases.damaged): T = 0, their windows are empty and carry the stream's bits,
    take no block and no byte; the clean files among them decode"""
    d = cases.damaged(Q4)
    ch = synth_host.SETUPS[Q4][0]
    windows = [(s, a, n) for s in range(len(d.files)) for a, n in ((0, 0), (0, 5), (5, 700))]
    info, (res,) = wc.run_ogg(exe, tmp_path, d.blob, d.files, d.setup_header, [wc.call(windows)], [len(windows)], ch)
    host_found = 0
    for (s, a, n), (status, pcm) in zip(windows, res["windows"]):
        if info[s][0]:
            host_found += 1
            assert info[s][0] & d.bit[s] and info[s][1] == 0 and status == info[s][0] and pcm.shape == (ch, 0), (s, d.kind[s])
        elif d.kind[s] is None:
            want = cases.expected(d.files[s])[2]
            lo, hi = wc.cut(a, n, want.shape[1])
            assert status == 0 and same_bits(pcm, want[:, lo:hi]), (s, a, n)
    assert host_found >= 3 * 8  # (the container's structure and the headers: most kinds of damage are the host's to find)


@pytest.mark.parametrize("name", SETUPS)
def test_damage(exe, tmp_path, name):
    """a page whose body has a flipped bit: a window beside it is clean; a window over it is BADPAGE, and its neighbour in the
    same call is clean (the deliberate deviation: a whole decode of the file flags the stream)"""
    blob, header, files, want, want1, over, beside = wc.damage_case(name)
    ch = synth_host.SETUPS[name][0]
    other = (1, 100, 3000)
    calls = [[beside, other], [beside, over, other, beside]]
    info, res = wc.run_ogg(exe, tmp_path, blob, files, header, [wc.call(c) for c in calls], [len(c) for c in calls], ch)
    assert [st for st, _ in info] == [0, 0]  # (a checksum is the device's to find: the index is clean)
    check_windows(res[0], calls[0], [want, want1], (name, "beside"))
    status, _ = res[1]["windows"][1]
    assert status & cases.STATUS_BADPAGE, status
    keep = [0, 2, 3]
    check_windows(dict(windows=[res[1]["windows"][i] for i in keep]), [calls[1][i] for i in keep], [want, want1], (name, "neighbours"))


def test_bad_descriptors(exe, tmp_path):
    """each refused descriptor gives no result, and the call after it is correct"""
    blob, headers, files = cases.base_files(Q4, "seeded")
    ch = synth_host.SETUPS[Q4][0]
    wants = [cases.expected(f)[2] for f in files]
    good = [(0, 100, 500), (3, 4000, 1000), (0, 300, 500)]
    sizes = [0] + [int(v) for v in np.cumsum([len(f) for f in files])]
    top = 1 << 62
    cols = lambda **kw: [kw.get("stream", [0, 3, 0]), kw.get("start", [100, 4000, 300]), kw.get("count", [500, 1000, 500])]
    longer = [files[0] + b"\0"] + files[1:]
    bad = [wc.call(good, null=wc.NULL_STREAM), wc.call(good, null=wc.NULL_START), wc.call(good, null=wc.NULL_COUNT), wc.call(good, null=wc.NULL_BYTES),
           wc.call(good, null=wc.NULL_FILE_OFFSET), wc.call(-1, columns=cols()),
           wc.call(good, columns=cols(stream=[0, 4, 0])), wc.call(good, columns=cols(stream=[0, -1, 0])),
           wc.call(good, columns=cols(start=[100, -1, 300])), wc.call(good, columns=cols(count=[500, 1000, -1])),
           wc.call(good, columns=cols(start=[100, top + 1, 300])), wc.call(good, columns=cols(count=[top + 1, 1000, 500])),
           wc.call(good, file_offset=[sizes[0], sizes[2], sizes[1], sizes[3], sizes[4]]), wc.call(good, file_offset=[-1] + sizes[1:]),
           wc.call(good, file_offset=sizes[:4] + [sizes[4] - 1]), wc.call(good, files=longer)]
    calls, nwindows = [], []
    for b in bad:
        calls += [b, wc.call(good)]
        nwindows += [3, 3]
    calls.append(wc.call([(1, top, top)]))  # (the largest a window may name: empty, and no overflow)
    nwindows.append(1)
    info, res = wc.run_ogg(exe, tmp_path, blob, files, headers[2], calls, nwindows, ch)
    for i in range(len(bad)):
        assert res[2 * i] is None, i
        check_windows(res[2 * i + 1], good, wants, ("after", i))
    assert res[-1]["windows"][0][0] == 0 and res[-1]["windows"][0][1].shape == (ch, 0) and res[-1]["staged"] == 0
    # the packet entry's window list
    g = decode_cases.short_streams(8)
    pw = [(1, 0, 50), (7, 10, 100)]
    pbad = [wc.call(pw, null=wc.NULL_STREAM), wc.call(-1, columns=[[1, 7], [0, 10], [50, 100]]), wc.call(pw, columns=[[1, 8], [0, 10], [50, 100]]),
            wc.call(pw, columns=[[1, 7], [0, -10], [50, 100]]), wc.call(pw, columns=[[1, 7], [0, 10], [top + 1, 100]])]
    pres = wc.run_packets(exe, tmp_path, g.blob, g.streams, g.ends, pbad + [wc.call(pw)], [2] * len(pbad) + [2], g.channels)
    assert all(r is None for r in pres[:-1])
    check_windows(pres[-1], pw, [g.want(s) for s in range(8)], "packets after refusals")
