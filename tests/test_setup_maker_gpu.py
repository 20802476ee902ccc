"""GPU: the header-made decoder (vamd_create_decoder; Analyzer.from_headers) under hand-made setups (tests/setup_maker.py)
and the packets written for them (tests/packet_writer.py; tests/test_setup_maker_cpu.py holds every one of them to the
reference first): k_unpack, k_synth / k_synth_values, k_lap and k_lap_window at the shapes no encoder writes, against
libvorbis' decoder under the same headers and against the one-lane host build, bit for bit; the keep policy over cut packets;
and the files, live, live Ogg and window entries against the whole decode."""
import numpy as np
import pytest

from oracle import ref
from tests import decode_live_host as live, ogg_demux_cases, ogg_framing, setup_maker, unpack_partial_host as partial
from tests.feed_cases import same_bits

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")]

NAMES, get, host_decode = setup_maker.NAMES, setup_maker.get, setup_maker.host_decode
GPU_SEEDS = tuple("seed%d" % s for s in range(8))
ENTRIES = ("equal_2048", "far_64_4096", "one_mode_short", "eight_ch_max")


@pytest.fixture(scope="module")
def exe():
    from tests import hostbuild
    return hostbuild.program("decode_headers_host.cpp")


def analyzer(c, keep=False):
    import vorbis_amd
    a = vorbis_amd.Analyzer.from_headers(c.headers[0], c.headers[2])
    a.keep_partial = keep
    assert (a.channels, tuple(a.blocksizes)) == (c.channels, tuple(c.bs))
    return a


@pytest.mark.parametrize("name", NAMES + GPU_SEEDS)
def test_streams_equal_the_reference_and_the_host_build(exe, tmp_path, name):
    c = get(name)
    a = analyzer(c)
    try:
        got, status = a.decode_streams(c.streams, None, with_status=True)
        got = [g.cpu().numpy() for g in got]
    finally:
        a.close()
    host, _, _ = host_decode(exe, tmp_path, c, c.streams)
    for s, packets in enumerate(c.streams):
        want = setup_maker.reference(c, packets)
        assert status[s] == 0 and got[s].shape == want.shape, (name, s, int(status[s]), got[s].shape, want.shape)
        assert same_bits(got[s], want), (name, s, int((got[s].view(np.uint32) != want.view(np.uint32)).sum()))
        assert host[s][0] == 0 and same_bits(got[s], host[s][1])


def test_eight_channels_of_4096_fit_a_workgroups_lds(exe, tmp_path):
    """the largest demand of synth_lds_words, taken from the library's own code (the host program prints
    4 * synth_lds_words(ch, n2, ch, Bound::res_off_ints) per size class): 135 168 bytes for a long block, below what the
    device gives a workgroup (hipDeviceProp_t::sharedMemPerBlock, which the context takes as its lds_per_block) -- and the
    block decodes: a stream of long blocks mostly"""
    import torch
    c = get("eight_ch_max")
    s = max(range(len(c.streams)), key=lambda s: sum(c.size_classes(s)))
    host_decode(exe, tmp_path, c, [c.streams[s]])
    (_, lds1), (_, off1) = host_decode.lds
    limit = torch.cuda.get_device_properties(0).shared_memory_per_block
    assert off1 == 4081 and lds1 == setup_maker.synth_lds_bytes(8, 2048, off1) == 135168 < limit, (host_decode.lds, limit)
    a = analyzer(c)
    try:
        got, status = a.decode_streams([c.streams[s]], None, with_status=True)
        assert status[0] == 0 and same_bits(got[0].cpu().numpy(), setup_maker.reference(c, c.streams[s]))
        assert a.L.vamd_residue_capacity(a.h, 1) > 0
    finally:
        a.close()


@pytest.mark.parametrize("name", NAMES)
def test_cut_packets_under_the_keep_policy(name):
    c = get(name)
    streams = setup_maker.keep_streams(c)
    a = analyzer(c, keep=True)
    try:
        got, status = a.decode_streams(streams, None, with_status=True)
        got = [g.cpu().numpy() for g in got]
    finally:
        a.close()
    for s, packets in enumerate(streams):
        want = setup_maker.reference(c, packets)
        assert status[s] == partial.STATUS_PARTIAL, (name, s, len(packets[1]), int(status[s]))
        assert got[s].shape == want.shape and same_bits(got[s], want), (name, s, len(packets[1]), got[s].shape, want.shape)


# ---- the other entries ----
def lengths(c):
    """the frames of each stream with no end granule: its last block centre"""
    return [c.centres(s)[-1] for s in range(len(c.streams))]


def files_of(c):
    """a file per stream under four paging policies.  (ogg_demux_cases.packet_granules reads a packet's size class from
    its mode bit; a one-mode setup has none, and every block is a short one: it is given the short size twice)"""
    bs = c.bs if len(c.M.S["modes"]) == 2 else (c.bs[0], c.bs[0])
    return [ogg_demux_cases.make(c.headers, p, T, bs, ("one_packet", "seeded", "shared", "full_255")[s], s) for s, (p, T) in enumerate(zip(c.streams, lengths(c)))]


def windows_of(c, s):
    """[(start, count)] of stream s: from a block centre to one frame before the next centre and to the next centre itself,
    at a step from a long block to a short one and at one back (at a change of mode where the sizes are equal; at any
    block where there is one mode); and windows that lie across those centres"""
    C = c.centres(s)
    kinds = [n["mode"] for n in c.notes[s]]
    out = []
    for pair in ((1, 0), (0, 1)) if len(c.M.S["modes"]) == 2 else ((0, 0),):
        k = next(k for k in range(1, len(C) - 1) if (kinds[k - 1], kinds[k]) == pair)
        out += [(C[k], C[k + 1] - C[k] - 1), (C[k], C[k + 1] - C[k]), (C[k - 1] + 1, C[k + 1] - C[k - 1] - 2), (C[k] - 1, 2)]
    return out


@pytest.mark.parametrize("name", ENTRIES)
def test_files_live_and_windows_equal_the_whole_decode(name):
    import vorbis_amd
    c = get(name)
    T, files = lengths(c), files_of(c)
    n = len(c.streams)
    a = analyzer(c)
    try:
        whole = [t.cpu().numpy() for t in a.decode_streams(c.streams, T)]
        for s in range(n):
            assert whole[s].shape == (c.channels, T[s]) and same_bits(whole[s], setup_maker.reference(c, c.streams[s])), (name, s)
        # whole files, through this context and through contexts made from the files' own headers
        got, status = a.decode_ogg(files, with_status=True)
        assert not status.any() and all(same_bits(g.cpu().numpy(), w) for g, w in zip(got, whole)), (name, list(status))
        assert all(same_bits(ogg_demux_cases.expected(f)[2], w) for f, w in zip(files, whole))
        got, status = vorbis_amd.decode_ogg_files(files, with_status=True)
        assert not status.any() and all(same_bits(g.cpu().numpy(), w) for g, w in zip(got, whole)), (name, list(status))
        # a live decoder in three pieces
        dec = a.live_decoder(n)
        calls, who = live.rounds(c.streams, [[len(p) // 3, 2 * len(p) // 3] for p in c.streams], T, None)
        res = []
        for slots, pieces, close, granules in calls:
            got, status = dec.write(slots, pieces, close, granules, with_status=True)
            res.append([(int(status[i]), got[i].cpu().numpy()) for i in range(len(got))])
        for s, ((st, pcm), w) in enumerate(zip(live.join(res, who, n, c.channels), whole)):
            assert st == 0 and pcm.shape == w.shape and same_bits(pcm, w), (name, "live", s, st)
        # a live Ogg decoder with a cut inside a page
        f = files[1]
        pages = ogg_framing.demux(f)[0]
        cut = pages[len(pages) // 2]["offset"] + pages[len(pages) // 2]["bytes"] // 2
        odec = a.live_ogg_decoder(1)
        p1, s1 = odec.write([0], [f[:cut]], with_status=True)
        p2, s2 = odec.write([0], [f[cut:]], close=[0], with_status=True)
        joined = np.concatenate([p1[0].cpu().numpy(), p2[0].cpu().numpy()], axis=1)
        assert not s1.any() and not s2.any() and same_bits(joined, whole[1]), (name, "live ogg", list(s1), list(s2))
        # windows of the packet streams and of the files
        wins = [(s, start, count) for s in range(n) for start, count in windows_of(c, s)]
        cols = [[w[k] for w in wins] for k in range(3)]
        got, status = a.decode_window(c.streams, T, *cols, with_status=True)
        for (s, start, count), g, st in zip(wins, got, status):
            assert st == 0 and count > 0 and same_bits(g.cpu().numpy(), whole[s][:, start:start + count]), (name, "window", s, start, count, int(st))
        x = a.ogg_index(files)
        got, status = x.decode(*cols, with_status=True)
        x.close()
        for (s, start, count), g, st in zip(wins, got, status):
            assert st == 0 and same_bits(g.cpu().numpy(), whole[s][:, start:start + count]), (name, "index", s, start, count, int(st))
    finally:
        a.close()
