"""GPU: the keep policy (vamd_decode_partial; Analyzer.keep_partial) -- k_unpack_partial and the bounded k_synth forms in
place of k_unpack / k_synth, through every decode entry -- against libvorbis' decoder over the same packets and against the
one-lane host build of the same code (tests/test_unpack_partial_cpu.py has taken every case through it), bit for bit."""
import numpy as np
import pytest

from oracle import ref
from tests import decode_partial_cases as cases
from tests import ogg_demux_cases, unpack_partial_host as host
from tests.feed_cases import same_bits
from tests.unpack_partial_host import STATUS_PARTIAL, STATUS_TRUNCATED

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")]


@pytest.fixture(scope="module")
def exe():
    return host.build()


def analyzer(S=None, headers=None, keep=True):
    import vorbis_amd
    an = vorbis_amd.Analyzer.from_headers(headers[0], headers[2]) if headers is not None else vorbis_amd.Analyzer(S.blob)
    an.keep_partial = keep
    assert an.keep_partial == keep
    return an


def assert_streams(got, status, want, flags, what):
    assert len(got) == len(want)
    for s, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy()
        assert status[s] == flags[s], (what, s, status[s], flags[s])
        assert g.shape == w.shape and same_bits(g, w), (what, s, g.shape, w.shape)


def assert_host(exe, exe_setup, tmp_path, streams, got, status, ch):
    """the device against the host build on every stream: the same statuses, the same samples"""
    res = host.host_streams(exe, tmp_path, exe_setup, streams, [-1] * len(streams), ch, keep=1)
    assert len(res) == len(got)
    for s, (st, pcm) in enumerate(res):
        g = got[s].cpu().numpy()
        assert status[s] == st and g.shape == pcm.shape and same_bits(g, pcm), (s, status[s], st)


@pytest.mark.parametrize("context", ["blob", "headers"])
def test_every_cut_of_two_stereo_streams(exe, tmp_path, context):
    """a stream per cut in one decode call; the second time on a context made from the stream's own headers"""
    S, streams, want = cases.cut_streams()
    an = analyzer(S, S.headers if context == "headers" else None)
    try:
        got, status = an.decode_streams(streams, None, with_status=True)
    finally:
        an.close()
    assert_streams(got, status, want, [STATUS_PARTIAL] * len(streams), context)
    assert_host(exe, host.setup_args(tmp_path, blob=S.blob), tmp_path, streams, got, status, S.channels)


def test_streams_with_cut_packets():
    S, streams, ends, damaged, want = cases.damaged_streams()
    an = analyzer(S)
    try:
        got, status = an.decode_streams(streams, ends, with_status=True)
    finally:
        an.close()
    assert_streams(got, status, want, [STATUS_PARTIAL if d else 0 for d in damaged], "streams")


def test_a_value_list_setup(exe, tmp_path):
    hv, streams, want = cases.value_list_streams()
    an = analyzer(headers=hv)
    try:
        got, status = an.decode_streams(streams, None, with_status=True)
    finally:
        an.close()
    assert_streams(got, status, want, [STATUS_PARTIAL] * len(streams), "value lists")
    assert_host(exe, host.setup_args(tmp_path, headers=hv), tmp_path, streams, got, status, 2)


@pytest.mark.parametrize("name,kind", [("44k_stereo_q4", "spare_phrase"), ("44k_51_q3", "spare_phrase"), ("44k_stereo_q4", "empty_phrase"),
                                       ("44k_stereo_q4", "empty_floor"), ("44k_stereo_q4", "empty_value")])
def test_stops_that_leave_the_reader_alone(exe, tmp_path, name, kind):
    """rewritten headers (decode_partial_cases.rewritten_headers): a phrase word beyond the classes, books without used entries.
    Each genuine or bit-flipped packet between two whole ones as a stream of its own: the statuses and samples are the host
    build's, and every stream it does not flag is reference_decode's (a value book without used entries flags: BADCODE)"""
    hv, bs, ch, packets, classes = cases.rewritten_cases(name, kind)
    anchor = next(p for p, (r, _) in zip(packets, classes) if r == 0 and (p[0] >> 1) & 1)
    streams = [[anchor, p, anchor] for p, (r, _) in zip(packets, classes) if r == 0]
    an = analyzer(headers=hv)
    try:
        got, status = an.decode_streams(streams, None, with_status=True)
    finally:
        an.close()
    assert_host(exe, host.setup_args(tmp_path, headers=hv), tmp_path, streams, got, status, ch)
    kept = 0
    for s, packets_ in enumerate(streams):
        if int(status[s]) & ~STATUS_PARTIAL:
            assert kind == "empty_value" and int(status[s]) & host.STATUS_BADCODE and tuple(got[s].shape) == (ch, 0), (s, status[s])
            continue
        want = cases.ref_host.reference_decode(list(hv) + packets_, [-1] * 3)
        g = got[s].cpu().numpy()
        assert g.shape == want.shape and same_bits(g, want), s
        kept += 1
    assert kept >= 10 and sum(int(v) == STATUS_PARTIAL for v in status) >= (3 if kind == "empty_value" else 10)


def four_streams():
    """two clean streams and two with cut packets (one in the middle; two in one stream) -> (setup, packets, ends, flags, want)"""
    S, streams, ends, damaged, want = cases.damaged_streams()
    pick = [0, 3, 2, 6]
    return S, [streams[s] for s in pick], [ends[s] for s in pick], [STATUS_PARTIAL if damaged[s] else 0 for s in pick], [want[s] for s in pick]


def test_files():
    S, streams, ends, flags, want = four_streams()
    files = [ogg_demux_cases.make(S.headers, p, e, S.bs, ("one_packet", "seeded", "shared", "full_255")[s], s) for s, (p, e) in enumerate(zip(streams, ends))]
    an = analyzer(S)
    try:
        got, status = an.decode_ogg(files, with_status=True)
    finally:
        an.close()
    assert_streams(got, status, want, flags, "files")


def test_live_packets_in_three_pieces():
    """the cut packet in the middle piece: the slot stays alive, and the pieces laid end to end are the whole stream"""
    S, streams, ends, flags, want = four_streams()
    thirds = [(len(p) // 3, 2 * len(p) // 3) for p in streams]
    an = analyzer(S)
    try:
        dec = an.live_decoder(4)
        parts, seen = [[] for _ in streams], []
        for r in range(3):
            pieces = [p[(0, a, b)[r]:(a, b, len(p))[r]] for p, (a, b) in zip(streams, thirds)]
            got, status = dec.write([0, 1, 2, 3], pieces, close=[0, 1, 2, 3] if r == 2 else (), end_granules=ends if r == 2 else None,
                                    with_status=True)
            seen.append([int(v) for v in status])
            for s, g in enumerate(got):
                parts[s].append(g.cpu().numpy())
    finally:
        an.close()
    assert seen[1] == flags and seen[2] == [0, 0, 0, 0] and seen[0] == [0, 0, 0, STATUS_PARTIAL], seen  # (stream 3's first cut is packet 1)
    for s, w in enumerate(want):
        assert all(p.shape[1] > 0 for p in parts[s][1:])  # alive behind the cut packet
        g = np.concatenate(parts[s], axis=1)
        assert g.shape == w.shape and same_bits(g, w), (s, g.shape, w.shape)


def test_live_files_in_byte_pieces():
    S, streams, ends, flags, want = four_streams()
    files = [ogg_demux_cases.make(S.headers, p, e, S.bs, "seeded", 40 + s) for s, (p, e) in enumerate(zip(streams, ends))]
    step = 997
    an = analyzer(S)
    try:
        dec = an.live_ogg_decoder(4)
        parts, seen = [[] for _ in files], [0] * len(files)
        for r in range(max((len(f) + step - 1) // step for f in files)):
            live = [s for s, f in enumerate(files) if r * step < len(f)]
            got, status = dec.write(live, [files[s][r * step:(r + 1) * step] for s in live], close=[s for s in live if (r + 1) * step >= len(files[s])],
                                    with_status=True)
            for s, g, st in zip(live, got, status):
                parts[s].append(g.cpu().numpy())
                seen[s] |= int(st)
    finally:
        an.close()
    assert seen == flags, seen
    for s, w in enumerate(want):
        g = np.concatenate(parts[s], axis=1)
        assert g.shape == w.shape and same_bits(g, w), (s, g.shape, w.shape)


def test_a_window_that_straddles_the_cut_block():
    S, streams, ends, flags, want = four_streams()
    # stream 1's cut packet is its middle one; the frames around that block's centre, and the same frames of a clean stream
    gr = ogg_demux_cases.packet_granules(streams[1], ends[1], S.bs)
    mid = len(streams[1]) // 2
    start, count = gr[mid - 1] - 300, gr[mid] - gr[mid - 1] + 600
    assert 0 < start and start + count < ends[1]
    an = analyzer(S)
    try:
        got, status = an.decode_window(streams, ends, [1, 0, 3], [start, start, 0], [count, count, ends[3]], with_status=True)
    finally:
        an.close()
    assert [int(v) for v in status] == [STATUS_PARTIAL, 0, STATUS_PARTIAL], status
    for g, (s, a, n) in zip(got, [(1, start, count), (0, start, count), (3, 0, ends[3])]):
        assert same_bits(g.cpu().numpy(), want[s][:, a:a + n]), s


def test_a_window_of_indexed_files():
    """vamd_decode_ogg_window under the policy: the same windows out of an index of the four streams' files"""
    S, streams, ends, flags, want = four_streams()
    files = [ogg_demux_cases.make(S.headers, p, e, S.bs, "seeded", 60 + s) for s, (p, e) in enumerate(zip(streams, ends))]
    gr = ogg_demux_cases.packet_granules(streams[1], ends[1], S.bs)
    mid = len(streams[1]) // 2
    start, count = gr[mid - 1] - 300, gr[mid] - gr[mid - 1] + 600
    an = analyzer(S)
    try:
        index = an.ogg_index(files)
        assert [int(v) for v in index.status] == [0, 0, 0, 0]
        got, status = index.decode([1, 0, 3], [start, start, 0], [count, count, ends[3]], with_status=True)
    finally:
        an.close()
    assert [int(v) for v in status] == [STATUS_PARTIAL, 0, STATUS_PARTIAL], status
    for g, (s, a, n) in zip(got, [(1, start, count), (0, start, count), (3, 0, ends[3])]):
        assert same_bits(g.cpu().numpy(), want[s][:, a:a + n]), s


def test_the_setting_is_per_context_and_reversible():
    S, streams, ends, flags, want = four_streams()
    an, other = analyzer(S, keep=False), analyzer(S, keep=False)
    try:
        assert an.keep_partial is False
        res = []
        for keep in (True, False, True):
            an.keep_partial = keep
            assert an.keep_partial is keep and other.keep_partial is False
            res.append(an.decode_streams(streams, ends, with_status=True))
    finally:
        an.close()
        other.close()
    for (got, status), keep in zip(res, (True, False, True)):
        if keep:
            assert_streams(got, status, want, flags, "on")
        else:
            assert [int(v) for v in status] == [STATUS_TRUNCATED if f else 0 for f in flags], status
            for g, w, f in zip(got, want, flags):
                assert tuple(g.shape) == (2, 0) if f else same_bits(g.cpu().numpy(), w)
