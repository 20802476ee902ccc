"""GPU: the live Ogg decoder (vamd_decode_ogg_live_*; Analyzer.live_ogg_decoder, LiveOggDecoder.write) -- continuing Ogg
Vorbis streams decoded in pieces of bytes cut anywhere: the page walk's state per slot on the host, a divided page held
there, the packet that whole pages leave open carried on the device (k_ogg_packet_carry_in ahead of k_ogg_depage,
k_ogg_packet_carry_out behind it), the lap carried as the live packet decoder carries it.  A stream's pieces laid end to
end are held, bit for bit, against libvorbis' decoder over the WHOLE stream (tests/ogg_demux_cases.expected) and against
Analyzer.decode_ogg of the whole file.  The cuts are the ones tests/test_demux_live_cpu.py takes through the same code on
the host.  Every stream of every case is compared, or has its flagged status asserted."""
import numpy as np
import pytest

from oracle import ref
from tests import decode_cases, demux_live_host as H, ogg_demux_cases as cases, ogg_framing, ref_host, synth_host
from tests.feed_cases import Q4, same_bits

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")]


def analyzer(blob):
    import vorbis_amd
    return vorbis_amd.Analyzer(blob)


def run_calls(an, dec, calls):
    """calls as (slots, pieces, close) through LiveOggDecoder.write -> per call [(status, samples on the host)]"""
    res = []
    for slots, pieces, close in calls:
        got, status = dec.write(slots, pieces, close, with_status=True)
        assert len(got) == len(slots) and all(t.is_cuda and t.device.index == an.device and t.shape[0] == an.channels for t in got)
        res.append([(int(status[i]), got[i].cpu().numpy()) for i in range(len(got))])
    return res


def join(res, who, n, ch):
    status, parts = [0] * n, [[np.zeros((ch, 0), np.float32)] for _ in range(n)]
    for rows, live in zip(res, who):
        assert len(rows) == len(live)
        for i, (st, pcm) in zip(live, rows):
            status[i] |= st
            parts[i].append(pcm)
    return [(status[i], np.concatenate(parts[i], axis=1)) for i in range(n)]


def run_rounds(an, dec, files, cut_lists, slots=None):
    calls, who = H.rounds(files, cut_lists, slots)
    return join(run_calls(an, dec, calls), who, len(files), an.channels)


def assert_files(an, got, files, what):
    """each stream against the reference decoder over the whole file and against decode_ogg of the whole file"""
    whole, status = an.decode_ogg(files, with_status=True)
    assert len(got) == len(files)
    for s, ((st, pcm), f) in enumerate(zip(got, files)):
        want = cases.expected(f)[2]
        assert st == 0 and status[s] == 0, (what, s, st, status[s])
        assert pcm.shape == want.shape, (what, s, pcm.shape, want.shape)
        assert same_bits(pcm, want), (what, s, int((pcm.view(np.uint32) != want.view(np.uint32)).sum()))
        assert same_bits(pcm, whole[s].cpu().numpy()), (what, s)


def page_ends(f):
    return [p["offset"] + p["bytes"] for p in ogg_framing.demux(f)[0]]


@pytest.mark.parametrize("name", synth_host.FEED_SETUPS)
def test_four_slots_in_pieces_of_997_bytes(name):
    """four files of one policy each on four slots: they end at different calls, so later calls name fewer slots (the one with
    the comment header of 131 000 bytes goes on alone for a hundred calls)"""
    files = [cases.base_files(name, p)[2][i] for i, p in enumerate(("feed", "big_comment", "shared", "singles"))]
    blob = cases.base_files(name, "feed")[0]
    an = analyzer(blob)
    try:
        dec = an.live_ogg_decoder(4)
        calls, who = H.rounds(files, [H.every(f, 997) for f in files], [2, 0, 3, 1])
        assert len({len(w) for w in who}) > 1
        assert_files(an, join(run_calls(an, dec, calls), who, 4, an.channels), files, name)
    finally:
        an.close()


def test_a_packet_open_across_three_pieces():
    """a piece per page of a file with a segment a page: the 5.1 setup's packets of 510 bytes and more are left open by two
    whole pages (carry -> arena -> carry); then the cuts a few bytes off the page ends, the held tail and the carry at once"""
    name = "44k_51_q3"
    blob, _, files = cases.base_files(name, "singles")
    f = files[0]
    assert max(len(p) for p in cases.expected(f, decode=False)[0]) >= 510
    ends = page_ends(f)
    an = analyzer(blob)
    try:
        dec = an.live_ogg_decoder(2, max_packet_bytes=510)  # (exactly what the longest open packet takes)
        for shift in (0, -1, 5):
            got = run_rounds(an, dec, [f], [[e + shift for e in ends[:-1]]], [1])
            assert_files(an, got, [f], ("a piece per page", shift))
        # one byte less: flagged on the host when the open packet reaches 510 bytes, dead until the closing piece
        small = an.live_ogg_decoder(2, max_packet_bytes=509)
        calls, who = H.rounds([f], [ends[:-1]], [1])
        status = [r[0][0] for r in run_calls(an, small, calls)]
        first = status.index(cases.STATUS_BADPAGE)
        assert first > 0 and status == [0] * first + [cases.STATUS_BADPAGE] * (len(status) - first)
        assert_files(an, run_rounds(an, small, [files[1]], [[]], [1]), [files[1]], "the slot's next stream, in one piece")
    finally:
        an.close()


def test_one_byte_pieces_and_closing_variants():
    """a byte a call through the headers and the first two audio pages; the stream closed with its last bytes, closed later
    with an empty piece, and -- without the end-of-stream flag -- closed with the piece that holds its last packet"""
    blob, headers, files = cases.base_files(Q4, "shared")
    f = files[2]
    pages = ogg_framing.demux(f)[0]
    audio = [p for i, p in enumerate(pages) if sum(q["done"] for q in pages[:i + 1]) > 3]
    upto = audio[1]["offset"] + audio[1]["bytes"] + 3
    an = analyzer(blob)
    try:
        dec = an.live_ogg_decoder(1, setup_header=headers[2])
        assert_files(an, run_rounds(an, dec, [f], [list(range(1, upto + 1))]), [f], "one-byte pieces")
        rng = np.random.default_rng(29)
        for k in range(4):
            cuts = H.random_cuts(len(f), rng)
            pieces = H.pieces_of(f, cuts)
            calls = [([0], [p], []) for p in pieces] + [([0], [b""], [0])]
            assert_files(an, join(run_calls(an, dec, calls), [[0]] * len(calls), 1, 2), [f], ("closed later", cuts))
            assert_files(an, run_rounds(an, dec, [f], [cuts]), [f], ("closed with the last piece", cuts))
        last = pages[-1]
        g = cases.reseal(f[:last["offset"] + 5] + bytes([f[last["offset"] + 5] & ~4]) + f[last["offset"] + 6:], last["offset"])
        assert_files(an, run_rounds(an, dec, [g], [[1234, 1234, len(g) - 600]]), [g], "no end-of-stream flag")
        # another setup header than the streams': flagged when the third header packet completes
        other = an.live_ogg_decoder(1, setup_header=headers[2][:-1] + bytes([headers[2][-1] ^ 1]))
        status = [r[0][0] for r in run_calls(an, other, H.rounds([f], [H.every(f, 2000)])[0])]
        assert status[-1] == cases.STATUS_BADHEADER and cases.STATUS_BADHEADER in status[:-1]
    finally:
        an.close()


def test_a_damaged_stream_beside_three_clean_ones():
    """a body bit flipped in piece 2 of 4 on slot 2: piece 1 stands, pieces 2 to 4 have no frames and carry BADPAGE; the
    neighbours are untouched; the slot then takes a clean stream"""
    blob, _, files = cases.base_files(Q4, "one_packet")
    f = files[2]
    pages = ogg_framing.demux(f)[0]
    a0 = next(p for i, p in enumerate(pages) if sum(q["done"] for q in pages[:i]) >= 3)["offset"]  # the first audio page
    cuts = [a0 + k * (len(f) - a0) // 4 for k in (1, 2, 3)]
    page = next(p for p in pages if p["offset"] >= cuts[0] + 50)  # a page that lies in piece 2
    assert page["offset"] + page["bytes"] < cuts[1] and page["body"] > 100
    at = page["offset"] + 27 + page["nseg"] + page["body"] // 2
    bad = f[:at] + bytes([f[at] ^ 0x20]) + f[at + 1:]
    group = [files[0], files[1], bad, files[3]]
    an = analyzer(blob)
    try:
        dec = an.live_ogg_decoder(4)
        calls, who = H.rounds(group, [cuts] * 4)
        res = run_calls(an, dec, calls)
        status = [r[2][0] for r in res]
        first = next(k for k, v in enumerate(status) if v)
        assert first == 1 and status == [0] * first + [cases.STATUS_BADPAGE] * (4 - first), status
        before = np.concatenate([r[2][1] for r in res[:first]], axis=1)
        want = cases.expected(f)[2]
        assert same_bits(before, want[:, :before.shape[1]]) and all(r[2][1].shape == (2, 0) for r in res[first:])
        clean = join([[r[0], r[1], r[3]] for r in res], [[0, 1, 2]] * 4, 3, 2)
        assert_files(an, clean, [files[0], files[1], files[3]], "the clean neighbours")
        assert_files(an, run_rounds(an, dec, [f], [cuts], [2]), [f], "the slot's next stream")
    finally:
        an.close()


def test_many_short_streams():
    """130 short streams in one decoder, pieces of 4096 bytes and, for the carry kernels' grid, a piece per page of the same
    streams with a segment a page: more than one row of k_lap's grid, many carry rows in a launch"""
    g = decode_cases.short_streams(130)
    files = cases.group_files(g, "one_packet")
    singles = cases.group_files(g, "singles")
    an = analyzer(g.blob)
    try:
        dec = an.live_ogg_decoder(130)
        got = run_rounds(an, dec, files, [H.every(f, 4096) for f in files])
        decode_cases.check(g, got)
        got = run_rounds(an, dec, singles, [page_ends(f)[:-1] for f in singles])
        decode_cases.check(g, got)
        whole, status = an.decode_ogg(singles, with_status=True)
        assert not status.any() and all(same_bits(a[1], b.cpu().numpy()) for a, b in zip(got, whole))
    finally:
        an.close()


@pytest.mark.parametrize("flush", [True, False])
def test_a_live_ogg_feeds_loop(flush):
    """the loop the decoder exists for: a live Ogg feed's bytes, group by group as they come out (with vamd_feed_ogg_flush
    on every write, and without), straight into LiveOggDecoder.write; the joined samples are decode_ogg's of the joined file"""
    import vorbis_amd
    from tests.signals import mixed_streams
    streams, cuts = mixed_streams(np.random.default_rng(9), 2)
    blob = vorbis_amd.default_setup_blob(Q4)
    headers = ref_host.reference_headers(2, 44100, 0.4)
    feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=8, max_frames=32000, write_frames=1024, ogg_headers=headers)
    an = vorbis_amd.Analyzer(blob)
    try:
        dec = an.live_ogg_decoder(len(streams), setup_header=headers[2])
        n = len(streams)
        pos, files, out = [0] * n, [b""] * n, [[] for _ in range(n)]
        for r in range(max(len(c) for c in cuts)):
            frames = [c[r] if r < len(c) else 0 for c in cuts]
            close = [r == len(c) - 1 for c in cuts]
            pieces = [x[p:p + k] for x, p, k in zip(streams, pos, frames)]
            pos = [p + k for p, k in zip(pos, frames)]
            group = feed.encode_live_ogg(pieces, close, serials=list(range(50, 50 + n)), flush=True if flush else None)
            got, status = dec.write(list(range(n)), group, close=[s for s in range(n) if close[s]], with_status=True)
            assert not status.any(), (r, status)
            for s in range(n):
                files[s] += group[s]
                out[s].append(got[s].cpu().numpy())
        got = [(0, np.concatenate(o, axis=1)) for o in out]
        assert [g[1].shape[1] for g in got] == [len(x) for x in streams]
        assert_files(an, got, files, ("a live Ogg feed", flush))
    finally:
        an.close()
        feed.close()


def test_refused_calls():
    """a slot named twice, a slot outside the decoder, more streams than slots, offsets that go back: EINVAL with a reason,
    and the decoder goes on as if the call had not been made"""
    import vorbis_amd
    blob, _, files = cases.base_files(Q4, "shared")
    f = files[1]
    a, b = f[:3001], f[3001:]
    an = analyzer(blob)
    try:
        dec = an.live_ogg_decoder(2)
        first, st = dec.write([1], [a], with_status=True)
        assert not st.any()
        for slots, pieces, reason in (([1, 1], [b, b""], "twice"), ([2], [b], "outside"), ([0, 1, 1], [b"", b, b""], "more streams")):
            with pytest.raises(vorbis_amd.VamdError) as e:
                dec.write(slots, pieces, close=slots)
            assert e.value.code == vorbis_amd.api.VAMD_EINVAL and reason in str(e.value), str(e.value)
        with pytest.raises(vorbis_amd.VamdError) as e:
            dec.run(dec.prepare([1], [b], [1], piece_offset=[len(b), 0]))
        assert e.value.code == vorbis_amd.api.VAMD_EINVAL and "monotone" in str(e.value)
        last, st = dec.write([1], [b], close=[1], with_status=True)
        assert not st.any()
        assert_files(an, [(0, np.concatenate([first[0].cpu().numpy(), last[0].cpu().numpy()], axis=1))], [f], "around the refused calls")
    finally:
        an.close()
