"""CPU: the live Ogg decoder -- the shipped walk with its state per slot (vorbis_amd/csrc/vamd_demux_live.h), the live block
plan over its packet table and the bodies of k_ogg_packet_carry_in, k_ogg_depage and k_ogg_packet_carry_out (k_demux.h)
compiled for the host, tests/c/demux_live_host.cpp, a program of its own built with -fsanitize=address,undefined and run as
a child process with many cut lists per run -- against tests/ogg_framing.py's reader (the container) and the reference
decoder (the signal) over the WHOLE file: the pieces' packets, end granule and samples, laid end to end, are the file's.

The base files of tests/ogg_demux_cases.py are some 8 KiB with packets of at most 713 bytes, and under its `full_255` and
`seeded` policies no page of theirs ends inside an audio packet; the cases that need a packet left open by whole pages
lay the same streams out with a segment a page (`singles`) and with one to three segments a page (cases.write)."""
import numpy as np
import pytest

from oracle import ref
from tests import decode_cases, demux_live_host as H, ogg_demux_cases as cases, ogg_framing, ref_host, synth_host

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")
BADPAGE, BADHEADER = cases.STATUS_BADPAGE, cases.STATUS_BADHEADER
CONTAINER = BADPAGE | BADHEADER
Q4 = "44k_stereo_q4"


@pytest.fixture(scope="module")
def exe():
    return H.build()


def want(f):
    return H.ref(*cases.expected(f))


def channels(name):
    return synth_host.SETUPS[name][0]


def assert_compact(res, what):
    bad = [(i, r) for i, r in enumerate(res) if r["refused"] or any(r["verdict"])]
    assert not bad, (what, len(bad), bad[:4])


def assert_stream(got, f, what):
    packets, end, pcm = cases.expected(f)
    assert got["status"] == 0 and got["packets"] == packets and got["end"] == end, (what, got["status"], got["end"], end, len(got["packets"]), len(packets))
    assert got["pcm"].shape == pcm.shape and np.array_equal(got["pcm"].view(np.uint32), pcm.view(np.uint32)), (what, got["pcm"].shape, pcm.shape)


def joined(rows_of, nstreams=1, ch=2, who=None):
    return H.join(rows_of, who or [[0]] * len(rows_of), nstreams, ch)


def small_pages(name, v=0, seed=5):
    """a base stream with one to three segments a page: packets of 255 bytes and more lie across pages"""
    blob, headers, bs, base = decode_cases.base_streams(name, 1)
    packets, end = base[v]
    rng = np.random.default_rng(seed)
    return blob, cases.write(list(headers) + list(packets), [0, 0, 0] + cases.packet_granules(packets, end, bs), lambda *a: rng.integers(1, 4))


def page_ends(f):
    return [p["offset"] + p["bytes"] for p in ogg_framing.demux(f)[0]]


# ---- every single byte cut ----
@pytest.mark.parametrize("policy", [p for p in cases.POLICIES if p != "big_comment"])
def test_every_byte_cut(exe, tmp_path, policy):
    """two pieces, the cut at every byte of the file, both ends included"""
    blob, _, files = cases.base_files(Q4, policy)
    f = files[0]
    runs = [H.compact(H.one_stream(f, [c]), [(0, 0)]) for c in range(len(f) + 1)]
    assert_compact(H.run(exe, tmp_path, blob, 2, runs, [want(f)]), policy)


@pytest.mark.parametrize("name", [n for n in synth_host.FEED_SETUPS if n != Q4])
def test_every_seventh_cut(exe, tmp_path, name):
    blob, _, files = cases.base_files(name, "seeded")
    f = files[1]
    runs = [H.compact(H.one_stream(f, [c]), [(0, 0)]) for c in range(0, len(f) + 1, 7)]
    assert_compact(H.run(exe, tmp_path, blob, channels(name), runs, [want(f)]), name)


@pytest.mark.parametrize("policy", ["shared", "one_packet"])
def test_one_byte_pieces(exe, tmp_path, policy):
    """a byte at a time from byte 0 to behind the second audio page, then the rest in one piece"""
    blob, _, files = cases.base_files(Q4, policy)
    f = files[2]
    pages = ogg_framing.demux(f)[0]
    audio = [p for i, p in enumerate(pages) if sum(q["done"] for q in pages[:i + 1]) > 3]
    upto = audio[1]["offset"] + audio[1]["bytes"] + 3
    res = H.run(exe, tmp_path, blob, 2, [H.compact(H.one_stream(f, list(range(1, upto + 1))), [(0, 0)])], [want(f)])
    assert_compact(res, policy)


def test_big_comment(exe, tmp_path):
    """a comment header of 131 000 bytes in pieces of 4093: dozens of pieces and pages that complete nothing"""
    blob, _, files = cases.base_files(Q4, "big_comment")
    f = files[0]
    calls = H.one_stream(f, H.every(f, 4093))
    assert len(calls) > 30
    got = joined(H.run(exe, tmp_path, blob, 2, [H.full(calls)])[0])[0]
    assert_stream(got, f, "big_comment")
    # the same bytes with less room for headers than the comment takes: flagged when the bound is passed, dead from there on
    rows = H.run(exe, tmp_path, blob, 2, [H.full(calls)], max_header_bytes=cases.BIG_COMMENT - 1)[0]
    status = [r[0]["status"] for r in rows]
    first = next(i for i, s in enumerate(status) if s)
    assert 0 < first and 4093 * (first + 1) > cases.BIG_COMMENT - 1000 and status[first:] == [BADHEADER] * (len(status) - first)
    assert not any(r[0]["pcm"].size or r[0]["packets"] for r in rows)


# ---- the device carry ----
@pytest.mark.parametrize("name, layout", [(Q4, "singles"), ("44k_51_q3", "singles"), ("44k_51_q3", "small"), (Q4, "small")])
def test_packet_open_across_pieces(exe, tmp_path, name, layout):
    """a piece per page: an audio packet of 255 bytes and more is left open by a whole page, one of 510 and more by two --
    it goes carry -> arena -> carry -- and completes one or two pieces later"""
    if layout == "singles":
        blob, _, files = cases.base_files(name, "singles")
        f = files[0]
    else:
        blob, f = small_pages(name)
    ch = channels(name)
    ends = page_ends(f)
    rows = H.run(exe, tmp_path, blob, ch, [H.full(H.one_stream(f, ends[:-1]))])[0]
    assert_stream(joined(rows, 1, ch)[0], f, (name, layout))
    longest = max(len(p) for p in cases.expected(f, decode=False)[0])
    outs, ins = [r[0]["carry_out"] for r in rows], [r[0]["carry_in"] for r in rows]
    assert max(outs) > 0 and all(0 <= v < longest for v in outs), outs
    assert ins[1:] == outs[:-1], (ins, outs)  # what a call leaves is what the next takes
    two = any(o > 0 and i == 0 for i, o in zip(ins, outs))
    three = any(o > i > 0 for i, o in zip(ins, outs))  # open across a whole piece
    assert two and (three or longest < 510 or layout == "small"), (ins, outs)
    if (name, layout) == ("44k_51_q3", "singles"):
        assert three
    # the same with the cuts a few bytes off the page ends: the held tail and the carry at once
    for shift in (-1, 5):
        calls = H.one_stream(f, [e + shift for e in ends[:-1]])
        got = joined(H.run(exe, tmp_path, blob, ch, [H.full(calls)])[0], 1, ch)[0]
        assert_stream(got, f, (name, layout, shift))


def test_packet_bound(exe, tmp_path):
    """an open packet exactly at max_packet_bytes decodes; one byte over is BADPAGE with no row for the launches"""
    name = "44k_51_q3"
    blob, _, files = cases.base_files(name, "singles")
    f, ch = files[0], channels(name)
    ends = page_ends(f)
    calls = H.one_stream(f, ends[:-1])
    assert max(len(p) for p in cases.expected(f, decode=False)[0]) >= 510
    got = joined(H.run(exe, tmp_path, blob, ch, [H.full(calls)], max_packet_bytes=510)[0], 1, ch)[0]
    assert_stream(got, f, "at the bound")
    rows = H.run(exe, tmp_path, blob, ch, [H.full(calls + H.one_stream(f, ends[:-1]))], max_packet_bytes=509)[0]
    status = [r[0]["status"] for r in rows[:len(calls)]]
    first = status.index(BADPAGE)
    assert status == [0] * first + [BADPAGE] * (len(calls) - first)
    assert rows[first - 1][0]["carry_out"] == 255 and all(r[0]["carry_out"] == 0 and r[0]["carry_in"] == 0 and not r[0]["packets"] for r in rows[first:len(calls)])
    # the slot's next stream: the closing piece freed it.  It meets the same bound at the same place
    again = [r[0]["status"] for r in rows[len(calls):]]
    assert again == status


# ---- cut lists ----
def test_seeded_cut_lists(exe, tmp_path):
    """seeded cut lists with empty pieces, the stream closed with its last bytes and closed later with an empty piece"""
    rng = np.random.default_rng(29)
    refs, runs = [], []
    for policy in ("feed", "seeded", "shared", "singles"):
        blob, _, files = cases.base_files(Q4, policy)
        for f in files[:2]:
            refs.append(want(f))
            for k in range(12):
                runs.append(H.compact(H.one_stream(f, H.random_cuts(len(f), rng), slot=k % 4, close_with_last=bool(k & 1)), [(k % 4, len(refs) - 1)]))
    assert_compact(H.run(exe, tmp_path, blob, 2, runs, refs), "seeded cut lists")


def without_eos(f):
    last = ogg_framing.demux(f)[0][-1]
    assert last["flags"] & 4
    at = last["offset"] + 5
    return cases.reseal(f[:at] + bytes([f[at] & ~4]) + f[at + 1:], last["offset"])


def test_closed_without_the_flag(exe, tmp_path):
    """no end-of-stream flag: the closing piece holds the last packet, and the stream comes out as the whole file does; closed
    later with an empty piece the last block is not cut (the live packet decoder's rule)"""
    blob, _, files = cases.base_files(Q4, "seeded")
    f = without_eos(files[3])
    packets, end, pcm = cases.expected(f)
    rng = np.random.default_rng(3)
    runs = []
    for k in range(16):
        cuts = [c for c in H.random_cuts(len(f), rng) if c < len(f) - 400]  # (the last packet lies in the last piece)
        runs.append(H.compact(H.one_stream(f, cuts), [(0, 0)]))
    assert_compact(H.run(exe, tmp_path, blob, 2, runs, [want(f)]), "no flag, closed with the last bytes")
    rows = H.run(exe, tmp_path, blob, 2, [H.full(H.one_stream(f, [3000], close_with_last=False))])[0]
    got = joined(rows)[0]
    assert got["status"] == 0 and got["packets"] == packets and got["end"] == -1
    assert got["pcm"].shape[1] >= pcm.shape[1] and np.array_equal(got["pcm"][:, :pcm.shape[1]].view(np.uint32), pcm.view(np.uint32))


def test_streams_side_by_side(exe, tmp_path):
    """four slots, four files of one policy each, pieces of 997 bytes: later calls name fewer slots; slots in another order"""
    files = [cases.base_files(Q4, p)[2][i] for i, p in enumerate(("feed", "one_packet", "shared", "singles"))]
    blob = cases.base_files(Q4, "feed")[0]
    slots = [2, 0, 3, 1]
    calls, who = H.rounds(files, [H.every(f, 997 - 100 * i) for i, f in enumerate(files)], slots)
    assert len({len(w) for w in who}) > 1
    rows = H.run(exe, tmp_path, blob, 2, [H.full([H.call(*c) for c in calls])])[0]
    for got, f in zip(H.join(rows, who, 4, 2), files):
        assert_stream(got, f, "side by side")


# ---- damage ----
@pytest.mark.parametrize("name", [Q4, "44k_51_q3"])
def test_damage(exe, tmp_path, name):
    """tests/ogg_demux_cases.py's damaged files beside their clean neighbours, every file in 4 pieces: the status bit is the
    whole-file contract's; the pieces before the flagged one stand and are the undamaged stream's beginning; the clean
    neighbours are as without the damaged ones"""
    d = cases.damaged(name)
    ch, n = channels(name), len(d.files)
    singles = cases.base_files(name, "singles")[2]
    calls, who = H.rounds(d.files, [[len(f) // 4, len(f) // 2, 3 * len(f) // 4] for f in d.files])
    rows = H.run(exe, tmp_path, d.blob, ch, [H.full([H.call(*c) for c in calls])], max_streams=n, setup_header=d.setup_header)[0]
    assert all(r is not None for r in rows)
    clean = [s for s in range(n) if d.kind[s] is None]
    alone, who_alone = H.rounds([d.files[s] for s in clean], [[len(d.files[s]) // 4, len(d.files[s]) // 2, 3 * len(d.files[s]) // 4] for s in clean], clean)
    rows_alone = H.run(exe, tmp_path, d.blob, ch, [H.full([H.call(*c) for c in alone])], max_streams=n, setup_header=d.setup_header)[0]
    got_alone = dict(zip(clean, H.join(rows_alone, who_alone, len(clean), ch)))
    for s, got in enumerate(H.join(rows, who, n, ch)):
        what = (name, s, d.kind[s])
        per_piece = [r[who[k].index(s)]["status"] for k, r in enumerate(rows)]
        if not d.bit[s]:
            assert_stream(got, d.files[s], what)
            if d.kind[s] is None:
                assert np.array_equal(got["pcm"].view(np.uint32), got_alone[s]["pcm"].view(np.uint32)) and got_alone[s]["status"] == 0, what
            continue
        first = next(k for k, v in enumerate(per_piece) if v)
        assert per_piece[first] & d.bit[s] and all(v == per_piece[first] for v in per_piece[first:-1]) and per_piece[-1], (what, per_piece)
        base = cases.expected(singles[(s // 2) % 4])[2]
        before = np.concatenate([np.zeros((ch, 0), np.float32)] + [r[who[k].index(s)]["pcm"] for k, r in enumerate(rows[:first])], axis=1)
        assert before.shape[1] <= base.shape[1] and np.array_equal(before.view(np.uint32), base[:, :before.shape[1]].view(np.uint32)), (what, before.shape)
        assert all(r[who[k].index(s)]["pcm"].size == 0 for k, r in enumerate(rows) if k >= first), what
    assert {k for k in d.kind if k} == set(cases.DAMAGE)


def test_closing_and_ended_streams(exe, tmp_path):
    """closing inside a page, inside a packet, before the headers are complete and on a free slot; a page behind the
    end-of-stream page; after each the slot takes a whole clean stream"""
    blob, _, files = cases.base_files(Q4, "singles")
    f, g = files[0], files[1]
    pages = ogg_framing.demux(f)[0]
    done = np.cumsum([p["done"] for p in pages])
    open_audio = next(p for i, p in enumerate(pages) if p["open"] and done[i] >= 3)
    in_packet = open_audio["offset"] + open_audio["bytes"]
    setup_open = next(p for i, p in enumerate(pages) if p["open"] and done[i] < 3)
    good = H.one_stream(g, H.every(g, 1500))
    cases_ = [
        ("inside a page", [H.call([0], [f[:in_packet + 40]], [0])], BADPAGE),
        ("inside a packet", [H.call([0], [f[:in_packet]], [0])], BADPAGE),
        ("inside a header packet", [H.call([0], [f[:setup_open["offset"] + setup_open["bytes"]]], [0])], BADPAGE),
        ("two headers", [H.call([0], [f[:pages[1]["offset"] + pages[1]["bytes"]]], [0])], BADHEADER),
        ("a free slot", [H.call([0], [b""], [0])], BADHEADER),
        ("no bytes, then closed", [H.call([0], [b""]), H.call([0], [b""], [0])], BADHEADER),
        ("a page behind the last", [H.call([0], [f]), H.call([0], [g[:pages[0]["bytes"]]]), H.call([0], [b"x"]), H.call([0], [b""], [0])], BADPAGE),
        ("bytes behind the last page", [H.call([0], [f]), H.call([0], [b"Ogg"]), H.call([0], [b""], [0])], BADPAGE),
    ]
    calls = []
    for _, c, _ in cases_:
        calls += c + good
    rows = H.run(exe, tmp_path, blob, 2, [H.full(calls)])[0]
    at = 0
    for what, c, bit in cases_:
        mine, after = rows[at:at + len(c)], rows[at + len(c):at + len(c) + len(good)]
        at += len(c) + len(good)
        status = [r[0]["status"] for r in mine]
        assert status[-1] == bit, (what, status)
        if what == "a page behind the last":
            assert status == [0, BADPAGE, BADPAGE, BADPAGE], status
            assert_stream(joined(mine[:1])[0], f, what)  # (the whole stream had left before: it stands)
        elif what == "bytes behind the last page":
            assert status == [0, 0, BADPAGE], status
        else:
            assert not any(status[:-1]) and mine[-1][0]["pcm"].size == 0 and not mine[-1][0]["packets"], (what, status)
        assert_stream(joined(after)[0], g, "the slot's next stream after " + what)


# ---- seeded mutations ----
FUZZ = 1200


def page_flags(f):
    """the flag bytes of a file that reads whole (ogg_framing.demux would refuse a flag bit it does not know)"""
    pos, out = 0, []
    while pos < len(f):
        n = f[pos + 26]
        out.append(f[pos + 5])
        pos += 27 + n + sum(f[pos + 27:pos + 27 + n])
    return out


def test_fuzz(exe, tmp_path):
    """seeded mutations of small files in pieces of 1000 bytes, each stream alone and every buffer exactly its size, under
    the sanitisers.  A stream comes out without a container bit exactly where the non-asserting reader reads the file
    whole and no page but its last carries the end-of-stream flag (an ended stream takes no further page); where that last
    page carries it and nothing else was touched the samples are the reference's"""
    g = decode_cases.short_streams(4)
    files = cases.group_files(g, "one_packet") + cases.group_files(g, "seeded")
    ch, rate = synth_host.SETUPS[g.name][:2]
    enc = ref_host.encoder(g.name)
    bs = (enc.blocksize(0), enc.blocksize(1))
    mutated = cases.mutations(files, FUZZ)
    runs = [H.full(H.one_stream(f, H.every(f, 1000))) for f in mutated]
    res = H.run(exe, tmp_path, g.blob, ch, runs, max_streams=1, max_packet_bytes=65536)
    clean = 0
    for i, (rows, f) in enumerate(zip(res, mutated)):
        assert all(r is not None for r in rows)
        whole = cases.reads_whole(f, ch, rate, bs)
        if whole:
            whole = not any(v & 4 for v in page_flags(f)[:-1])
        status = 0
        for r in rows:
            status |= r[0]["status"]
        assert (status & CONTAINER == 0) == whole, (i, i % 6, status, whole, len(f))
        clean += whole
        if whole and f in files:
            assert_stream(joined(rows, 1, ch)[0], f, i)
    assert FUZZ // 20 <= clean <= FUZZ - FUZZ // 4, clean  # both verdicts are well represented


# ---- refused descriptors ----
def test_refused_descriptors(exe, tmp_path):
    """each bad descriptor between two pieces of a stream: refused, and the stream comes out as if it had not been there"""
    blob, _, files = cases.base_files(Q4, "shared")
    f = files[1]
    a, b = f[:3001], f[3001:]
    bad = [H.call([0], [b], null=H.NULL_SLOT), H.call([0], [b], null=H.NULL_BYTES), H.call([0], [b], null=H.NULL_OFFSET),
           H.call([0], [b], piece_offset=[len(b), 0]), H.call([0], [b], piece_offset=[-1, len(b)]),
           H.call([4], [b]), H.call([-1], [b]), H.call([0, 0], [b, b""]), H.call([0, 1, 2, 3, 0], [b, b"", b"", b"", b""]),
           H.call([0], [b], nstreams=-1)]
    runs = [H.full([H.call([0], [a]), c, H.call([0], [b], [0])]) for c in bad]
    for rows in H.run(exe, tmp_path, blob, 2, runs):
        assert rows[1] is None
        assert_stream(H.join([rows[0], rows[2]], [[0], [0]], 1, 2)[0], f, "behind a refused call")
    # a NULL close is no error: nothing closes
    rows = H.run(exe, tmp_path, blob, 2, [H.full([H.call([0], [a], null=H.NULL_CLOSE), H.call([0], [b], [0])])])[0]
    assert_stream(joined(rows)[0], f, "null close")
