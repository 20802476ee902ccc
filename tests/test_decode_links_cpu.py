"""CPU: the reader's bookkeeping (vamd_decode_follow; vamd_decode_streams_marked) on the one-lane host build,
tests/c/decode_links_host.cpp with -fsanitize=address,undefined: the shipped page walk with links and foreign pages, the
plan from per-packet marks, k_ogg_depage's body, unpack_packet, synth_block and the segments' lap body, in buffers of
exactly the library's sizes -- against libvorbis' decoder over what an independent reader makes of each file
(tests/decode_links_cases.py).  Every comparison is exact equality of every frame."""
import struct

import numpy as np
import pytest

from tests import decode_links_cases as cases
from tests import demux_host
from tests.feed_cases import same_bits

BADPAGE, BADHEADER = cases.STATUS_BADPAGE, cases.STATUS_BADHEADER
WALK = ["shift", "trim_k1_below", "trim_k1_equal", "trim_k1_above", "trim_k1_none", "trim_k3_below", "trim_k3_equal", "trim_k3_above", "trim_k3_none",
        "trim_packet0", "trim_only_page_eos", "no_eos", "mid_low", "mid_high", "plain"]


@pytest.fixture(scope="module")
def exe():
    return cases.build()


@pytest.fixture(scope="module")
def followed(exe, tmp_path_factory):
    """every stereo file of the cases in ONE followed call -> name -> result"""
    F = cases.files()
    a = cases.stream()
    res = cases.run_ogg(exe, tmp_path_factory.mktemp("links"), a.blob, [F[k][0] for k in F], 2, True, a.headers[2])
    return dict(zip(F, res))


def parent_plan(s, granules):
    """what the block plan without marks gives a file: the span of the centres, cut against the end granule counted from 0"""
    steps = s.steps()
    total, end = sum(steps), granules[-1]
    return total - min(total - end, steps[-1]) if 0 <= end < total else total


def test_every_file_has_its_status_and_its_frames(followed):
    F = cases.files()
    for name, (f, status) in F.items():
        got = followed[name]
        assert got["status"] == status, name
        if status:
            assert got["frames"] == 0 and not got["segments"], name
            continue
        want = cases.expected(f)[0]
        assert got["frames"] == want.shape[1], (name, got["frames"], want.shape)
        assert same_bits(got["pcm"], want), name


@pytest.mark.parametrize("name", WALK)
def test_granule_walk(followed, name):
    """the walk's cases one by one, each held to what it is there to show"""
    a, b = cases.stream(cases.STEREO, 0), cases.stream(cases.STEREO, 1)
    f = cases.files()[name][0]
    got, want = followed[name], cases.expected(f)[0]
    assert got["status"] == 0 and same_bits(got["pcm"], want)
    s = b if name in ("trim_only_page_eos", "mid_low", "mid_high") else a
    steps, T = s.steps(), want.shape[1]
    if name == "shift":  # the end is cut against the tracked position: the parent's plan, counting from 0, cuts nothing
        assert T == a.end and parent_plan(a, [g + cases.SHIFT for g in a.granules]) == sum(steps) > T
        assert same_bits(want, cases.expected(cases.files()["plain"][0])[0])
    elif name.startswith("trim_k"):
        k = int(name[6])
        extra = {"below": steps[k] - 7, "equal": steps[k], "above": steps[k] + 40, "none": 0}[name.split("_")[2]]
        # the cap: no more than packet k adds; and a page granule below -1 (k = 1, above: 128 - 168) is no position at all
        cut = min(extra, steps[k]) if sum(steps[:k + 1]) - extra >= -1 else 0
        whole = cases.expected(cases.files()["plain"][0])[0]
        lo = sum(steps[:k])
        # frames of packet k -- the LAST packet of the first page -- go, from their beginning; the next page's granule is
        # the encoder's count again and is believed, so the end is cut as the plain file's is
        assert T == a.end - cut, (name, T)
        assert same_bits(want[:, :lo], whole[:, :lo]) and same_bits(want[:, lo:lo + 50], whole[:, lo + cut:lo + cut + 50])
        assert len(got["segments"]) == (2 if cut and lo else 1)  # (packet 1's frames are the stream's first: nothing kept in front of the cut)
    elif name == "trim_only_page_eos":  # first and last page at once: the END is cut
        whole = cases.reference_decode(b.headers + b.packets, [-1] * len(b.packets), [0] * len(b.packets))
        assert T == sum(steps) - 300 and same_bits(want, whole[:, :T]) and len(got["segments"]) == 1
    elif name == "no_eos":
        assert T == sum(steps) > a.end
    elif name in ("mid_low", "mid_high"):  # believe the bitstream: no sample changes, the end cut moves with the position
        d = -90 if name == "mid_low" else 90
        whole = cases.reference_decode(b.headers + b.packets, [-1] * len(b.packets), [0] * len(b.packets))
        assert T == min(b.end - d, sum(steps)) and same_bits(want, whole[:, :T])


def _mark_lists():
    """(stream, granules, eos) -- the files' mark lists and a few more, for the plan alone"""
    a, b = cases.stream(cases.STEREO, 0), cases.stream(cases.STEREO, 1)
    out = []
    for name in WALK:
        s = b if name in ("trim_only_page_eos", "mid_low", "mid_high") else a
        (_, _, _, pages), = cases.read_links(cases.files()[name][0])
        _, gran, eos = cases.link_marks(pages)
        out.append((s, gran, eos))
    n = len(a.packets)
    out.append((a, [-1] * n, [0] * n))                                    # no position at all
    out.append((a, [-5] + [-1] * (n - 2) + [a.end], [0] * (n - 1) + [1]))   # below -1: none
    out.append((a, [g - 60 * p for p, g in enumerate(a.granules)], [1] * n))  # every packet e_o_s and 60 short of the tracked position: a run per packet
    out.append((a, [2 ** 62] + a.granules[1:], [0] * (n - 1) + [1]))      # a huge first position, then believed back
    out.append((a, a.granules, None))                                     # eos NULL: the last packet
    return out


def test_plan_from_marks_alone(exe, tmp_path):
    """decode_plan_build_marked against the walk restated (tests/decode_links_cases.py: walk): frames and segments"""
    lists = _mark_lists()
    a = cases.stream()
    res = cases.run_packets(exe, tmp_path, a.blob, [s.packets for s, _, _ in lists[:-1]], [g for _, g, _ in lists[:-1]], [e for _, _, e in lists[:-1]], 2,
                            decode=False)
    res += cases.run_packets(exe, tmp_path, a.blob, [lists[-1][0].packets], [lists[-1][1]], None, 2, decode=False)
    k = 0
    for (s, gran, eos), got in zip(lists, res):
        n = len(s.packets)
        k = k if eos is not None else 0  # (the last list went through a call of its own)
        frames, runs = cases.walk(s.Ws, s.bs, gran, eos if eos is not None else [0] * (n - 1) + [1])
        assert got["status"] == 0 and got["frames"] == frames
        assert [(k, k + n) + r for r in runs] == [tuple(g) for g in got["segments"]], (gran, eos)
        k += n
    assert len(res[len(WALK) + 2]["segments"]) >= len(a.packets) - 2  # (the run per packet)


def test_marks_decode_as_the_reference(exe, tmp_path):
    """the mark lists through the packet form, decoded: the frames of the reference over the same marks"""
    lists = _mark_lists()[:-1]
    a = cases.stream()
    res = cases.run_packets(exe, tmp_path, a.blob, [s.packets for s, _, _ in lists], [g for _, g, _ in lists], [e for _, _, e in lists], 2)
    for (s, gran, eos), got in zip(lists, res):
        want = cases.reference_decode(s.headers + s.packets, [g if g >= -1 else -1 for g in gran], eos)
        assert got["status"] == 0 and same_bits(got["pcm"], want), (gran, eos)


def test_a_bad_descriptor_is_refused(exe, tmp_path):
    a = cases.stream()
    n = len(a.packets)
    assert cases.run_packets(exe, tmp_path, a.blob, [a.packets], [a.granules], [[0] * n], 2, decode=False) is not None
    # stream_start beyond the packets: the same job with a second stream that names packets that are not there
    off = np.concatenate([[0], np.cumsum([len(p) for p in a.packets])])
    job = (struct.pack("<iii", 2, n, 0) + cases._i64s(off) + cases._i64s([0, n, n + 3]) + cases._i64s(a.granules) + cases._i64s([0] * n) +
           struct.pack("<i", int(off[-1])) + cases._padded(b"".join(a.packets)))
    raw = cases._run(exe, tmp_path, "packets", a.blob, job, "bad")
    assert struct.unpack_from("<i", raw, 0)[0] == 0 and len(raw) == 4


def test_links_decode_alone_as_in_the_whole(exe, tmp_path, followed):
    """each link's byte range as a file of its own equals its part of the whole"""
    F = cases.files()
    a = cases.stream()
    names = ["two_links", "three_links", "one_packet_link", "no_eos_then_bos", "foreign_interleaved"]
    parts, owner = [], []
    for name in names:
        f = F[name][0]
        for begin, end, _, _ in cases.read_links(f):
            parts.append(f[begin:end]), owner.append(name)
    res = cases.run_ogg(exe, tmp_path, a.blob, parts, 2, True, a.headers[2])
    for name in names:
        mine = [r for r, o in zip(res, owner) if o == name]
        assert all(r["status"] == 0 for r in mine)
        assert same_bits(np.concatenate([r["pcm"] for r in mine], axis=1), followed[name]["pcm"]), name
    assert len([o for o in owner if o == "three_links"]) == 3


def test_the_mono_stream(exe, tmp_path):
    M = cases.mono_files()
    m = cases.stream(cases.MONO, 3)
    res = cases.run_ogg(exe, tmp_path, m.blob, [f for f, _ in M.values()], 1, True, m.headers[2])
    for (name, (f, _)), got in zip(M.items(), res):
        assert got["status"] == 0 and same_bits(got["pcm"], cases.expected(f)[0]), name
    assert res[2]["frames"] == 2 * m.end and res[1]["frames"] == m.end


def test_policy_off_is_the_existing_walk(exe, tmp_path):
    """without the policy every one of the files has the status and the frames the existing scan gives it"""
    F = cases.files()
    a = cases.stream()
    off = cases.run_ogg(exe, tmp_path, a.blob, [F[k][0] for k in F], 2, False, a.headers[2])
    was = demux_host.host_scan(demux_host.build(), tmp_path, np.frombuffer(a.blob, np.uint8), [F[k][0] for k in F], a.headers[2])
    for name, got, old in zip(F, off, was):
        assert (got["status"], got["frames"]) == (old["status"], old["frames"]) and not got["segments"], name
        # one serial number: decoded as before; a second one: flagged at it, as before
        assert got["status"] == (0 if name in WALK else BADPAGE), name
    assert off[list(F).index("shift")]["frames"] == sum(a.steps())  # (the wrong tail the policy is there to mend)


def test_ogg_links(exe, tmp_path):
    """vamd_ogg_links' body: the links an independent reader finds; a cap that is too small; cut files"""
    F = cases.files()
    a = cases.stream()
    for name in ("plain", "three_links", "foreign_bos_first", "foreign_only", "no_eos_then_bos", "other_setup"):
        f = F[name][0]
        want = [(b, e, s) for b, e, s, _ in cases.read_links(f)]
        rc, n, rows = cases.run_links(exe, tmp_path, a.blob, f, 8)
        assert rc == 0 and n == len(want), name
        for (b, e, s), row in zip(want, rows):
            assert row[:2] == (b, e) and (s is None or row[2] == s), name
    f = F["three_links"][0]
    assert cases.run_links(exe, tmp_path, a.blob, f, 2)[:2] == (-131, 3) and cases.run_links(exe, tmp_path, a.blob, f, 0) == (-131, 3, [])
    links = cases.read_links(f)
    firsts = [b + cases.ogg_framing.pages_of(f[b:e])[0]["bytes"] for b, e, _, _ in links]  # where each link's first page ends
    for cut in (1, 26, 27, 28, links[1][0] + 5, links[1][0] + 27, links[2][0] + 100, len(f) - 1):  # inside headers, lacing tables and bodies
        rc, n, rows = cases.run_links(exe, tmp_path, a.blob, f[:cut], 8)
        assert rc == -133 and n == sum(e <= cut for e in firsts) and all(e <= cut for _, e, _ in rows), cut  # (a link is listed once its first page holds)
    assert cases.run_links(exe, tmp_path, a.blob, b"", 4) == (0, 0, [])
