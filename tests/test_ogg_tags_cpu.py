"""CPU suite: a comment header per stream (vamd_feed_ogg_comments) as far as it needs no GPU -- the pure-Python builder and
reader of comment headers against the reference's vorbis_commentheader_out, the validator of vorbis_amd/csrc/k_ogg.h
(ogg_comment_check, compiled with the host compiler) against the reference's vorbis_synthesis_headerin, and the bounds a
group with comments of its own is sized by: page slots from its longest comment, the file arena from their sum."""
import struct

import numpy as np
import pytest

import vorbis_amd
from tests import ogg_host as oh
from tests import ref_host as rh
from tests.signals import LIVE_SIZE_LISTS, WHOLE_SIZE_LISTS as SIZE_LISTS

TAG_SETS = {
    "none": [],
    "one": [("TITLE", "Track 1")],
    "utf8": [("TITLE", "Überfahrt"), ("ARTIST", "Ðe Ensemble ☃"), ("ALBUM", "夜の歌"), ("TITLE", "a second title")],
    "empty_value": [("TITLE", ""), ("ARTIST", "x")],
    "100000": [("TITLE", "long"), ("METADATA_BLOCK_PICTURE", "QUJD" * 25000)],
}
COMMENT_LENGTHS = [7, 255, 65025, 65026, 200000]


def _ref():
    from oracle import ref
    if not ref.available():
        pytest.skip("needs the reference build")
    return ref


@pytest.fixture(scope="module")
def hosts():
    host = oh.HostOgg()
    return host, host, host


@pytest.fixture(scope="module")
def reference_packets():
    """per tag set the comment header vorbis_commentheader_out writes, and the identification header beside it"""
    _ref()
    out = {}
    for name, tags in TAG_SETS.items():
        h = rh.reference_headers(2, 44100, 0.4, tags=tags)
        out[name] = h[1]
        out["ident"] = h[0]
    return out


@pytest.mark.parametrize("name", list(TAG_SETS))
def test_builder_writes_the_references_packet(reference_packets, name):
    want = reference_packets[name]
    vendor, tags = vorbis_amd.comment_fields(want)
    assert tags == TAG_SETS[name] and vendor
    assert vorbis_amd.comment_packet(TAG_SETS[name], vendor) == want
    assert vorbis_amd.comment_fields(vorbis_amd.comment_packet(TAG_SETS[name], "another vendor ☃")) == ("another vendor ☃", TAG_SETS[name])


def test_builder_without_the_reference():
    """the layout itself (Vorbis I 5.2.1), so that the builder is covered where the reference build is absent"""
    p = vorbis_amd.comment_packet([("A", "b"), ("C", "")], "v")
    assert p == b"\x03vorbis" + struct.pack("<I", 1) + b"v" + struct.pack("<I", 2) + struct.pack("<I", 3) + b"A=b" + \
        struct.pack("<I", 2) + b"C=" + b"\x01"
    assert vorbis_amd.comment_fields(p) == ("v", [("A", "b"), ("C", "")])
    assert vorbis_amd.comment_packet([], "") == b"\x03vorbis" + b"\0" * 8 + b"\x01"
    for bad in (p[:-1], p[:12], b"\x05" + p[1:], p[:-1] + b"\0"):
        with pytest.raises((ValueError, struct.error)):
            vorbis_amd.comment_fields(bad)


def _raised(packet, at, by):
    """the little-endian length at byte `at` of the packet raised by `by`"""
    v, = struct.unpack_from("<I", packet, at)
    return packet[:at] + struct.pack("<I", v + by) + packet[at + 4:]


def validator_cases(packets):
    """-> [(what, candidate, accepted)] -- what the issue lists: the reference's packets, padded; every strict prefix of a
    small one; lengths raised past the end; the framing bit cleared; other packet types"""
    cases = []
    for name in TAG_SETS:
        p = packets[name]
        cases += [(name, p, True), (name + " + 1 zero byte", p + b"\0", True), (name + " + 300 zero bytes", p + b"\0" * 300, True)]
    small = packets["one"]
    cases += [("prefix %d" % n, small[:n], False) for n in range(len(small))]
    vlen, = struct.unpack_from("<I", small, 7)
    count_at = 11 + vlen
    first_at = count_at + 4
    rest = len(small) - 1                                            # (the framing byte's place)
    cases += [("vendor length past the end", _raised(small, 7, len(small)), False),
              ("vendor length up to the framing byte", _raised(small, 7, rest - (11 + vlen)), False),
              ("comment count past the end", _raised(small, count_at, 1), False),
              ("comment count 2^31", _raised(small, count_at, 1 << 31), False),
              ("comment length one past its bytes", _raised(small, first_at, 1), False),
              ("comment length past the end", _raised(small, first_at, 1000), False),
              ("framing bit cleared", small[:-1] + b"\0", False),
              ("framing byte 0xfe", small[:-1] + b"\xfe", False),
              ("framing byte 0xff", small[:-1] + b"\xff", True),
              ("type 1", b"\x01" + small[1:], False),
              ("type 5", b"\x05" + small[1:], False)]
    utf8 = packets["utf8"]
    uv, = struct.unpack_from("<I", utf8, 7)
    second_at = 11 + uv + 4 + 4 + struct.unpack_from("<I", utf8, 11 + uv + 4)[0]
    cases.append(("second comment's length past the end", _raised(utf8, second_at, len(utf8)), False))
    return cases


def test_validator_agrees_with_the_reference(hosts, reference_packets):
    """ogg_comment_check accepts exactly what the reference's vorbis_synthesis_headerin accepts as the second header
    packet -- and each case's expectation is stated here too, so that two wrong readers cannot agree unnoticed."""
    tags = hosts[2]
    for what, candidate, accepted in validator_cases(reference_packets):
        code = tags.check(candidate)
        assert (code == 0) == accepted, "%s: ogg_comment_check = %d (%s)" % (what, code, tags.why(code))
        r = rh.reference_headerin(reference_packets["ident"], candidate)
        assert (r == 0) == (code == 0), "%s: vorbis_synthesis_headerin = %d, ogg_comment_check = %d" % (what, r, code)


def test_validator_without_the_reference(hosts):
    tags = hosts[2]
    p = vorbis_amd.comment_packet([("TITLE", "x")], "vendor")
    assert tags.check(p) == 0 and tags.check(p + b"\0" * 300) == 0
    assert all(tags.check(p[:n]) != 0 for n in range(len(p)))
    assert tags.check(p[:-1] + b"\0") != 0 and tags.check(b"\x01" + p[1:]) != 0 and tags.check(b"\x05" + p[1:]) != 0
    assert tags.check(_raised(p, 7, len(p))) != 0 and tags.check(_raised(p, 17, 1)) != 0 and tags.check(_raised(p, 21, 1)) != 0
    assert tags.check(vorbis_amd.comment_packet([], "")) == 0
    assert "framing" in tags.why(tags.check(p[:-1] + b"\0"))


def _lists():
    out = {"whole:" + k: v for k, v in SIZE_LISTS.items()}
    out.update({"live:" + k: v for k, v in LIVE_SIZE_LISTS.items()})
    return out


def test_slots_and_file_bound_of_a_group_with_comments(hosts):
    """Every packet list of the CPU Ogg suites with every comment length: a stream's pages fit the slots computed from
    the group's LONGEST comment, and the group's files fit ogg_file_bound_v of the comments' SUM."""
    whole, _, tags = hosts
    setup = 4140
    for name, sizes in _lists().items():
        n, cap = len(sizes), max(max(sizes), 1)
        granules = list(range(1, n + 1))
        rounded = sum((v + 3) // 4 * 4 for v in sizes)
        total = 0
        for c in COMMENT_LENGTHS:
            planned, file_bytes = whole.plan(sizes, granules, [30, c, setup])
            for longest in (c, max(COMMENT_LENGTHS)):
                assert len(planned) <= whole.slots([30, longest, setup], n, cap), (name, c, longest, len(planned))
            assert file_bytes <= tags.file_bound_v(sum(sizes), n, 1, [30, c, setup], c), (name, c)
            assert file_bytes <= tags.file_bound_v(rounded + 1000, n, 1, [30, c, setup], c), (name, c)
            total += file_bytes
        ns = len(COMMENT_LENGTHS)
        assert total <= tags.file_bound_v(ns * rounded, ns * n, ns, [30, max(COMMENT_LENGTHS), setup], sum(COMMENT_LENGTHS)), name


def test_live_slots_and_file_bound_of_a_group_with_comments(hosts):
    """The same for a file in pieces: the group that begins a stream carries all its header pages; later groups none."""
    whole, live, tags = hosts
    setup = 4140
    rng = np.random.default_rng(23)
    for name, sizes in LIVE_SIZE_LISTS.items():
        packets = [rng.integers(0, 256, v, dtype=np.uint8).tobytes() for v in sizes]
        granules = list(range(1, len(sizes) + 1))
        cap = max(sizes)
        for c in COMMENT_LENGTHS:
            headers = [rng.integers(0, 256, v, dtype=np.uint8).tobytes() for v in (30, c, setup)]
            hb = [30, c, setup]
            want = whole.mux(headers, packets, granules, 9)
            for groups in ([0, len(sizes)], [len(sizes) // 2, len(sizes) - len(sizes) // 2], [1, 0, len(sizes) - 1], [len(sizes), 0]):
                st, k, got = live.stream(headers, 9), 0, b""
                for g, m in enumerate(groups):
                    piece = st.piece(packets[k:k + m], granules[k:k + m], g == len(groups) - 1)
                    new = sum((v + 3) // 4 * 4 for v in sizes[k:k + m])
                    k += m
                    for longest in (c, max(COMMENT_LENGTHS)):
                        assert st.npages <= live.live_slots([30, longest, setup], m, cap), (name, c, g, st.npages)
                    assert len(piece) <= tags.live_file_bound_v(new, m, 1, hb, c), (name, c, g, len(piece))
                    got += piece
                assert got == want, (name, c, groups)


def test_one_picture_among_many_plain_streams(hosts):
    """One stream with a 200 000-byte comment among 63 of 7 bytes: the bound follows the sum, not 64 times the longest --
    and still holds every file."""
    whole, _, tags = hosts
    setup = 4140
    sizes = SIZE_LISTS["fill_rule"]
    granules = list(range(1, len(sizes) + 1))
    comments = [200000] + [7] * 63
    total = sum(whole.plan(sizes, granules, [30, c, setup])[1] for c in comments)
    rounded = sum((v + 3) // 4 * 4 for v in sizes)
    for fn in (tags.file_bound_v, tags.live_file_bound_v):
        bound = fn(64 * rounded, 64 * len(sizes), 64, [30, 200000, setup], sum(comments))
        assert total <= bound
        assert fn(0, 0, 64, [30, 200000, setup], sum(comments)) - fn(0, 0, 64, [30, 7, setup], 64 * 7) < 64 * 200000
        plain = fn(64 * rounded, 64 * len(sizes), 64, [30, 7, setup], 64 * 7)
        assert bound - plain < 64 * 200000 / 8, (bound, plain)       # what the picture adds: its bytes and its pages' headers, once
        assert bound - plain < 1.01 * 200000 + 4096
