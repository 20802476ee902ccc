"""Files for the Ogg decode entry's tests (tests/test_demux_cpu.py on the host build, tests/test_decode_ogg_gpu.py on the
GPU): a plain page writer from doc/framing.html with tests/ogg_framing.py's CRC, which lays a stream's headers and audio
packets out under named cut policies no encoder has to follow; damaged files with the status bit the contract of
include/vorbis_amd.h ("Ogg Vorbis files in") gives them; seeded mutations of small files, and a reader that says, without
asserting, whether a file reads whole.  Nothing here comes from the code under test, except the `feed` policy's files,
which the shipped host mux writes.

What a file must decode to is the reference decoder over what tests/ogg_framing.py reads back from it (expected())."""
import struct

import numpy as np

from tests import decode_cases, ogg_framing, ref_host
from tests.ogg_framing import _crc

STATUS_BADPAGE, STATUS_BADHEADER = 32, 64  # include/vorbis_amd.h
POLICIES = ("feed", "one_packet", "full_255", "seeded", "shared", "big_comment")
SERIAL = 0x5eed0000
BIG_COMMENT = 131000  # bytes of the one tag: more than two pages of 255 x 255 body bytes that complete nothing
_files, _expected, _host = {}, {}, []


# ---- the page writer ----
def page(flags, granule, serial, seq, lacing, body):
    h = b"OggS\0" + bytes([flags]) + struct.pack("<qIII", granule, serial, seq, 0) + bytes([len(lacing)]) + bytes(lacing)
    return h[:22] + struct.pack("<I", _crc(h + body)) + h[26:] + body


def write(packets, granules, take, serial=SERIAL, empty_from=None):
    """packets with their granule positions -> a file.  A packet of n bytes is n // 255 lacing values of 255 and one of
    n % 255; take(seq, at, segs) says how many of the segments from `at` on the next page holds (cut to 1 .. 255 and to what
    is left); segs[i] = (lacing value, packet, whether it ends the packet).  empty_from: the first packet boundary at or
    behind that page number gets a page without segments."""
    segs = [(v, k, q == len(p) // 255) for k, p in enumerate(packets) for q, v in enumerate([255] * (len(p) // 255) + [len(p) % 255])]
    data, at, byte, seq, is_open, out = b"".join(packets), 0, 0, 0, False, []
    while at < len(segs):
        n = max(1, min(int(take(seq, at, segs)), 255, len(segs) - at))
        chunk = segs[at:at + n]
        size = sum(v for v, _, _ in chunk)
        done = [k for _, k, last in chunk if last]
        flags = (1 if is_open else 0) | (2 if seq == 0 else 0) | (4 if at + n == len(segs) else 0)
        out.append(page(flags, granules[done[-1]] if done else -1, serial, seq, [v for v, _, _ in chunk], data[byte:byte + size]))
        at, byte, seq, is_open = at + n, byte + size, seq + 1, not chunk[-1][2]
        if empty_from is not None and seq >= empty_from and not is_open and at < len(segs):
            out.append(page(0, -1, serial, seq, [], b""))
            seq, empty_from = seq + 1, None
    assert empty_from is None
    return b"".join(out)


def _to_packet_end(seq, at, segs, packets=1):
    n = 0
    while at + n < len(segs) and packets:
        packets -= segs[at + n][2]
        n += 1
    return n


def _shared(seq, at, segs):
    """the identification header alone, the comment header alone, the setup header with the first three audio packets,
    then four packets a page"""
    return _to_packet_end(seq, at, segs, 1 if seq < 2 else 4)


def packet_granules(packets, end, bs):
    """the granule position behind each audio packet, as the encoder counts them (lib/block.c:840-842): the centres are
    bs[lW] / 4 + bs[W] / 4 apart, the first at 0; the last packet's is the stream's length"""
    Ws = [(p[0] >> 1) & 1 if bs[0] != bs[1] else 0 for p in packets]
    out, at = [], 0
    for i in range(len(packets)):
        at += bs[Ws[i - 1]] // 4 + bs[Ws[i]] // 4 if i else 0
        out.append(at)
    if len(out) > 1:
        assert out[-2] < end <= out[-1], (out[-2:], end)
    if out:
        out[-1] = end
    return out


def make(headers, packets, end, bs, policy, seed=0):
    """one stream under a policy -> its file.  Beside POLICIES, for the damaged files: "singles", a segment a page, so that a
    stream of twenty packets has pages enough to damage, and every packet of 255 bytes and more lies across pages"""
    gr = packet_granules(packets, end, bs)
    if policy == "feed":
        if not _host:
            from tests.ogg_host import HostOgg
            _host.append(HostOgg())
        return _host[0].mux(headers, packets, gr, SERIAL + seed)
    if policy == "big_comment":
        from vorbis_amd import comment_packet
        headers = [headers[0], comment_packet([("BLOB", "x" * BIG_COMMENT)], "tests/ogg_demux_cases.py"), headers[2]]
    rng = np.random.default_rng(seed)
    take = {"one_packet": _to_packet_end, "full_255": lambda *a: 255, "big_comment": lambda *a: 255, "shared": _shared,
            "seeded": lambda *a: rng.integers(1, 256), "singles": lambda *a: 1}[policy]
    return write(list(headers) + list(packets), [0, 0, 0] + gr, take, SERIAL + seed, 3 if policy == "shared" else None)


def base_files(name, policy, seed=1):
    """decode_cases.base_streams(name) under a policy -> (setup blob, headers, [file] x 4)"""
    if (name, policy, seed) not in _files:
        blob, headers, bs, base = decode_cases.base_streams(name, seed)
        _files[name, policy, seed] = (blob, headers, [make(headers, p, end, bs, policy, 10 * seed + v) for v, (p, end) in enumerate(base)])
    return _files[name, policy, seed]


def group_files(g, policy):
    """a decode_cases.Group's streams (short_streams) under a policy -> [file]"""
    enc = ref_host.encoder(g.name)
    bs = (enc.blocksize(0), enc.blocksize(1))
    return [make(g.headers, p, end, bs, policy, s) for s, (p, end) in enumerate(zip(g.streams, g.ends))]


def expected(f, decode=True):
    """What the independent reader and the reference make of a well-formed file -> (audio packets, end granule, pcm):
    the end granule is that of the page that completes the last audio packet (-1 without one); pcm (read-only) is
    reference_decode over the packets with the granule positions their pages give them."""
    f = bytes(f)
    if f not in _expected:
        pages, packets = ogg_framing.demux(f)
        gr = ogg_framing.page_granules(pages, len(packets) - 3)
        _expected[f] = [packets, gr, None]
    packets, gr, want = _expected[f]
    if decode and want is None:
        want = ref_host.reference_decode(packets, gr)
        want.setflags(write=False)
        _expected[f][2] = want
    return packets[3:], (gr[-1] if gr else -1), want


# ---- damage ----
def reseal(f, offset):
    """the file with the checksum of the page at `offset` computed anew"""
    n = f[offset + 26]
    end = offset + 27 + n + sum(f[offset + 27:offset + 27 + n])
    pg = f[offset:end]
    return f[:offset + 22] + struct.pack("<I", _crc(pg[:22] + b"\0\0\0\0" + pg[26:])) + f[offset + 26:]


def _patch(f, at, value, seal=None):
    f = f[:at] + bytes([value]) + f[at + 1:]
    return reseal(f, seal) if seal is not None else f


def _audio_page(pages, rng, need=lambda p: True):
    """a page that holds audio bytes alone, not the first of them and not the last"""
    first = next(i for i, p in enumerate(pages) if sum(q["done"] for q in pages[:i]) >= 3)
    ok = [i for i in range(first + 1, len(pages) - 1) if need(pages[i])]
    return pages[ok[int(rng.integers(0, len(ok)))]]


def _d_body_bit(f, pages, rng, **_):
    p = _audio_page(pages, rng, lambda p: p["body"] > 0)
    at = p["offset"] + 27 + p["nseg"] + int(rng.integers(0, p["body"]))
    return _patch(f, at, f[at] ^ (1 << int(rng.integers(0, 8)))), STATUS_BADPAGE


def _d_granule_bit(f, pages, rng, **_):
    at = _audio_page(pages, rng)["offset"] + 6 + int(rng.integers(0, 8))
    return _patch(f, at, f[at] ^ (1 << int(rng.integers(0, 8)))), STATUS_BADPAGE


def _d_capture(f, pages, rng, **_):
    o = _audio_page(pages, rng)["offset"]
    return _patch(f, o + 3, ord("X"), o), STATUS_BADPAGE


def _d_version(f, pages, rng, **_):
    o = _audio_page(pages, rng)["offset"]
    return _patch(f, o + 4, 1, o), STATUS_BADPAGE


def _d_page_removed(f, pages, rng, **_):
    p = _audio_page(pages, rng)
    return f[:p["offset"]] + f[p["offset"] + p["bytes"]:], STATUS_BADPAGE


def _d_serial(f, pages, rng, **_):
    o = _audio_page(pages, rng)["offset"]
    return _patch(f, o + 15, f[o + 15] ^ 0x40, o), STATUS_BADPAGE


def _d_continued(f, pages, rng, **_):
    o = _audio_page(pages, rng)["offset"]
    return _patch(f, o + 5, f[o + 5] ^ 1, o), STATUS_BADPAGE


def _d_bos_page3(f, pages, rng, **_):
    o = pages[3]["offset"]
    return _patch(f, o + 5, f[o + 5] | 2, o), STATUS_BADPAGE


def _d_cut_header(f, pages, rng, **_):
    return f[:_audio_page(pages, rng)["offset"] + int(rng.integers(1, 27))], STATUS_BADPAGE


def _d_cut_lacing(f, pages, rng, **_):
    p = _audio_page(pages, rng, lambda p: p["nseg"] > 0)
    return f[:p["offset"] + 27 + int(rng.integers(0, p["nseg"]))], STATUS_BADPAGE


def _d_cut_body(f, pages, rng, **_):
    p = _audio_page(pages, rng, lambda p: p["body"] > 0)
    return f[:p["offset"] + 27 + p["nseg"] + int(rng.integers(0, p["body"]))], STATUS_BADPAGE


def _d_cut_in_packet(f, pages, rng, **_):
    p = _audio_page(pages, rng, lambda p: p["open"])
    return f[:p["offset"] + p["bytes"]], STATUS_BADPAGE


def _d_cut_between(f, pages, rng, **_):
    """a cut at a page boundary between packets: a shorter stream, clean"""
    p = _audio_page(pages, rng, lambda p: not p["open"])
    return f[:p["offset"] + p["bytes"]], 0


def _d_ident_channels(f, pages, rng, **_):
    at = pages[0]["offset"] + 27 + pages[0]["nseg"] + 11
    return _patch(f, at, f[at] + 1, pages[0]["offset"]), STATUS_BADHEADER


def _d_setup_byte(f, pages, rng, headers, **_):
    """one byte of the setup header (behind its type and "vorbis"), wherever its pages put it"""
    k = 7 + int(rng.integers(0, len(headers[2]) - 7))
    at = len(headers[0]) + len(headers[1]) + k  # the byte's place among the body bytes
    for p in pages:
        if at < p["body"]:
            return _patch(f, p["offset"] + 27 + p["nseg"] + at, f[p["offset"] + 27 + p["nseg"] + at] ^ 0x10, p["offset"]), STATUS_BADHEADER
        at -= p["body"]
    raise AssertionError("no setup header")


def _d_two_headers(f, pages, rng, headers, **_):
    return write(list(headers[:2]), [0, 0], _to_packet_end), STATUS_BADHEADER


def _d_chained(f, pages, rng, **_):
    """a second logical stream behind the first: the same pages under another serial number"""
    other = b""
    for p in pages:
        o = len(other)
        other = reseal(other + _patch(f[p["offset"]:p["offset"] + p["bytes"]], 14, f[p["offset"] + 14] ^ 1), o)
    return f + other, STATUS_BADPAGE


DAMAGE = {"body_bit": _d_body_bit, "granule_bit": _d_granule_bit, "capture": _d_capture, "version": _d_version,
          "page_removed": _d_page_removed, "serial": _d_serial, "continued": _d_continued, "bos_page3": _d_bos_page3,
          "cut_header": _d_cut_header, "cut_lacing": _d_cut_lacing, "cut_body": _d_cut_body, "cut_in_packet": _d_cut_in_packet,
          "cut_between": _d_cut_between, "ident_channels": _d_ident_channels, "setup_byte": _d_setup_byte,
          "two_headers": _d_two_headers, "chained": _d_chained}
_damaged = {}


class Damaged:
    """files: per damage kind an untouched base stream's file and then the damaged one (so the clean streams are as many
    and lie between them, and the group ends on a damaged one); kind[s]: None or the damage; bit[s]: the status bit the
    contract gives stream s, 0 for a clean one; setup_header: what every file's third packet must equal"""

    def __init__(self, name, seed=1):
        self.name = name
        self.blob, headers, singles = base_files(name, "singles", seed)
        _, _, seeded = base_files(name, "seeded", seed)
        _, _, single = base_files(name, "one_packet", seed)
        self.setup_header, self.files, self.kind, self.bit = headers[2], [], [], []
        rng = np.random.default_rng(seed)
        for i, (kind, fn) in enumerate(DAMAGE.items()):
            clean = (single if i & 1 else seeded)[(i + 1) % 4]
            base = singles[i % 4]
            f, bit = fn(base, ogg_framing.demux(base)[0], rng, headers=headers)
            assert f != base
            self.files += [clean, f]
            self.kind += [None, kind]
            self.bit += [0, bit]
        assert self.bit[-1] and 2 * sum(b == 0 for b in self.bit) >= len(self.bit)


def damaged(name):
    if name not in _damaged:
        _damaged[name] = Damaged(name)
    return _damaged[name]


# ---- a reader that does not assert ----
def _comment_ok(p):
    """Vorbis I 5.2.1 as far as its framing goes: type 3, "vorbis", the vendor's length and bytes, the comment count, each
    comment's length and bytes, the framing bit -- all inside the packet"""
    n = len(p)
    if n < 7 or n > 1 << 24 or p[:7] != b"\x03vorbis" or n - 7 < 4:
        return False
    at = 11 + struct.unpack_from("<I", p, 7)[0]
    if at > n or n - at < 4:
        return False
    count = struct.unpack_from("<I", p, at)[0]
    at += 4
    if count > (n - at) // 4:
        return False
    for _ in range(count):
        if n - at < 4:
            return False
        at += 4 + struct.unpack_from("<I", p, at)[0]
        if at > n:
            return False
    return at < n and bool(p[at] & 1)


def reads_whole(f, channels, rate, bs, setup_header=None):
    """tests/ogg_framing.py's reader with a verdict in place of its assertions, and the three headers looked at as the
    contract says: True where the file is one well-formed logical stream -- capture patterns, version, lengths inside the
    file, one serial number, sequence numbers from 0, continued flags that agree with "a packet is open", begin-of-stream
    on page 0 alone, correct checksums, no packet left open -- that begins with an identification header of this
    geometry, a well-formed comment header and a setup header (equal to setup_header where one is given)."""
    f = bytes(f)
    pos, seq, is_open, serial, packets, cur = 0, 0, False, None, [], b""
    while pos < len(f):
        if len(f) - pos < 27 or f[pos:pos + 4] != b"OggS" or f[pos + 4] != 0:
            return False
        flags, n = f[pos + 5], f[pos + 26]
        _, ser, sq, crc = struct.unpack("<qIII", f[pos + 6:pos + 26])
        lacing = f[pos + 27:pos + 27 + n]
        end = pos + 27 + n + sum(lacing)
        if len(lacing) < n or end > len(f):
            return False
        pg = f[pos:end]
        if _crc(pg[:22] + b"\0\0\0\0" + pg[26:]) != crc:
            return False
        serial = ser if serial is None else serial
        if ser != serial or sq != seq or (seq > 0 and flags & 2) or bool(flags & 1) != is_open:
            return False
        o = pos + 27 + n
        for v in lacing:
            cur, o, is_open = cur + f[o:o + v], o + v, True
            if v < 255:
                packets.append(cur)
                cur, is_open = b"", False
        pos, seq = end, seq + 1
    if is_open or len(packets) < 3:
        return False
    h = packets[0]
    if len(h) < 30 or h[:7] != b"\x01vorbis" or h[7:11] != b"\0\0\0\0" or h[11] != channels or struct.unpack_from("<I", h, 12)[0] != rate:
        return False
    if (1 << (h[28] & 15), 1 << (h[28] >> 4)) != tuple(bs):
        return False
    return _comment_ok(packets[1]) and packets[2][:7] == b"\x05vorbis" and (setup_header is None or packets[2] == bytes(setup_header))


# ---- seeded mutations of small files ----
def _reseal_all(f):
    """every page that still parses gets its checksum anew"""
    pos = 0
    while len(f) - pos >= 27 and f[pos:pos + 4] == b"OggS":
        n = f[pos + 26]
        end = pos + 27 + n + sum(f[pos + 27:pos + 27 + n])
        if len(f) - pos - 27 < n or end > len(f):
            break
        f, pos = reseal(f, pos), end
    return f


def mutations(files, count, seed=7):
    """count files: each one of `files` with random bytes changed, cut at a random length, a page's segment count or one of
    its lacing values replaced, or a byte of its header fields; half of them with every checksum made right again, so that
    what the walk itself says decides"""
    rng = np.random.default_rng(seed)
    out, read = [], [ogg_framing.demux(f)[0] for f in files]
    for i in range(count):
        k = int(rng.integers(0, len(files)))
        f, pages = files[k], read[k]
        p = pages[int(rng.integers(0, len(pages)))]
        kind = i % 6
        if kind == 0:
            for _ in range(int(rng.integers(1, 4))):
                at = int(rng.integers(0, len(f)))
                f = _patch(f, at, int(rng.integers(0, 256)))
        elif kind == 1:
            f = f[:int(rng.integers(0, len(f)))]
        elif kind == 2:
            f = _patch(f, p["offset"] + 26, int(rng.integers(0, 256)))
        elif kind == 3 and p["nseg"]:
            f = _patch(f, p["offset"] + 27 + int(rng.integers(0, p["nseg"])), int(rng.integers(0, 256)))
        elif kind == 4:
            f = _patch(f, p["offset"] + int(rng.integers(4, 22)), int(rng.integers(0, 256)))
        elif kind == 5 and p["body"]:  # a body byte: a header packet's or an audio packet's
            at = p["offset"] + 27 + p["nseg"] + int(rng.integers(0, p["body"]))
            f = _patch(f, at, f[at] ^ (1 << int(rng.integers(0, 8))))
        out.append(_reseal_all(f) if rng.integers(0, 2) else f)
    return out
