"""Host-side helpers around the bytes the library hands over: a packet out of its row, the Vorbis comment header, and the
block-switching marks of the detector's per-step flags.  Pure numpy / struct: no library, no GPU."""
import struct

import numpy as np


def packet_bytes(row, bits):
    """A packet as oggpack_get_buffer() / oggpack_bytes() hand it over: the first (bits+7)/8 bytes of its row."""
    nbytes = (int(bits) + 7) // 8
    if nbytes > len(row):
        raise ValueError("packet (%d bits) was cut off at its row length %d" % (bits, len(row)))
    return bytes(bytearray(row[:nbytes]))


def comment_packet(tags, vendor):
    """The Vorbis comment header (Vorbis I 5.2.1) of a vendor string and [(key, value), ...] -- str (UTF-8) or bytes --
    byte for byte what vorbis_commentheader_out() writes for comments added with vorbis_comment_add_tag(key, value)."""
    def raw(v):
        return v.encode("utf-8") if isinstance(v, str) else bytes(v)
    vendor = raw(vendor)
    out = [b"\x03vorbis", struct.pack("<I", len(vendor)), vendor, struct.pack("<I", len(tags))]
    for k, v in tags:
        entry = raw(k) + b"=" + raw(v)
        out += [struct.pack("<I", len(entry)), entry]
    return b"".join(out) + b"\x01"


def comment_fields(packet):
    """-> (vendor, [(key, value), ...]) of a comment header, as str; a comment without "=" comes back as (comment, "")."""
    p = bytes(packet)
    if p[:7] != b"\x03vorbis":
        raise ValueError("not a Vorbis comment header")
    def take(at):
        n, = struct.unpack_from("<I", p, at)
        if at + 4 + n > len(p):
            raise ValueError("the comment header is cut off")
        return p[at + 4:at + 4 + n], at + 4 + n
    vendor, at = take(7)
    count, = struct.unpack_from("<I", p, at)
    at, tags = at + 4, []
    for _ in range(count):
        entry, at = take(at)
        k, _, v = entry.partition(b"=")
        tags.append((k.decode("utf-8"), v.decode("utf-8")))
    if at >= len(p) or not p[at] & 1:
        raise ValueError("the comment header's framing bit is missing")
    return vendor.decode("utf-8"), tags


def envelope_marks(ret, first=0, marks=None):
    """Apply per-step flags to a mark array exactly as lib/envelope.c:241-258 does (host-side
    integer logic of the binding): step j = first + index."""
    n = first + len(ret) + 2
    if marks is None:
        marks = np.zeros(n, np.int32)
    elif len(marks) < n:
        marks = np.concatenate([marks, np.zeros(n - len(marks), np.int32)])
    for k, r in enumerate(ret):
        j = first + k
        marks[j + 2] = 0
        if r & 1:
            marks[j] = 1
            marks[j + 1] = 1
        if r & 2:
            marks[j] = 1
            if j > 0:
                marks[j - 1] = 1
    return marks
