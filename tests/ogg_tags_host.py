"""What the tests of the Ogg feed's comment headers per stream stand on, beside tests/ogg_host.py and
tests/ogg_live_host.py: the shipped k_ogg.h compiled with the host compiler once more, for the comment validator
(ogg_comment_check) and the bounds a group with comments of its own is sized by (ogg_file_bound_v,
ogg_live_file_bound_v) -- and the reference's own reading of a comment header: vorbis_synthesis_headerin over a
candidate, and the tags of a file's three headers through vorbis_comment_query."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import ogg_host as oh

_SHIM = r"""
#include "k_ogg.h"
using namespace vamd;
extern "C" int comment_check(const uint8_t *p, long long n) { return ogg_comment_check(p, n); }
extern "C" const char *comment_why(int code) { return ogg_comment_why(code); }
extern "C" long long file_bound_v(long long packet_bytes, long long npackets, long long nstreams, const int32_t *header_bytes,
                                  long long comment_sum) {
  return ogg_file_bound_v(packet_bytes, npackets, nstreams, header_bytes, comment_sum);
}
extern "C" long long live_file_bound_v(long long packet_bytes, long long npackets, long long nstreams, const int32_t *header_bytes,
                                       long long comment_sum) {
  return ogg_live_file_bound_v(packet_bytes, npackets, nstreams, header_bytes, comment_sum);
}
"""


def build(outdir):
    src = os.path.join(outdir, "ogg_tags_shim.cpp")
    lib = os.path.join(outdir, "libogg_tags_host.so")
    with open(src, "w") as f:
        f.write(_SHIM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(oh.ROOT, "include"),
                           "-I" + os.path.join(oh.ROOT, "vorbis_amd", "csrc"), src, "-o", lib])
    return lib


class TagsOgg:
    def __init__(self, lib):
        self.L = C.CDLL(lib)
        self.L.file_bound_v.restype = self.L.live_file_bound_v.restype = C.c_longlong
        self.L.comment_check.argtypes = [C.c_void_p, C.c_longlong]
        self.L.comment_why.restype = C.c_char_p

    def check(self, packet):
        """ogg_comment_check: 0 where the packet is a well-formed comment header, else what is wrong (a code)"""
        packet = bytes(packet)
        buf = C.create_string_buffer(packet, max(len(packet), 1))   # (exactly as long: a read past the end is a read past the buffer)
        return int(self.L.comment_check(C.cast(buf, C.c_void_p), len(packet)))

    def why(self, code):
        return self.L.comment_why(code).decode()

    def _bound(self, fn, packet_bytes, npackets, nstreams, header_bytes, comment_sum):
        hb = np.ascontiguousarray(header_bytes, dtype=np.int32)
        return int(fn(C.c_longlong(packet_bytes), C.c_longlong(npackets), C.c_longlong(nstreams), C.c_void_p(hb.ctypes.data),
                      C.c_longlong(comment_sum)))

    def file_bound_v(self, packet_bytes, npackets, nstreams, header_bytes, comment_sum):
        return self._bound(self.L.file_bound_v, packet_bytes, npackets, nstreams, header_bytes, comment_sum)

    def live_file_bound_v(self, packet_bytes, npackets, nstreams, header_bytes, comment_sum):
        return self._bound(self.L.live_file_bound_v, packet_bytes, npackets, nstreams, header_bytes, comment_sum)


# ---- the reference's reading of a comment header ----
class _Comment(C.Structure):  # vorbis_comment (include/vorbis/codec.h)
    _fields_ = [("user_comments", C.POINTER(C.c_void_p)), ("comment_lengths", C.POINTER(C.c_int)), ("comments", C.c_int),
                ("vendor", C.c_char_p)]


def _headerin(L, packets):
    """vorbis_synthesis_headerin over the packets in turn -> (the return codes, up to the first failure; vi, vc; buffers)"""
    vi, vc = C.create_string_buffer(4096), C.create_string_buffer(4096)
    L.vorbis_info_init(vi)
    L.vorbis_comment_init(vc)
    L.vorbis_synthesis_headerin.argtypes = [C.c_void_p] * 3
    keep, codes = [], []
    for i, p in enumerate(packets):
        p = bytes(p)
        b = C.create_string_buffer(p, max(len(p), 1))
        keep.append(b)
        o = oh.OggPacket(C.cast(b, C.c_void_p), len(p), 1 if i == 0 else 0, 0, 0, i)
        codes.append(int(L.vorbis_synthesis_headerin(vi, vc, C.byref(o))))
        if codes[-1]:
            break
    return codes, vi, vc, keep


def reference_headerin(ident, candidate):
    """The reference's vorbis_synthesis_headerin, given the identification header and then `candidate` as the second
    header packet -> its return code for the candidate (0: accepted)"""
    L = oh._reflib()
    codes, vi, vc, _ = _headerin(L, [ident, candidate])
    assert codes[0] == 0, "the identification header is refused: %d" % codes[0]
    L.vorbis_comment_clear(vc)
    L.vorbis_info_clear(vi)
    return codes[1]


def reference_tags(headers, keys):
    """A file's three headers through vorbis_synthesis_headerin -> (the vendor string, the number of comments, per key
    the values vorbis_comment_query returns, in order) -- bytes throughout"""
    L = oh._reflib()
    codes, vi, vc, _ = _headerin(L, headers)
    assert codes == [0, 0, 0], codes
    L.vorbis_comment_query.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.vorbis_comment_query.restype = C.c_char_p
    L.vorbis_comment_query_count.argtypes = [C.c_void_p, C.c_char_p]
    c = C.cast(vc, C.POINTER(_Comment)).contents
    vendor, count = c.vendor, int(c.comments)
    out = {}
    for k in keys:
        kb = k.encode()
        out[k] = [L.vorbis_comment_query(vc, kb, i) for i in range(L.vorbis_comment_query_count(vc, kb))]
    L.vorbis_comment_clear(vc)
    L.vorbis_info_clear(vi)
    return vendor, count, out


def sized_comment(nbytes, title, vendor="vorbis_amd tests"):
    """A comment header of exactly nbytes: a TITLE and a PAD tag that takes up the rest (printable, so that
    vorbis_comment_query hands it back whole).  -> (packet, tags)"""
    import vorbis_amd
    base = len(vorbis_amd.comment_packet([("TITLE", title), ("PAD", "")], vendor))
    assert nbytes >= base, (nbytes, base)
    rng = np.random.default_rng(nbytes)
    pad = bytes(rng.integers(0x30, 0x7b, nbytes - base, dtype=np.uint8)).decode("ascii")
    tags = [("TITLE", title), ("PAD", pad)]
    packet = vorbis_amd.comment_packet(tags, vendor)
    assert len(packet) == nbytes
    return packet, tags
