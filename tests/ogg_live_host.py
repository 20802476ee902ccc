"""What the live Ogg feed's tests stand on, beside tests/ogg_host.py: the shipped k_ogg.h compiled with the host compiler
once more, for its mux in pieces (ogg_mux_piece: the resumed walk, the carry) and the live bounds -- and a page reader
that, unlike ogg_host.demux, takes a PIECE of a file: whole pages, every checksum verified, but free to begin with a
continued packet and to end inside one."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from tests import ogg_host as oh

_SHIM = r"""
#include "k_ogg.h"
using namespace vamd;
extern "C" long long pieces_bytes(void) { return (long long)sizeof(OggPieces); }
extern "C" int carry_body(void) { return OGG_CARRY_BODY; }
extern "C" int carry_bytes(void) { return OGG_CARRY_BYTES; }
extern "C" int pieces_ncarry(const OggPieces *T) { return T->ncarry; }
extern "C" long long pieces_carried(const OggPieces *T, int rounded) {
  long long n = 0;
  for (int j = 0; j < T->ncarry; j++) n += rounded ? (T->cbytes[j] + 3) / 4 * 4 : T->cbytes[j];
  return n;
}
extern "C" long long piece(OggPieces *T, int begin, const uint8_t *const *headers, const int32_t *header_bytes, long long npackets,
                           const uint8_t *const *packets, const int32_t *bytes, const int64_t *granule, int close, unsigned serial,
                           uint8_t *out, long long cap, OggPage *pages, long long page_cap, long long *npages, OggPage *open_page) {
  int64_t np = 0;
  const int64_t total = ogg_mux_piece(*T, begin, headers, header_bytes, npackets, packets, bytes, granule, close, serial, out, cap, pages,
                                      page_cap, &np, open_page);
  *npages = np;
  return total;
}
extern "C" long long live_slots(const int32_t *header_bytes, long long npackets, long long packet_cap) {
  return ogg_live_slots(header_bytes) + ogg_slots_per_packet(packet_cap) * npackets;
}
extern "C" long long live_file_bound(long long packet_bytes, long long npackets, long long nstreams, const int32_t *header_bytes) {
  return ogg_live_file_bound(packet_bytes, npackets, nstreams, header_bytes);
}
"""


def build(outdir):
    src = os.path.join(outdir, "ogg_live_shim.cpp")
    lib = os.path.join(outdir, "libogg_live_host.so")
    with open(src, "w") as f:
        f.write(_SHIM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(oh.ROOT, "include"),
                           "-I" + os.path.join(oh.ROOT, "vorbis_amd", "csrc"), src, "-o", lib])
    return lib


class LiveOgg:
    def __init__(self, lib):
        self.L = C.CDLL(lib)
        for name in ("pieces_bytes", "pieces_carried", "piece", "live_slots", "live_file_bound"):
            getattr(self.L, name).restype = C.c_longlong
        self.carry_body, self.carry_bytes = self.L.carry_body(), self.L.carry_bytes()

    def stream(self, headers, serial):
        return Stream(self, headers, serial)

    def slots(self, header_bytes, npackets, packet_cap):
        hb = np.ascontiguousarray(header_bytes, dtype=np.int32)
        return int(self.L.live_slots(C.c_void_p(hb.ctypes.data), C.c_longlong(npackets), C.c_longlong(packet_cap)))

    def file_bound(self, packet_bytes, npackets, nstreams, header_bytes):
        hb = np.ascontiguousarray(header_bytes, dtype=np.int32)
        return int(self.L.live_file_bound(C.c_longlong(packet_bytes), C.c_longlong(npackets), C.c_longlong(nstreams), C.c_void_p(hb.ctypes.data)))


class Stream:
    """One stream through the shipped mux in pieces: piece(packets, granules, close) -> the bytes of the pages the group
    completes.  After each call: npages (of the group), open_page (the page left open, before its rebase), ncarry,
    carried / carried_rounded (the carry's bytes; with each packet at a multiple of 4, as the device keeps them)."""

    def __init__(self, host, headers, serial):
        self.host, self.L, self.serial = host, host.L, serial
        self.T = C.create_string_buffer(int(self.L.pieces_bytes()))
        self.headers = [bytes(h) for h in headers] if headers is not None else None
        self.begun = False
        self.npages, self.open_page, self.ncarry, self.carried, self.carried_rounded = 0, None, 0, 0, 0

    def piece(self, packets, granules, close):
        packets = [bytes(p) for p in packets]
        sizes, gr = np.ascontiguousarray([len(p) for p in packets], dtype=np.int32), np.ascontiguousarray(granules, dtype=np.int64)
        bufs = [C.create_string_buffer(p, max(len(p), 1)) for p in packets]
        ptrs = (C.c_void_p * max(len(bufs), 1))(*[C.cast(b, C.c_void_p) for b in bufs])
        hp, hb = None, None
        if self.headers is not None:
            hbufs = [C.create_string_buffer(h, len(h)) for h in self.headers]
            hp = (C.c_void_p * 3)(*[C.cast(b, C.c_void_p) for b in hbufs])
            hb = np.ascontiguousarray([len(h) for h in self.headers], dtype=np.int32)
        cap_pages = int(sizes.size + (int(sizes.sum()) + self.host.carry_body) // 255 + 300)
        cap = int(sizes.sum()) + self.host.carry_body + (sum(len(h) for h in self.headers) if self.headers else 0) + cap_pages * 282
        out = np.zeros(cap, np.uint8)
        pages = (oh.Page * cap_pages)()
        npages, left = C.c_longlong(), oh.Page()
        total = self.L.piece(self.T, C.c_int(0 if self.begun else 1), hp, C.c_void_p(hb.ctypes.data) if hb is not None else None,
                             C.c_longlong(sizes.size), ptrs, C.c_void_p(sizes.ctypes.data), C.c_void_p(gr.ctypes.data), C.c_int(int(bool(close))),
                             C.c_uint32(self.serial), C.c_void_p(out.ctypes.data), C.c_longlong(cap), pages, C.c_longlong(cap_pages),
                             C.byref(npages), C.byref(left))
        assert 0 <= total <= cap and npages.value <= cap_pages
        self.begun = not close
        self.npages = int(npages.value)
        self.open_page = {k: getattr(left, k) for k, _ in oh.Page._fields_}
        self.ncarry = int(self.L.pieces_ncarry(self.T))
        self.carried = int(self.L.pieces_carried(self.T, 0))
        self.carried_rounded = int(self.L.pieces_carried(self.T, 1))
        return out[:total].tobytes()


# ---- a piece of a file, from framing.html ----
_TABLE = [oh.crc_bitserial(bytes([i])) for i in range(256)]  # the bit-serial definition, a byte at a time
_verified = set()


def _crc(data):
    r = 0
    for b in data:
        r = ((r << 8) & 0xffffffff) ^ _TABLE[(r >> 24) ^ b]
    return r


def pages_of(piece):
    """-> the pages of a piece of a file: it must be a whole number of well-formed pages, each with a correct checksum.
    Unlike ogg_host.demux it may begin with a continued packet and end inside one.  Per page also `open` (its last
    lacing value is 255), its lacing values and its body."""
    f, pos, pages = bytes(piece), 0, []
    while pos < len(f):
        assert f[pos:pos + 4] == b"OggS", "capture pattern at %d" % pos
        assert f[pos + 4] == 0 and len(f) >= pos + 27
        flags = f[pos + 5]
        gp, serial, seq, crc = struct.unpack("<qIII", f[pos + 6:pos + 26])
        n = f[pos + 26]
        lacing = list(f[pos + 27:pos + 27 + n])
        assert len(lacing) == n, "the piece ends inside a lacing table"
        end = pos + 27 + n + sum(lacing)
        assert end <= len(f), "the piece ends inside a page body"
        page = f[pos:end]
        if page not in _verified:  # (the same page comes back under every cut)
            assert _crc(page[:22] + b"\0\0\0\0" + page[26:]) == crc, "checksum of the page at %d" % pos
            _verified.add(page)
        assert not flags & ~7
        pages.append(dict(flags=flags, granule=gp, serial=serial, seq=seq, nseg=n, body=sum(lacing), done=sum(v < 255 for v in lacing),
                          open=bool(lacing) and lacing[-1] == 255, bytes=end - pos, lacing=lacing, data=page[27 + n:]))
        pos = end
    return pages


def packets_of(pages):
    """-> the packets a run of pages (pages_of) completes, put together again; what an open last packet holds is dropped"""
    out, cur = [], b""
    for p in pages:
        o = 0
        for v in p["lacing"]:
            cur += p["data"][o:o + v]
            o += v
            if v < 255:
                out.append(cur)
                cur = b""
    return out
