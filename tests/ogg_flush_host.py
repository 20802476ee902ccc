"""What the flush tests of the live Ogg feed stand on, beside tests/ogg_live_host.py: the shipped k_ogg.h compiled with the
host compiler once more, for its mux in pieces WITH a flush per group (ogg_mux_piece's trailing parameter) and the bounds a
live group is sized by -- and a second implementation of the paging policy with flush points, in plain Python, written from
the policy text of include/vorbis_amd.h ("the Ogg feed", "a flush per write"): a segment at a time, from sizes and granule
positions alone."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import ogg_host as oh
from tests import ogg_live_host as olh

_SHIM = r"""
#include "k_ogg.h"
using namespace vamd;
extern "C" long long pieces_bytes(void) { return (long long)sizeof(OggPieces); }
extern "C" int carry_body(void) { return OGG_CARRY_BODY; }
extern "C" int carry_bytes(void) { return OGG_CARRY_BYTES; }
extern "C" int live_flush_bit(void) { return OGG_LIVE_FLUSH; }
extern "C" int pieces_ncarry(const OggPieces *T) { return T->ncarry; }
extern "C" long long pieces_carried(const OggPieces *T, int rounded) {
  long long n = 0;
  for (int j = 0; j < T->ncarry; j++) n += rounded ? (T->cbytes[j] + 3) / 4 * 4 : T->cbytes[j];
  return n;
}
extern "C" long long piece_flush(OggPieces *T, int begin, const uint8_t *const *headers, const int32_t *header_bytes, long long npackets,
                                 const uint8_t *const *packets, const int32_t *bytes, const int64_t *granule, int close, int flush,
                                 unsigned serial, uint8_t *out, long long cap, OggPage *pages, long long page_cap, long long *npages,
                                 OggPage *open_page) {
  int64_t np = 0;
  const int64_t total = ogg_mux_piece(*T, begin, headers, header_bytes, npackets, packets, bytes, granule, close, serial, out, cap, pages,
                                      page_cap, &np, open_page, flush);
  *npages = np;
  return total;
}
extern "C" long long live_slots(const int32_t *header_bytes, long long npackets, long long packet_cap) {
  return ogg_live_slots(header_bytes) + ogg_slots_per_packet(packet_cap) * npackets;
}
extern "C" long long live_file_bound(long long packet_bytes, long long npackets, long long nstreams, const int32_t *header_bytes) {
  return ogg_live_file_bound(packet_bytes, npackets, nstreams, header_bytes);
}
extern "C" long long live_file_bound_v(long long packet_bytes, long long npackets, long long nstreams, const int32_t *header_bytes,
                                       long long comment_sum) {
  return ogg_live_file_bound_v(packet_bytes, npackets, nstreams, header_bytes, comment_sum);
}
"""


def build(outdir):
    src = os.path.join(outdir, "ogg_flush_shim.cpp")
    lib = os.path.join(outdir, "libogg_flush_host.so")
    with open(src, "w") as f:
        f.write(_SHIM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(oh.ROOT, "include"),
                           "-I" + os.path.join(oh.ROOT, "vorbis_amd", "csrc"), src, "-o", lib])
    return lib


class FlushOgg:
    def __init__(self, lib):
        self.L = C.CDLL(lib)
        for name in ("pieces_bytes", "pieces_carried", "piece_flush", "live_slots", "live_file_bound", "live_file_bound_v"):
            getattr(self.L, name).restype = C.c_longlong
        self.carry_body, self.carry_bytes, self.flush_bit = self.L.carry_body(), self.L.carry_bytes(), self.L.live_flush_bit()

    def stream(self, headers, serial):
        return Stream(self, headers, serial)

    def slots(self, header_bytes, npackets, packet_cap):
        hb = np.ascontiguousarray(header_bytes, dtype=np.int32)
        return int(self.L.live_slots(C.c_void_p(hb.ctypes.data), C.c_longlong(npackets), C.c_longlong(packet_cap)))

    def file_bound(self, packet_bytes, npackets, nstreams, header_bytes, comment_sum=None):
        hb = np.ascontiguousarray(header_bytes, dtype=np.int32)
        if comment_sum is None:
            return int(self.L.live_file_bound(C.c_longlong(packet_bytes), C.c_longlong(npackets), C.c_longlong(nstreams), C.c_void_p(hb.ctypes.data)))
        return int(self.L.live_file_bound_v(C.c_longlong(packet_bytes), C.c_longlong(npackets), C.c_longlong(nstreams), C.c_void_p(hb.ctypes.data),
                                            C.c_longlong(comment_sum)))


class Stream:
    """One stream through the shipped mux in pieces: piece(packets, granules, close, flush) -> the bytes of the pages the
    group hands out.  After each call: npages and pages (the group's page table as dicts), open_page (the page left open,
    before its rebase), ncarry, carried / carried_rounded (the carry's bytes; with each packet at a multiple of 4)."""

    def __init__(self, host, headers, serial):
        self.host, self.L, self.serial = host, host.L, serial
        self.T = C.create_string_buffer(int(self.L.pieces_bytes()))
        self.headers = [bytes(h) for h in headers] if headers is not None else None
        self.begun = False
        self.npages, self.pages, self.open_page, self.ncarry, self.carried, self.carried_rounded = 0, [], None, 0, 0, 0

    def twin(self):
        """-> a second stream in this one's state (the walk, the open page, the carry)"""
        t = Stream(self.host, self.headers, self.serial)
        C.memmove(t.T, self.T, len(self.T))
        t.begun = self.begun
        return t

    def piece(self, packets, granules, close, flush=False):
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
        total = self.L.piece_flush(self.T, C.c_int(0 if self.begun else 1), hp, C.c_void_p(hb.ctypes.data) if hb is not None else None,
                                   C.c_longlong(sizes.size), ptrs, C.c_void_p(sizes.ctypes.data), C.c_void_p(gr.ctypes.data),
                                   C.c_int(int(bool(close))), C.c_int(int(bool(flush))), C.c_uint32(self.serial), C.c_void_p(out.ctypes.data),
                                   C.c_longlong(cap), pages, C.c_longlong(cap_pages), C.byref(npages), C.byref(left))
        assert 0 <= total <= cap and npages.value <= cap_pages
        self.begun = not close
        self.npages = int(npages.value)
        self.pages = [{k: getattr(pages[i], k) for k, _ in oh.Page._fields_} for i in range(self.npages)]
        self.open_page = {k: getattr(left, k) for k, _ in oh.Page._fields_}
        self.ncarry = int(self.L.pieces_ncarry(self.T))
        self.carried = int(self.L.pieces_carried(self.T, 0))
        self.carried_rounded = int(self.L.pieces_carried(self.T, 1))
        return out[:total].tobytes()


# ---- the second implementation: the policy text, a segment at a time ----
class PolicyModel:
    """The pages of one stream from packet sizes and granule positions, by the words of include/vorbis_amd.h: a packet of
    n bytes is n / 255 lacing values of 255 and one of n % 255; segments are taken in order; before a segment is taken
    the page is closed if it holds 255 segments; at a packet boundary it is closed once its body holds more than 4096
    bytes and at least four packets have been completed on it; the end of a run closes its page; a flush closes the open
    page if it holds a segment; flags 0x01 / 0x02 / 0x04; a page's granule position is that of the last packet completed
    on it, -1 if none.  group(...) -> the pages that group hands out, each a dict(nseg, body, done, flags, granule, seq,
    flushed)."""

    def __init__(self, header_bytes):
        self.header_bytes, self.seq, self.begun = header_bytes, 0, False
        self._fresh(0)

    def _fresh(self, flags):
        self.lacing, self.done, self.granule, self.flags = [], 0, -1, flags

    def _close(self, out, extra=0, flushed=False):
        out.append(dict(nseg=len(self.lacing), body=sum(self.lacing), done=self.done, flags=self.flags | extra, granule=self.granule,
                        seq=self.seq, flushed=flushed))
        self.seq += 1
        self._fresh(0)

    def _packet(self, out, n, granule):
        if self.lacing and sum(self.lacing) > oh.FILL and self.done >= oh.MIN_PACKETS:
            self._close(out)
        values = [255] * (n // 255) + [n % 255]
        for q, v in enumerate(values):
            if len(self.lacing) == 255:
                self._close(out)
            if not self.lacing and q:
                self.flags |= 1
            self.lacing.append(v)
        self.done, self.granule = self.done + 1, granule

    def _end_run(self, out, eos):
        if self.lacing:
            self._close(out, 4 if eos else 0)

    def group(self, sizes, granules, close, flush):
        out = []
        if not self.begun:
            self.begun, self.seq = True, 0
            if self.header_bytes is not None:
                self._fresh(2)
                self._packet(out, self.header_bytes[0], 0)
                self._end_run(out, False)
                self._packet(out, self.header_bytes[1], 0)
                self._packet(out, self.header_bytes[2], 0)
                self._end_run(out, False)
            self._fresh(0)
        for n, g in zip(sizes, granules):
            self._packet(out, n, g)
        if close:
            self._end_run(out, True)
            self.begun = False
        elif flush and self.lacing:
            self._close(out, flushed=True)
        return out


class Reassembler:
    """The packets a stream's pages (ogg_live_host.pages_of) complete, page after page; `open` the bytes of a packet not
    yet completed.  The continued flag must agree with it."""

    def __init__(self):
        self.packets, self.open, self.is_open = [], b"", False

    def take(self, pages):
        for p in pages:
            assert bool(p["flags"] & 1) == self.is_open, "continued flag of page %d" % p["seq"]
            o = 0
            for v in p["lacing"]:
                self.open += p["data"][o:o + v]
                o += v
                self.is_open = True
                if v < 255:
                    self.packets.append(self.open)
                    self.open, self.is_open = b"", False


pages_of = olh.pages_of
packets_of = olh.packets_of
