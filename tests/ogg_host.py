"""The shipped vorbis_amd/csrc/k_ogg.h compiled with the host compiler -- the header itself, not a sibling of it: the
paging walk, the chunked-and-combined CRC as k_ogg_pages computes it, the host mux whole and in pieces (ogg_mux_piece: the
resumed walk, the carry, a flush per group), the comment validator, and the bounds a group is sized by.

What its results are held against lies elsewhere and does not come from this header: tests/ogg_framing.py (the container
and the paging policy) and tests/ref_host.py (the reference build)."""
import ctypes as C

import numpy as np

from tests import hostbuild

_SHIM = r"""
#include "k_ogg.h"
using namespace vamd;
extern "C" unsigned crc_chunked(const uint8_t *data, long long n, int min_chunk, int lanes) { return ogg_crc_chunked(data, n, min_chunk, lanes); }
extern "C" unsigned crc_shipped_constants(const uint8_t *data, long long n) { return ogg_crc_chunked(data, n, OGG_CRC_MIN_CHUNK, OGG_CRC_LANES); }
extern "C" int page_bytes(void) { return (int)sizeof(OggPage); }
// header_bytes null: a bare audio run
extern "C" long long plan(const int32_t *header_bytes, long long npackets, const int32_t *bytes, const int64_t *granule, OggPage *pages,
                          long long cap, long long *file_bytes) {
  int64_t fb = 0;
  const int64_t np = ogg_plan_stream(header_bytes, npackets, bytes, granule, pages, cap, &fb);
  *file_bytes = fb;
  return np;
}
// the same through the packet-at-a-time walk (which the header runs use)
extern "C" long long plan_serial(long long npackets, const int32_t *bytes, const int64_t *granule, OggPage *pages, long long cap,
                                 long long *file_bytes) {
  OggWalk w;
  ogg_walk_init(w, 0);
  ogg_run_begin(w, 2, 0);
  for (long long k = 0; k < npackets; k++) ogg_walk_packet(w, pages, cap, (int32_t)k, bytes[k], granule[k]);
  ogg_run_end(w, pages, cap, 1);
  *file_bytes = w.file_off;
  return w.npages;
}
extern "C" long long mux(const uint8_t *const *headers, const int32_t *header_bytes, long long npackets, const uint8_t *const *packets,
                         const int32_t *bytes, const int64_t *granule, unsigned serial, uint8_t *out, long long cap, OggPage *pages,
                         long long page_cap, long long *npages) {
  int64_t np = 0;
  const int64_t total = ogg_mux(headers, header_bytes, npackets, packets, bytes, granule, serial, out, cap, pages, page_cap, &np);
  *npages = np;
  return total;
}
// the mux in pieces
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
extern "C" long long piece(OggPieces *T, int begin, const uint8_t *const *headers, const int32_t *header_bytes, long long npackets,
                           const uint8_t *const *packets, const int32_t *bytes, const int64_t *granule, int close, int flush,
                           unsigned serial, uint8_t *out, long long cap, OggPage *pages, long long page_cap, long long *npages,
                           OggPage *open_page) {
  int64_t np = 0;
  const int64_t total = ogg_mux_piece(*T, begin, headers, header_bytes, npackets, packets, bytes, granule, close, serial, out, cap, pages,
                                      page_cap, &np, open_page, flush);
  *npages = np;
  return total;
}
// the bounds
extern "C" long long slots(const int32_t *header_bytes, long long npackets, long long packet_cap) {
  return ogg_header_slots(header_bytes) + ogg_slots_per_packet(packet_cap) * npackets;
}
extern "C" long long live_slots(const int32_t *header_bytes, long long npackets, long long packet_cap) {
  return ogg_live_slots(header_bytes) + ogg_slots_per_packet(packet_cap) * npackets;
}
extern "C" long long file_bound(long long packet_bytes, long long npackets, long long nstreams, const int32_t *header_bytes) {
  return ogg_file_bound(packet_bytes, npackets, nstreams, header_bytes);
}
extern "C" long long live_file_bound(long long packet_bytes, long long npackets, long long nstreams, const int32_t *header_bytes) {
  return ogg_live_file_bound(packet_bytes, npackets, nstreams, header_bytes);
}
extern "C" long long file_bound_v(long long packet_bytes, long long npackets, long long nstreams, const int32_t *header_bytes,
                                  long long comment_sum) {
  return ogg_file_bound_v(packet_bytes, npackets, nstreams, header_bytes, comment_sum);
}
extern "C" long long live_file_bound_v(long long packet_bytes, long long npackets, long long nstreams, const int32_t *header_bytes,
                                       long long comment_sum) {
  return ogg_live_file_bound_v(packet_bytes, npackets, nstreams, header_bytes, comment_sum);
}
// the comment validator
extern "C" int comment_check(const uint8_t *p, long long n) { return ogg_comment_check(p, n); }
extern "C" const char *comment_why(int code) { return ogg_comment_why(code); }
"""


class Page(C.Structure):  # vamd::OggPage
    _fields_ = [("file_off", C.c_int64), ("granule", C.c_int64)] + \
               [(k, C.c_int32) for k in ("run", "first", "byte0", "npackets", "nseg", "body", "seq", "flags", "stream", "done")]


def _page(p):
    return {k: getattr(p, k) for k, _ in Page._fields_}


def _sizes(v):
    return np.ascontiguousarray(v, dtype=np.int32)


class _Packets:
    """(headers, packets, granules) as the mux takes them: headers three packets, or None for a bare audio run.  `room`:
    what a carry may add to the bodies."""

    def __init__(self, headers, packets, granules, room, spare_pages):
        packets = [bytes(p) for p in packets]
        self.sizes, self.granules = _sizes([len(p) for p in packets]), np.ascontiguousarray(granules, dtype=np.int64)
        self._bufs = [C.create_string_buffer(p, max(len(p), 1)) for p in packets]
        self.ptrs = (C.c_void_p * max(len(self._bufs), 1))(*[C.cast(b, C.c_void_p) for b in self._bufs])
        self.header_ptrs, self.header_sizes = None, None
        if headers is not None:
            self._hbufs = [C.create_string_buffer(bytes(h), len(h)) for h in headers]
            self.header_ptrs = (C.c_void_p * 3)(*[C.cast(b, C.c_void_p) for b in self._hbufs])
            self._hb = _sizes([len(h) for h in headers])
            self.header_sizes = C.c_void_p(self._hb.ctypes.data)
        self.page_cap = int(self.sizes.size + (int(self.sizes.sum()) + room) // 255 + spare_pages)
        self.cap = int(self.sizes.sum()) + room + (sum(len(h) for h in headers) if headers else 0) + self.page_cap * 282
        self.out, self.pages, self.npages = np.zeros(self.cap, np.uint8), (Page * self.page_cap)(), C.c_longlong()

    def front(self):
        return (self.header_ptrs, self.header_sizes, C.c_longlong(self.sizes.size), self.ptrs, C.c_void_p(self.sizes.ctypes.data),
                C.c_void_p(self.granules.ctypes.data))

    def back(self):
        return (C.c_void_p(self.out.ctypes.data), C.c_longlong(self.cap), self.pages, C.c_longlong(self.page_cap), C.byref(self.npages))

    def result(self, total):
        assert 0 <= total <= self.cap and self.npages.value <= self.page_cap
        return self.out[:total].tobytes()


class HostOgg:
    def __init__(self):
        self.L = C.CDLL(hostbuild.shim("ogg", _SHIM))
        for name in ("plan", "plan_serial", "mux", "pieces_bytes", "pieces_carried", "piece", "slots", "live_slots", "file_bound",
                     "live_file_bound", "file_bound_v", "live_file_bound_v"):
            getattr(self.L, name).restype = C.c_longlong
        self.L.crc_chunked.restype = self.L.crc_shipped_constants.restype = C.c_uint32
        self.L.crc_chunked.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int]
        self.L.crc_shipped_constants.argtypes = [C.c_void_p, C.c_longlong]
        self.L.comment_check.argtypes = [C.c_void_p, C.c_longlong]
        self.L.comment_why.restype = C.c_char_p
        assert self.L.page_bytes() == C.sizeof(Page)
        self.carry_body, self.carry_bytes, self.flush_bit = self.L.carry_body(), self.L.carry_bytes(), self.L.live_flush_bit()

    def crc_chunked(self, data, min_chunk, lanes):
        buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
        return int(self.L.crc_chunked(buf.ctypes.data, len(data), min_chunk, lanes))

    def crc_shipped(self, data):
        buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
        return int(self.L.crc_shipped_constants(buf.ctypes.data, len(data)))

    def plan(self, sizes, granules, header_bytes=None, serial=False):
        """-> (pages as dicts, file bytes) of the walk over one stream's packet sizes: 64 packets at a time and a page per
        step, as k_ogg_plan runs it -- or (serial, audio run only) a packet at a time"""
        sizes, gr = _sizes(sizes), np.ascontiguousarray(granules, dtype=np.int64)
        cap = int(sizes.size + sizes.sum() // 255 + 8)
        pages = (Page * cap)()
        fb = C.c_longlong()
        hb = _sizes(header_bytes) if header_bytes is not None else None
        if serial:
            assert hb is None
            n = self.L.plan_serial(C.c_longlong(sizes.size), C.c_void_p(sizes.ctypes.data), C.c_void_p(gr.ctypes.data), pages,
                                   C.c_longlong(cap), C.byref(fb))
        else:
            n = self.L.plan(C.c_void_p(hb.ctypes.data) if hb is not None else None, C.c_longlong(sizes.size), C.c_void_p(sizes.ctypes.data),
                            C.c_void_p(gr.ctypes.data), pages, C.c_longlong(cap), C.byref(fb))
        assert n <= cap
        return [_page(pages[i]) for i in range(n)], fb.value

    def mux(self, headers, packets, granules, serial):
        """The shipped host mux: headers (three packets, or None for a bare audio run), the audio packets -> the file"""
        m = _Packets(headers, packets, granules, 0, 16)
        return m.result(self.L.mux(*m.front(), C.c_uint32(serial), *m.back()))

    def stream(self, headers, serial):
        return Stream(self, headers, serial)

    def check(self, packet):
        """ogg_comment_check: 0 where the packet is a well-formed comment header, else what is wrong (a code)"""
        packet = bytes(packet)
        buf = C.create_string_buffer(packet, max(len(packet), 1))   # (exactly as long: a read past the end is a read past the buffer)
        return int(self.L.comment_check(C.cast(buf, C.c_void_p), len(packet)))

    def why(self, code):
        return self.L.comment_why(code).decode()

    def slots(self, header_bytes, npackets, packet_cap, live=False):
        hb = _sizes(header_bytes)
        return int((self.L.live_slots if live else self.L.slots)(C.c_void_p(hb.ctypes.data), C.c_longlong(npackets), C.c_longlong(packet_cap)))

    def live_slots(self, header_bytes, npackets, packet_cap):
        return self.slots(header_bytes, npackets, packet_cap, live=True)

    def _bound(self, fn, packet_bytes, npackets, nstreams, header_bytes, *comment_sum):
        hb = _sizes(header_bytes)
        return int(fn(C.c_longlong(packet_bytes), C.c_longlong(npackets), C.c_longlong(nstreams), C.c_void_p(hb.ctypes.data),
                      *[C.c_longlong(v) for v in comment_sum]))

    def file_bound(self, packet_bytes, npackets, nstreams, header_bytes):
        return self._bound(self.L.file_bound, packet_bytes, npackets, nstreams, header_bytes)

    def file_bound_v(self, packet_bytes, npackets, nstreams, header_bytes, comment_sum):
        return self._bound(self.L.file_bound_v, packet_bytes, npackets, nstreams, header_bytes, comment_sum)

    def live_file_bound(self, packet_bytes, npackets, nstreams, header_bytes, comment_sum=None):
        if comment_sum is None:
            return self._bound(self.L.live_file_bound, packet_bytes, npackets, nstreams, header_bytes)
        return self.live_file_bound_v(packet_bytes, npackets, nstreams, header_bytes, comment_sum)

    def live_file_bound_v(self, packet_bytes, npackets, nstreams, header_bytes, comment_sum):
        return self._bound(self.L.live_file_bound_v, packet_bytes, npackets, nstreams, header_bytes, comment_sum)


class Stream:
    """One stream through the shipped mux in pieces: piece(packets, granules, close, flush) -> the bytes of the pages the
    group hands out.  After each call: npages and pages (the group's page table as dicts), open_page (the page left open,
    before its rebase), ncarry, carried / carried_rounded (the carry's bytes; with each packet at a multiple of 4, as the
    device keeps them)."""

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
        m, left = _Packets(self.headers, packets, granules, self.host.carry_body, 300), Page()
        total = self.L.piece(self.T, C.c_int(0 if self.begun else 1), *m.front(), C.c_int(int(bool(close))), C.c_int(int(bool(flush))),
                             C.c_uint32(self.serial), *m.back(), C.byref(left))
        piece = m.result(total)
        self.begun = not close
        self.npages = int(m.npages.value)
        self.pages = [_page(m.pages[i]) for i in range(self.npages)]
        self.open_page = _page(left)
        self.ncarry = int(self.L.pieces_ncarry(self.T))
        self.carried = int(self.L.pieces_carried(self.T, 0))
        self.carried_rounded = int(self.L.pieces_carried(self.T, 1))
        return piece
