"""What the Ogg feed's tests stand on.

* The oracle for the CONTAINER, written from doc/framing.html alone and independent of vorbis_amd/csrc/k_ogg.h: a
  bit-serial CRC and a demuxer (capture pattern, version, flags, granule position, serial, sequence number, checksum,
  lacing, packets reassembled across pages; the continued flag must agree with "a packet is open").
* The oracle for the CONTENTS, through ctypes on the reference build (oracle/_ref/libvorbis_ref.so): the three header
  packets vorbis_analysis_headerout() gives, and the reference decoder over a demuxed file's packets.
* The shipped k_ogg.h compiled with the host compiler -- the header itself, not a sibling of it: the paging walk, the
  chunked-and-combined CRC as k_ogg_pages computes it, and the host mux."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FILL, MIN_PACKETS = 4096, 4  # the paging policy (include/vorbis_amd.h, "the Ogg feed")


# ---- from framing.html ----
def crc_bitserial(data):
    """polynomial 0x04c11db7, initial value 0, no final XOR, most significant bit first, one bit at a time"""
    r = 0
    for b in bytes(data):
        r ^= b << 24
        for _ in range(8):
            r = ((r << 1) ^ 0x04c11db7) & 0xffffffff if r & 0x80000000 else (r << 1) & 0xffffffff
    return r


def demux(f):
    """-> (pages, packets): every page's fields (and how many packets it completes), the packets put together again.
    Asserts what framing.html asks of a well-formed single stream."""
    f = bytes(f)
    pos, pages, packets, open_packet, is_open = 0, [], [], b"", False
    while pos < len(f):
        assert f[pos:pos + 4] == b"OggS", "capture pattern at %d" % pos
        assert f[pos + 4] == 0, "stream structure version"
        flags = f[pos + 5]
        gp, serial, seq, crc = struct.unpack("<qIII", f[pos + 6:pos + 26])
        n = f[pos + 26]
        lacing = list(f[pos + 27:pos + 27 + n])
        assert len(lacing) == n, "file ends inside a lacing table"
        body = f[pos + 27 + n:pos + 27 + n + sum(lacing)]
        assert len(body) == sum(lacing), "file ends inside a page body"
        zeroed = f[pos:pos + 22] + b"\0\0\0\0" + f[pos + 26:pos + 27 + n] + body
        assert crc_bitserial(zeroed) == crc, "checksum of page %d" % len(pages)
        assert bool(flags & 1) == is_open, "continued flag of page %d" % len(pages)
        assert not flags & ~7
        o = done = 0
        for v in lacing:
            open_packet += body[o:o + v]
            o += v
            is_open = True
            if v < 255:
                packets.append(open_packet)
                open_packet, is_open = b"", False
                done += 1
        pages.append(dict(flags=flags, granule=gp, serial=serial, seq=seq, nseg=n, body=len(body), done=done, offset=pos,
                          bytes=27 + n + len(body)))
        pos += 27 + n + len(body)
    assert not is_open, "the file ends inside a packet"
    return pages, packets


def page_granules(pages, npackets, nheaders=3):
    """Per audio packet the granule position a demuxer can give a decoder: the page's, on the last packet the page
    completes; -1 elsewhere."""
    out = [-1] * npackets
    k = -nheaders
    for p in pages:
        k += p["done"]
        if p["done"] and k > 0:
            out[k - 1] = p["granule"]
    return out


def check_policy(pages, first_audio_page):
    """The policy's page-level rules over a demuxed file's audio pages (or a bare run's pages)."""
    audio = pages[first_audio_page:]
    for i, p in enumerate(audio):
        assert 1 <= p["nseg"] <= 255
        if i + 1 < len(audio):
            assert (p["body"] > FILL and p["done"] >= MIN_PACKETS) or p["nseg"] == 255, (i, p)
        assert bool(p["flags"] & 4) == (i + 1 == len(audio)), (i, p)
        if p["done"] == 0:
            assert p["granule"] == -1
    for i, p in enumerate(pages):
        assert p["seq"] == i


# ---- the reference build ----
class OggPacket(C.Structure):  # ogg_packet (oracle/shim/ogg/ogg.h)
    _fields_ = [("packet", C.c_void_p), ("bytes", C.c_long), ("b_o_s", C.c_long), ("e_o_s", C.c_long),
                ("granulepos", C.c_int64), ("packetno", C.c_int64)]


def _reflib():
    from oracle import ref
    L = C.CDLL(ref.LIB_PATH)
    for name in ("vorbis_info_init", "vorbis_comment_init", "vorbis_info_clear", "vorbis_comment_clear", "vorbis_dsp_clear"):
        getattr(L, name).argtypes = [C.c_void_p]
    return L


def reference_headers(ch, rate, q=None, managed=None, tags=(("ENCODER", "vorbis_amd feed"),)):
    """[identification, comment, setup] of vorbis_analysis_headerout() for vorbis_encode_init_vbr(ch, rate, q), or for
    vorbis_encode_init(ch, rate, *managed) with managed = (max, nominal, min)."""
    L = _reflib()
    vi, vc, vd = (C.create_string_buffer(4096) for _ in range(3))
    L.vorbis_info_init(vi)
    if managed is None:
        L.vorbis_encode_init_vbr.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_float]
        assert L.vorbis_encode_init_vbr(vi, ch, rate, q) == 0
    else:
        L.vorbis_encode_init.argtypes = [C.c_void_p] + [C.c_long] * 5
        assert L.vorbis_encode_init(vi, ch, rate, *[int(v) for v in managed]) == 0
    L.vorbis_comment_init(vc)
    L.vorbis_comment_add_tag.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    for k, v in tags:
        L.vorbis_comment_add_tag(vc, k.encode(), v.encode())
    L.vorbis_analysis_init.argtypes = [C.c_void_p, C.c_void_p]
    assert L.vorbis_analysis_init(vd, vi) == 0
    ops = (OggPacket * 3)()
    L.vorbis_analysis_headerout.argtypes = [C.c_void_p] * 5
    assert L.vorbis_analysis_headerout(vd, vc, C.byref(ops[0]), C.byref(ops[1]), C.byref(ops[2])) == 0
    out = [C.string_at(o.packet, o.bytes) for o in ops]
    L.vorbis_dsp_clear(vd)
    L.vorbis_comment_clear(vc)
    L.vorbis_info_clear(vi)
    return out


def reference_decode(packets, granules):
    """The reference decoder over a demuxed file: packets = the three headers, then the audio packets; granules[i] the
    granule position of audio packet i where its page gives one, else -1 (page_granules); e_o_s on the last packet.
    -> float32 [channels, frames]"""
    L = _reflib()
    vi, vc, vd, vb = (C.create_string_buffer(4096) for _ in range(4))
    L.vorbis_info_init(vi)
    L.vorbis_comment_init(vc)
    keep = []

    def op(i, p, gp=-1, eos=0):
        b = C.create_string_buffer(bytes(p), len(p))
        keep.append(b)
        return OggPacket(C.cast(b, C.c_void_p), len(p), 1 if i == 0 else 0, eos, gp, i)
    L.vorbis_synthesis_headerin.argtypes = [C.c_void_p] * 3
    for i in range(3):
        o = op(i, packets[i], 0)
        r = L.vorbis_synthesis_headerin(vi, vc, C.byref(o))
        assert r == 0, "vorbis_synthesis_headerin(%d) = %d" % (i, r)
    L.vorbis_synthesis_init.argtypes = [C.c_void_p] * 2
    L.vorbis_block_init.argtypes = [C.c_void_p] * 2
    L.vorbis_synthesis.argtypes = [C.c_void_p] * 2
    L.vorbis_synthesis_blockin.argtypes = [C.c_void_p] * 2
    L.vorbis_synthesis_pcmout.argtypes = [C.c_void_p] * 2
    L.vorbis_synthesis_read.argtypes = [C.c_void_p, C.c_int]
    L.vorbis_block_clear.argtypes = [C.c_void_p]
    assert L.vorbis_synthesis_init(vd, vi) == 0
    L.vorbis_block_init(vd, vb)
    ch = C.cast(vi, C.POINTER(C.c_int))[1]  # vorbis_info.channels
    pcm = C.POINTER(C.POINTER(C.c_float))()
    out = [[np.zeros(0, np.float32)] for _ in range(ch)]
    for i in range(3, len(packets)):
        o = op(i, packets[i], granules[i - 3], 1 if i == len(packets) - 1 else 0)
        if L.vorbis_synthesis(vb, C.byref(o)) == 0:
            L.vorbis_synthesis_blockin(vd, vb)
        while True:
            n = L.vorbis_synthesis_pcmout(vd, C.byref(pcm))
            if n <= 0:
                break
            for c in range(ch):
                out[c].append(np.ctypeslib.as_array(pcm[c], (n,)).copy())
            L.vorbis_synthesis_read(vd, n)
    L.vorbis_block_clear(vb)
    L.vorbis_dsp_clear(vd)
    L.vorbis_comment_clear(vc)
    L.vorbis_info_clear(vi)
    return np.stack([np.concatenate(o) for o in out])


# ---- the shipped k_ogg.h on the host ----
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
extern "C" long long slots(const int32_t *header_bytes, long long npackets, long long packet_cap) {
  return ogg_header_slots(header_bytes) + ogg_slots_per_packet(packet_cap) * npackets;
}
extern "C" long long file_bound(long long packet_bytes, long long npackets, long long nstreams, const int32_t *header_bytes) {
  return ogg_file_bound(packet_bytes, npackets, nstreams, header_bytes);
}
"""


class Page(C.Structure):  # vamd::OggPage
    _fields_ = [("file_off", C.c_int64), ("granule", C.c_int64)] + \
               [(k, C.c_int32) for k in ("run", "first", "byte0", "npackets", "nseg", "body", "seq", "flags", "stream", "done")]


def build(outdir):
    src = os.path.join(outdir, "ogg_shim.cpp")
    lib = os.path.join(outdir, "libogg_host.so")
    with open(src, "w") as f:
        f.write(_SHIM)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "vorbis_amd", "csrc"), src, "-o", lib])
    return lib


class HostOgg:
    def __init__(self, lib):
        self.L = C.CDLL(lib)
        for name in ("plan", "plan_serial", "mux", "slots", "file_bound"):
            getattr(self.L, name).restype = C.c_longlong
        self.L.crc_chunked.restype = self.L.crc_shipped_constants.restype = C.c_uint32
        self.L.crc_chunked.argtypes = [C.c_void_p, C.c_longlong, C.c_int, C.c_int]
        self.L.crc_shipped_constants.argtypes = [C.c_void_p, C.c_longlong]
        assert self.L.page_bytes() == C.sizeof(Page)

    def crc_chunked(self, data, min_chunk, lanes):
        buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
        return int(self.L.crc_chunked(buf.ctypes.data, len(data), min_chunk, lanes))

    def crc_shipped(self, data):
        buf = np.frombuffer(bytes(data) + b"\0", np.uint8)
        return int(self.L.crc_shipped_constants(buf.ctypes.data, len(data)))

    @staticmethod
    def _sizes(v):
        return np.ascontiguousarray(v, dtype=np.int32)

    def plan(self, sizes, granules, header_bytes=None, serial=False):
        """-> (pages as dicts, file bytes) of the walk over one stream's packet sizes: 64 packets at a time and a page per
        step, as k_ogg_plan runs it -- or (serial, audio run only) a packet at a time"""
        sizes, gr = self._sizes(sizes), np.ascontiguousarray(granules, dtype=np.int64)
        cap = int(sizes.size + sizes.sum() // 255 + 8)
        pages = (Page * cap)()
        fb = C.c_longlong()
        hb = self._sizes(header_bytes) if header_bytes is not None else None
        if serial:
            assert hb is None
            n = self.L.plan_serial(C.c_longlong(sizes.size), C.c_void_p(sizes.ctypes.data), C.c_void_p(gr.ctypes.data), pages,
                                   C.c_longlong(cap), C.byref(fb))
        else:
            n = self.L.plan(C.c_void_p(hb.ctypes.data) if hb is not None else None, C.c_longlong(sizes.size), C.c_void_p(sizes.ctypes.data),
                            C.c_void_p(gr.ctypes.data), pages, C.c_longlong(cap), C.byref(fb))
        assert n <= cap
        return [{k: getattr(pages[i], k) for k, _ in Page._fields_} for i in range(n)], fb.value

    def mux(self, headers, packets, granules, serial):
        """The shipped host mux: headers (three packets, or None for a bare audio run), the audio packets -> the file"""
        packets = [bytes(p) for p in packets]
        sizes, gr = self._sizes([len(p) for p in packets]), np.ascontiguousarray(granules, dtype=np.int64)
        bufs = [C.create_string_buffer(p, max(len(p), 1)) for p in packets]
        ptrs = (C.c_void_p * max(len(bufs), 1))(*[C.cast(b, C.c_void_p) for b in bufs])
        hp, hb = None, None
        if headers is not None:
            hbufs = [C.create_string_buffer(bytes(h), len(h)) for h in headers]
            hp = (C.c_void_p * 3)(*[C.cast(b, C.c_void_p) for b in hbufs])
            hb = self._sizes([len(h) for h in headers])
        cap_pages = int(sizes.size + sizes.sum() // 255 + 16)
        cap = int(sizes.sum() + (sum(len(h) for h in headers) if headers else 0) + cap_pages * 282)
        out = np.zeros(cap, np.uint8)
        pages = (Page * cap_pages)()
        npages = C.c_longlong()
        total = self.L.mux(hp, C.c_void_p(hb.ctypes.data) if hb is not None else None, C.c_longlong(sizes.size), ptrs,
                           C.c_void_p(sizes.ctypes.data), C.c_void_p(gr.ctypes.data), C.c_uint32(serial), C.c_void_p(out.ctypes.data),
                           C.c_longlong(cap), pages, C.c_longlong(cap_pages), C.byref(npages))
        assert 0 <= total <= cap and npages.value <= cap_pages
        return out[:total].tobytes()

    def slots(self, header_bytes, npackets, packet_cap):
        hb = self._sizes(header_bytes)
        return int(self.L.slots(C.c_void_p(hb.ctypes.data), C.c_longlong(npackets), C.c_longlong(packet_cap)))

    def file_bound(self, packet_bytes, npackets, nstreams, header_bytes):
        hb = self._sizes(header_bytes)
        return int(self.L.file_bound(C.c_longlong(packet_bytes), C.c_longlong(npackets), C.c_longlong(nstreams), C.c_void_p(hb.ctypes.data)))


def s16_streams(rng, ch, frames, kinds):
    """tests/test_feed.py's stream kinds (that module is marked gpu as a whole; the CPU suite takes them from here)"""
    from tests import test_feed
    return test_feed.s16_streams(rng, ch, frames, kinds)


def planar(pcm_s16):
    return np.ascontiguousarray((pcm_s16.astype(np.float32) / np.float32(32768.0)).T)
