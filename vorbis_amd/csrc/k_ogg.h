// k_ogg.h -- Ogg pages around the feed's packets (doc/framing.html: page layout, lacing, CRC; doc/a1-encapsulation-ogg.tex:
// how Vorbis I sits in Ogg).  Three parts, and the way back:
//   * the CRC: table-driven per byte, and the algebra that lets a page be summed in chunks -- the register after a message
//     M (initial value 0, no final XOR, MSb first) is M(x) x^32 mod P, so crc(A || B) = crc(A) x^(8 |B|) + crc(B): every
//     lane sums a contiguous chunk, and a log-step tree joins neighbours with one multiply mod P each;
//   * the paging walk: from a stream's packet sizes to its pages (the policy is fixed, include/vorbis_amd.h "the Ogg
//     feed"), in two forms that the CPU suite holds together: a packet at a time (the header runs), and 64 packets at a
//     time with a page per step (the audio run: prefix sums of the sizes, every packet asked at once where the page ends);
//   * the kernels: k_ogg_plan (a wave per stream runs the walk, sizes scanned into LDS 64 at a time) and k_ogg_pages (a
//     wave per page: header, lacing table, body gathered from the packets, CRC, written with aligned dword stores) -- and,
//     for a live feed, whose files arrive in pieces, k_ogg_carry: what lies on the page still open stays on the device,
//     unless the group flushes the stream (vamd_feed_ogg_flush): then the open page leaves with the group;
//   * files back to packets, for the decoder (vamd_decode_ogg), is k_demux.h: k_ogg_depage, a wave per page of a table the
//     host walked (vamd_demux.h) -- this file's chunked CRC held against the stored field, the audio bytes into a packed arena.
// The CRC functions and the walk are ONE body: the library compiles them for gfx950, the CPU suite compiles this very
// file with the host compiler (tests/ogg_host.py) together with the host-only mux at the end, which lays the same
// pages out byte by byte -- the second implementation of the policy that the GPU's files are held against.
#pragma once
#include <stdint.h>
#include <string.h>
#if !defined(__HIP_DEVICE_COMPILE__)
#include <vector>
#endif

#if defined(__HIPCC__)
#define VAMD_OGG_FN __host__ __device__ inline
#else
#define VAMD_OGG_FN inline
#endif

namespace vamd {

enum {
  OGG_HEADER = 27,       // bytes of a page header in front of its lacing table
  OGG_MAX_SEGS = 255,    // segments a page holds at most
  OGG_FILL = 4096,       // a page is closed at a packet boundary once its body holds MORE than this ...
  OGG_MIN_PACKETS = 4,   // ... and at least this many packets have been completed on it
  OGG_CRC_LANES = 64,    // k_ogg_pages: chunks a page is summed in
  OGG_CRC_MIN_CHUNK = 16, // ... none shorter than this (a short page leaves its first lanes empty)
  // a live stream's carry: the packets with a segment on its open page -- at most 255 of them, 255 * 255 body bytes; on
  // the device each at a multiple of 4, and 18 bytes behind them that k_ogg_pages' whole-word reads may touch
  OGG_CARRY_BODY = OGG_MAX_SEGS * OGG_MAX_SEGS,
  OGG_CARRY_BYTES = OGG_CARRY_BODY + 3 * OGG_MAX_SEGS + 18
};
#define VAMD_OGG_POLY 0x04c11db7u

// ---- CRC (framing.html: polynomial 0x04c11db7, direct, initial value and final XOR 0, MSb first) ----
VAMD_OGG_FN uint32_t ogg_crc_entry(uint32_t byte) {  // entry `byte` of the 256-entry table
  uint32_t r = byte << 24;
  for (int i = 0; i < 8; i++) r = (r & 0x80000000u) ? (r << 1) ^ VAMD_OGG_POLY : r << 1;
  return r;
}
VAMD_OGG_FN uint32_t ogg_crc_byte(const uint32_t *table, uint32_t crc, uint32_t byte) {
  return (crc << 8) ^ table[((crc >> 24) ^ byte) & 0xffu];
}
// a * b mod P (bit i of a word is the coefficient of x^i): Horner over b's bits, 32 shift-and-xor steps
VAMD_OGG_FN uint32_t ogg_crc_mul(uint32_t a, uint32_t b) {
  uint32_t r = 0;
  for (int i = 31; i >= 0; i--) {
    r = (r & 0x80000000u) ? (r << 1) ^ VAMD_OGG_POLY : r << 1;
    if ((b >> i) & 1u) r ^= a;
  }
  return r;
}
// x^(8 n) mod P: what n more bytes multiply a CRC register by
VAMD_OGG_FN uint32_t ogg_crc_xpow8(int64_t n) {
  uint32_t r = 1u, base = 0x100u;
  while (n > 0) {
    if (n & 1) r = ogg_crc_mul(r, base);
    base = ogg_crc_mul(base, base);
    n >>= 1;
  }
  return r;
}
// The chunks of an n-byte page over `lanes` lanes: all of length c, laid from the page's END backwards, so that what lies
// behind any lane's chunk is a whole number of chunks (the short one is the first, in front of which nothing is summed;
// lanes before it are empty and hold a CRC of 0).  Lane l sums bytes [lo, hi).
VAMD_OGG_FN int64_t ogg_crc_chunk(int64_t n, int lanes, int min_chunk) {
  int64_t c = (n + lanes - 1) / lanes;
  if (c < min_chunk) c = min_chunk;
  return c < 1 ? 1 : c;
}
VAMD_OGG_FN void ogg_crc_range(int64_t n, int lanes, int64_t c, int lane, int64_t *lo, int64_t *hi) {
  const int64_t h = n - (int64_t)(lanes - 1 - lane) * c, l = h - c;
  *hi = h < 0 ? 0 : h;
  *lo = l < 0 ? 0 : l;
}
// one step of the tree: `mine` sums a run of chunks, `right` the equally long run behind it, m = x^(8 * that run's bytes)
VAMD_OGG_FN uint32_t ogg_crc_join(uint32_t mine, uint32_t right, uint32_t m) { return ogg_crc_mul(mine, m) ^ right; }

// ---- lacing ----
// A packet of n bytes is n / 255 segments of 255 and one of n % 255 (a multiple of 255 ends in a 0).
VAMD_OGG_FN int32_t ogg_segments(int32_t bytes) { return bytes / 255 + 1; }
VAMD_OGG_FN int32_t ogg_lace_value(int32_t bytes, int32_t q) { return q < bytes / 255 ? 255 : bytes % 255; }  // segment q of the packet
// bytes of the `take` segments of a packet from byte `start` (a multiple of 255) on
VAMD_OGG_FN int32_t ogg_piece_len(int32_t bytes, int32_t start, int32_t take) {
  return start / 255 + take == ogg_segments(bytes) ? bytes - start : take * 255;
}

// ---- the paging walk ----
// A stream's file is three RUNS of packets, each starting on a fresh page: the identification header alone (page 0, 58
// bytes with a 30-byte header), the comment and setup headers, the audio packets.  Within a run the walk takes segments
// in order; before taking one it closes the page if the page holds 255 segments, wherever that falls; before a packet's
// first segment it closes the page if its body holds more than OGG_FILL bytes and OGG_MIN_PACKETS packets have been
// completed on it; the end of a run closes its page.  A page's granule position is that of the last packet completed
// on it, -1 where none is.
// Every stream starts at granule position 0, so a1-encapsulation-ogg's rule for a stream that does not (the second audio
// packet flushes its page, so that the decoder learns the offset at once) never applies here.  A live stream starts at 0
// as well: it is the FILE that arrives in pieces, one walk interrupted at group boundaries (OggLive, below).
struct OggPage {
  int64_t file_off;  // where the page starts in its stream's file
  int64_t granule;
  int32_t run;       // 0: identification header; 1: comment + setup; 2: audio; -1: an unused slot of the page table
  int32_t first;     // the packet (of its run's list: headers 0..2, or the stream's audio packets) its first segment belongs to
  int32_t byte0;     // bytes of that packet on earlier pages (a multiple of 255; > 0: the page carries the continued flag)
  int32_t npackets;  // packets with a segment on the page
  int32_t nseg, body;
  int32_t seq, flags;
  int32_t stream, done;  // done: packets completed on the page
};

struct OggWalk {
  OggPage pg;       // the page being filled
  int64_t file_off; // where it starts
  int32_t seq, npages;
};

VAMD_OGG_FN void ogg_page_reset(OggWalk &w, int run) {
  w.pg.file_off = 0, w.pg.granule = -1;
  w.pg.run = run, w.pg.first = 0, w.pg.byte0 = 0, w.pg.npackets = 0, w.pg.nseg = 0, w.pg.body = 0, w.pg.seq = 0, w.pg.flags = 0;
  w.pg.done = 0;
}
VAMD_OGG_FN void ogg_walk_init(OggWalk &w, int stream) {
  w.file_off = 0, w.seq = 0, w.npages = 0;
  w.pg.stream = stream;
  ogg_page_reset(w, 0);
}
// the page is complete: into out[] (when it fits; npages counts on regardless), the next one begins empty
VAMD_OGG_FN void ogg_page_close(OggWalk &w, OggPage *out, int64_t cap, int extra_flags) {
  w.pg.file_off = w.file_off, w.pg.seq = w.seq, w.pg.flags |= extra_flags;
  if (w.npages < cap) out[w.npages] = w.pg;
  w.npages++, w.seq++;
  w.file_off += OGG_HEADER + w.pg.nseg + w.pg.body;
  ogg_page_reset(w, w.pg.run);
}
VAMD_OGG_FN void ogg_run_begin(OggWalk &w, int run, int bos) {
  ogg_page_reset(w, run);
  w.pg.flags = bos ? 0x02 : 0;
}
// packet k of the run: `bytes` long, granule position `granule`
VAMD_OGG_FN void ogg_walk_packet(OggWalk &w, OggPage *out, int64_t cap, int32_t k, int32_t bytes, int64_t granule) {
  const int32_t segs = ogg_segments(bytes);
  int32_t taken = 0;
  if (w.pg.nseg > 0 && w.pg.body > OGG_FILL && w.pg.done >= OGG_MIN_PACKETS) ogg_page_close(w, out, cap, 0);
  for (;;) {
    if (w.pg.nseg == OGG_MAX_SEGS) ogg_page_close(w, out, cap, 0);
    if (w.pg.npackets == 0) {
      w.pg.first = k, w.pg.byte0 = taken * 255;
      if (taken) w.pg.flags |= 0x01;
    }
    const int32_t room = OGG_MAX_SEGS - w.pg.nseg, take = segs - taken < room ? segs - taken : room;
    w.pg.body += ogg_piece_len(bytes, taken * 255, take);
    w.pg.nseg += take, w.pg.npackets++;
    taken += take;
    if (taken == segs) {
      w.pg.done++, w.pg.granule = granule;
      return;
    }
  }
}
// The same walk, up to 64 packets of a run at a time, a PAGE per step instead of a packet: with the chunk's sizes summed up
// in front of every packet (Bx[j], Sx[j]: bytes and segments of packets 0 .. j-1; n + 1 entries), what the page would hold
// if packets c .. j-1 joined it whole is a difference of two sums, so whether the walk stops in front of or inside packet j
// can be asked of every j at once -- a lane each on the device, the first lane that says yes found with one ballot
// (k_ogg_plan); the host asks them in turn (ogg_plan_stream).  c is the chunk's next packet, `taken` its segments already
// on earlier pages.
VAMD_OGG_FN void ogg_ahead(const OggPage &pg, const int32_t *Bx, const int32_t *Sx, int c, int taken, int j, int32_t *nseg, int32_t *body,
                           int32_t *done) {
  *nseg = pg.nseg + (Sx[j] - Sx[c]) - (j > c ? taken : 0);
  *body = pg.body + (Bx[j] - Bx[c]) - (j > c ? taken * 255 : 0);
  *done = pg.done + (j - c);
}
// 0: packet j joins the page whole; 1: the page is closed in front of it (4096 bytes and four packets); 2: it does not fit
// whole (the page is closed at 255 segments, inside the packet or in front of it)
VAMD_OGG_FN int ogg_stop_at(const OggPage &pg, const int32_t *Bx, const int32_t *Sx, const int32_t *bytes, int c, int taken, int j) {
  int32_t nseg, body, done;
  ogg_ahead(pg, Bx, Sx, c, taken, j, &nseg, &body, &done);
  if ((j > c || taken == 0) && nseg > 0 && body > OGG_FILL && done >= OGG_MIN_PACKETS) return 1;
  return nseg + ogg_segments(bytes[j]) - (j == c ? taken : 0) > OGG_MAX_SEGS ? 2 : 0;
}
// packets c .. j-1 join the page whole; then, by `why` (ogg_stop_at of packet j; 0 with j = n: the chunk is used up), the
// page is closed in front of packet j or filled up with its next segments and closed.  kbase: the chunk's first packet.
VAMD_OGG_FN void ogg_walk_join(OggWalk &w, OggPage *out, int64_t cap, int32_t kbase, const int32_t *Bx, const int32_t *Sx,
                               const int64_t *granule, int *c, int *taken, int j, int why) {
  if (j > *c) {
    int32_t nseg, body, done;
    ogg_ahead(w.pg, Bx, Sx, *c, *taken, j, &nseg, &body, &done);
    if (w.pg.npackets == 0) {
      w.pg.first = kbase + *c, w.pg.byte0 = *taken * 255;
      if (*taken) w.pg.flags |= 0x01;
    }
    w.pg.npackets += j - *c;
    w.pg.nseg = nseg, w.pg.body = body, w.pg.done = done, w.pg.granule = granule[j - 1];
    *c = j, *taken = 0;
  }
  if (why == 2) {
    const int32_t room = OGG_MAX_SEGS - w.pg.nseg;
    if (room > 0) {  // (fewer than the packet still has: none of them is its last, all are 255 long)
      if (w.pg.npackets == 0) {
        w.pg.first = kbase + *c, w.pg.byte0 = *taken * 255;
        if (*taken) w.pg.flags |= 0x01;
      }
      w.pg.npackets++, w.pg.nseg = OGG_MAX_SEGS, w.pg.body += room * 255;
      *taken += room;
    }
  }
  if (why) ogg_page_close(w, out, cap, 0);
}

// (eos = 0: the end of a header run -- and a live stream's FLUSH, ogg_flush below: the page is closed, the run goes on)
VAMD_OGG_FN void ogg_run_end(OggWalk &w, OggPage *out, int64_t cap, int eos) {
  if (w.pg.nseg > 0) ogg_page_close(w, out, cap, eos ? 0x04 : 0);
}
// the two header runs of a stream (header_bytes: identification, comment, setup)
VAMD_OGG_FN void ogg_walk_headers(OggWalk &w, OggPage *out, int64_t cap, const int32_t *header_bytes) {
  ogg_run_begin(w, 0, 1);
  ogg_walk_packet(w, out, cap, 0, header_bytes[0], 0);
  ogg_run_end(w, out, cap, 0);
  ogg_run_begin(w, 1, 0);
  ogg_walk_packet(w, out, cap, 1, header_bytes[1], 0);
  ogg_walk_packet(w, out, cap, 2, header_bytes[2], 0);
  ogg_run_end(w, out, cap, 0);
}
// the first 27 bytes of a page, checksum field zero
VAMD_OGG_FN void ogg_page_header(const OggPage &pg, uint32_t serial, uint8_t *h) {
  h[0] = 'O', h[1] = 'g', h[2] = 'g', h[3] = 'S', h[4] = 0, h[5] = (uint8_t)pg.flags;
  for (int i = 0; i < 8; i++) h[6 + i] = (uint8_t)((uint64_t)pg.granule >> (8 * i));
  for (int i = 0; i < 4; i++) h[14 + i] = (uint8_t)(serial >> (8 * i));
  for (int i = 0; i < 4; i++) h[18 + i] = (uint8_t)((uint32_t)pg.seq >> (8 * i));
  h[22] = h[23] = h[24] = h[25] = 0;
  h[26] = (uint8_t)pg.nseg;
}

// Page slots a stream needs at most, so that the page table can be laid out before any size is known: `header_slots`
// for the two header runs (1 + one page per 255 segments of comment + setup, rounded up), and per audio packet
// ogg_slots_per_packet(cap) slots, cap the longest packet the setup can make -- every audio page but the run's last either
// completes four packets or holds 255 segments, and a stream of n packets of at most cap bytes has at most
// n (1 + cap / 255) segments: n / 4 + n (1 + cap / 255) / 255 pages, and the run's last (among the header slots' + 2).
VAMD_OGG_FN int64_t ogg_slots_per_packet(int64_t packet_cap) { return 2 + (1 + packet_cap / 255) / 255; }
VAMD_OGG_FN int64_t ogg_header_slots(const int32_t *header_bytes) {
  return 1 + (ogg_segments(header_bytes[1]) + ogg_segments(header_bytes[2]) + 254) / 255 + 2;
}
// ... and the bytes the files of a group take at most, from its packets' bytes (each rounded up to 4 or not), their number
// and the streams': every page but a run's last holds more than OGG_FILL body bytes or 255 segments.
VAMD_OGG_FN int64_t ogg_file_bound(int64_t packet_bytes, int64_t npackets, int64_t nstreams, const int32_t *header_bytes) {
  const int64_t pages = packet_bytes / (OGG_FILL + 1) + (npackets + packet_bytes / 255) / 255 + nstreams * (2 + ogg_header_slots(header_bytes));
  return packet_bytes + nstreams * ((int64_t)header_bytes[0] + header_bytes[1] + header_bytes[2]) + pages * (OGG_HEADER + OGG_MAX_SEGS);
}

// A group whose streams carry comment headers of their own (vamd_feed_ogg_comments): the header slots are
// ogg_header_slots of the group's LONGEST comment (header_bytes[1] set to it), the bytes come from the SUM of the
// comments -- stream s's header runs take 1 + ceil((segments of its comment + of the setup header) / 255) pages, and a
// comment of c bytes is c / 255 + 1 segments, so all of them together take at most
// 2 nstreams + (comment_sum / 255 + nstreams (1 + segments of the setup header)) / 255 pages.
VAMD_OGG_FN int64_t ogg_file_bound_v(int64_t packet_bytes, int64_t npackets, int64_t nstreams, const int32_t *header_bytes, int64_t comment_sum) {
  const int64_t pages = packet_bytes / (OGG_FILL + 1) + (npackets + packet_bytes / 255) / 255 + nstreams * 4 +
                        (comment_sum / 255 + nstreams * (1 + ogg_segments(header_bytes[2]))) / 255 + 1;
  return packet_bytes + nstreams * ((int64_t)header_bytes[0] + header_bytes[2]) + comment_sum + pages * (OGG_HEADER + OGG_MAX_SEGS);
}

// A Vorbis comment header as far as its framing goes (Vorbis I 5.2.1; what the reference's vorbis_synthesis_headerin
// asks of one): type 3 and "vorbis", a little-endian vendor length and that many bytes, a comment count, that many
// length + bytes pairs, then a byte with bit 0 set -- every one of them inside the packet.  What lies behind the framing
// byte is not looked at (taggers pad there), nor are the strings.  0: well-formed; else what is wrong (ogg_comment_why).
enum { OGG_COMMENT_OK = 0, OGG_COMMENT_LENGTH, OGG_COMMENT_TYPE, OGG_COMMENT_VENDOR, OGG_COMMENT_COUNT, OGG_COMMENT_ENTRY, OGG_COMMENT_FRAMING };
VAMD_OGG_FN uint32_t ogg_le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }
VAMD_OGG_FN int ogg_comment_check(const uint8_t *p, int64_t n) {
  if (!p || n < 7 || n > ((int64_t)1 << 24)) return OGG_COMMENT_LENGTH;
  if (p[0] != 3 || p[1] != 'v' || p[2] != 'o' || p[3] != 'r' || p[4] != 'b' || p[5] != 'i' || p[6] != 's') return OGG_COMMENT_TYPE;
  int64_t at = 7;
  if (n - at < 4 || (int64_t)ogg_le32(p + at) > n - at - 4) return OGG_COMMENT_VENDOR;
  at += 4 + (int64_t)ogg_le32(p + at);
  if (n - at < 4) return OGG_COMMENT_COUNT;
  const int64_t count = (int64_t)ogg_le32(p + at);
  at += 4;
  if (count > (n - at) / 4) return OGG_COMMENT_COUNT;  // (every comment takes four bytes at least)
  for (int64_t i = 0; i < count; i++) {
    if (n - at < 4 || (int64_t)ogg_le32(p + at) > n - at - 4) return OGG_COMMENT_ENTRY;
    at += 4 + (int64_t)ogg_le32(p + at);
  }
  return at < n && (p[at] & 1) ? OGG_COMMENT_OK : OGG_COMMENT_FRAMING;
}
VAMD_OGG_FN const char *ogg_comment_why(int code) {
  switch (code) {
    case OGG_COMMENT_OK: return "well-formed";
    case OGG_COMMENT_LENGTH: return "its length is not 7 to 2^24 bytes";
    case OGG_COMMENT_TYPE: return "it does not begin with packet type 3 and \"vorbis\"";
    case OGG_COMMENT_VENDOR: return "the vendor string runs past its end";
    case OGG_COMMENT_COUNT: return "the comment count is not inside it, or counts more comments than it can hold";
    case OGG_COMMENT_ENTRY: return "a comment's length or bytes run past its end";
    default: return "the framing bit behind the last comment is missing or clear";
  }
}

// ---- a live feed: one walk per stream, interrupted at group boundaries ----
// At the end of a group every packet has been taken completely, so the walk's state is its OggWalk: the open page, the
// next sequence number and file_off, which stays absolute in the stream's file (the group's byte range starts at the
// file_off the group began with).  The packets with a segment on the open page are carried: the next group's list is the
// carried packets, then its own, and the open page's `first` is rebased to 0.  Of a continued first packet only the part
// from byte0 on is carried -- byte0 is a multiple of 255, so the remainder laces exactly as a packet of its own (byte0
// becomes 0; the continued flag stays in pg.flags).
struct OggLive {
  OggWalk w;
  uint32_t serial;
  int32_t started;  // the stream is open: its headers are out
  int32_t dead;     // != 0: the VAMD_STATUS_* of the block that had no packet; no page until the stream is closed (0x80: the state is unusable)
  int32_t ncarry;   // carried packets
};
// a stream in a group: it starts / ends with it / is not there / is flushed behind it (vamd_feed_ogg_flush)
enum { OGG_LIVE_BEGIN = 1, OGG_LIVE_CLOSE = 2, OGG_LIVE_ABSENT = 4, OGG_LIVE_FLUSH = 8 };
// the open page of a group's end, rebased onto the next group's list
VAMD_OGG_FN void ogg_walk_rebase(OggWalk &w) { w.pg.first = 0, w.pg.byte0 = 0, w.npages = 0; }
// A FLUSH (a group's end, behind its last packet; the stream goes on): the open page, if it holds a segment, is closed as
// the end of the run closes it, without the end-of-stream flag, and the run goes on -- the next packet starts a fresh page
// with the next sequence number.  Every packet on the page is complete there, so its granule position is the last one's,
// never -1, and its last lacing value is below 255.  Nothing lies on the open page afterwards: the carry is empty.  A
// close in the same group wins (the page ends the run, with its flag), and an empty open page hands out nothing.
// The case a feed never meets -- a close with no new packet onto an EMPTY open page, which a flush in the group before
// makes possible for this walk's callers: ogg_run_end writes no page there, so the file ends on the flushed page without
// an end-of-stream flag (no empty page is invented; RFC 3533 allows one, the policy above does not name one).  The feed
// cannot get there: a closing piece always yields the e_o_s packet, so its closing group always has a new packet.
VAMD_OGG_FN void ogg_flush(OggWalk &w, OggPage *out, int64_t cap) { ogg_run_end(w, out, cap, 0); }
// Page slots per stream of a live group: the header slots, one for the carried page, and ogg_slots_per_packet per NEW
// packet (every other page holds new packets only).  The count, flushes included -- a group's pages of stream s, n new
// packets of at most cap bytes: where the stream begins, at most ogg_header_slots - 2 header pages; the carried page (one slot: it is the only page with carried packets
// on it, flushed or not, since a flush leaves no carry); pages of new packets alone that are closed by the fill rule or at
// 255 segments, at most n / 4 + n (1 + cap / 255) / 255 <= n ogg_slots_per_packet(cap) of them; and ONE page that is
// neither -- the run's last (a close) or the flushed one, never both, since a close wins.  That one is among the two
// spare slots of ogg_header_slots, as the run's last always was: a flush adds no page that the close did not already
// have a slot for.  With n = 0 (a flushed 0-frame piece, a list of one-byte packets flushed one per group) the carried
// page's slot is the flushed page's.  So a flush needs no slot more, and the page table is the size it was without it.
VAMD_OGG_FN int64_t ogg_live_slots(const int32_t *header_bytes) { return ogg_header_slots(header_bytes) + 1; }
// The bytes a live group's pages take at most: ogg_file_bound of the new packets and every stream's full carry, and the
// carried page's header and lacing.  It holds with flushes as well: ogg_file_bound counts per page a full header and lacing table (282 bytes), and
// its pages are: those with more than OGG_FILL body bytes, those with 255 segments, and per stream 2 + ogg_header_slots,
// of which the header runs use ogg_header_slots - 2 at most -- four pages per stream and group that are neither full nor
// header pages.  A whole stream uses one of them (the run's last); a live group the same one for its close OR its
// flush, and the carried page has a header of its own on top (the last term).  The flushed page's body is packet bytes
// that are counted in any case (new ones, or the carry's).  ogg_live_file_bound_v: ogg_file_bound_v counts 4 pages per
// stream and the comments' segments / 255, of which the header runs use 2 per stream and that quotient -- two spare per
// stream, one of them the run's last or the flushed page.  So the pinned arena does not grow with a flush.
VAMD_OGG_FN int64_t ogg_live_file_bound(int64_t packet_bytes, int64_t npackets, int64_t nstreams, const int32_t *header_bytes) {
  return ogg_file_bound(packet_bytes + nstreams * OGG_CARRY_BODY, npackets + nstreams * OGG_MAX_SEGS, nstreams, header_bytes) +
         nstreams * (OGG_HEADER + OGG_MAX_SEGS);
}
// The same with comment headers per stream (ogg_file_bound_v; the slots: ogg_live_slots of the group's longest comment)
VAMD_OGG_FN int64_t ogg_live_file_bound_v(int64_t packet_bytes, int64_t npackets, int64_t nstreams, const int32_t *header_bytes,
                                          int64_t comment_sum) {
  return ogg_file_bound_v(packet_bytes + nstreams * OGG_CARRY_BODY, npackets + nstreams * OGG_MAX_SEGS, nstreams, header_bytes, comment_sum) +
         nstreams * (OGG_HEADER + OGG_MAX_SEGS);
}

// (VAMD_OGG_NO_FEED_KERNELS: a translation unit that wants the functions above and not the feed's kernels -- they are
// vamd_feed.hip's, and a second copy of their names would not link)
#if defined(__HIPCC__) && !defined(VAMD_OGG_NO_FEED_KERNELS)
// ---- the kernels ----
// What the pager reads: the device mirror of the group's packets (bytes at the offsets of the output arena, each packet at
// a multiple of 4, and their records), the three header packets, the streams' serial numbers, and, where the group names
// them, the streams' own comment headers.
struct OggIn {
  const int64_t *stream_start;  // [nstreams + 1] into the packets
  const int64_t *off, *gp;      // [packets] where a packet's bytes lie in `bytes`; its granule position
  const int32_t *bits;          // [packets] -1: no packet
  const uint8_t *info;          // [packets] (vamd_feed_result.info)
  const uint8_t *bytes;
  int64_t cap;                  // bytes of the mirror that hold packets (8 more are readable behind them)
  const int64_t *packet_total;  // null, or the bytes the group's packets take: beyond cap, nothing was mirrored
  const uint8_t *hdr;           // the header packets, each at a multiple of 4
  int32_t hdr_off[3], hdr_bytes[3];
  const uint32_t *serial;       // [nstreams]
  int64_t header_slots, slots_per_packet;
  // The group's comment headers per stream (vamd_feed_ogg_comments); null: none, header packet 1 is hdr's for all.  One
  // buffer, one pointer: [where stream s's lies in it (nstreams, 8 bytes each) | its length (nstreams, 4 each; negative:
  // the shared one) | the comments, each at a multiple of 4, 8 readable bytes behind the last]
  const uint8_t *cmt;
};
__device__ __forceinline__ int64_t ogg_slot_base(const OggIn &I, long s) { return s * I.header_slots + I.slots_per_packet * I.stream_start[s]; }
// the length of stream s's comment header: its own where the group has a table and the entry is set, else the shared one's
__device__ __forceinline__ int32_t ogg_comment_own(const OggIn &I, long nstreams, long s) {  // (I.cmt set) its length, or negative
  return ((const int32_t *)(I.cmt + nstreams * 8))[s];
}
__device__ __forceinline__ int32_t ogg_comment_bytes(const OggIn &I, long nstreams, long s) {
  if (I.cmt) {
    const int32_t n = ogg_comment_own(I, nstreams, s);
    if (n >= 0) return n;
  }
  return I.hdr_bytes[1];
}

// A live group (in == null: whole streams): per stream its state and carry as the last group left them, and where this
// group's go -- the other of two buffers each, swapped by the host once the group has succeeded, so that a group laid out
// twice advances its streams once.  A stream's carry: rec [2 * OGG_MAX_SEGS] (the packets' bytes, then where each lies in
// its OGG_CARRY_BYTES of `bytes`, a multiple of 4).  flags: OGG_LIVE_*; gstart: the file_off a stream's group began with
// (k_ogg_plan -> k_ogg_pages).  OggIn's header_slots are ogg_live_slots, serial[] names the streams that begin.
struct OggLiveIO {
  const OggLive *in;
  OggLive *out;
  const int32_t *rec_in;
  const uint8_t *bytes_in;
  int32_t *rec_out;
  uint8_t *bytes_out;
  const uint32_t *flags;
  int64_t *gstart;
};
__device__ __forceinline__ int ogg_live_ncarry(const OggLiveIO &V, long s) {  // packets in front of the group's own in stream s's list
  if (!V.in || (V.flags[s] & (OGG_LIVE_BEGIN | OGG_LIVE_ABSENT))) return 0;
  const int n = V.in[s].ncarry;
  return n < 0 || n > OGG_MAX_SEGS ? 0 : n;
}

// a wave per stream: its pages into its slots of the page table, the unused slots marked; file_bytes, npages, status.
// 64 packets at a time: one coalesced load of their sizes and granule positions, a wave-wide scan of bytes and segments
// into LDS, then a step per PAGE (ogg_stop_at in every lane, one ballot, ogg_walk_join) -- the walk is serial in pages
// only, and never touches memory.  A stream in which a block has no packet gets no page at all.
// A group with comment headers per stream (I.cmt set): the header runs are walked with the stream's own length of
// header packet 1; nothing else of the walk knows.
// A live group (V.in set): a stream that begins walks the headers and begins the audio run; an open one loads its walk --
// the open page already counts the carried packets, which come first in the group's list -- and walks the new packets;
// only a closing one ends the run; a flushed one (OGG_LIVE_FLUSH, and no close) closes its open page behind the last
// packet and goes on (ogg_flush): one more page in its slots, an empty open page in the state.  file_bytes is what the
// group adds to the file.  A stream that lost a packet writes no page from that group on and reports the block's status
// until it is closed; it, an absent one and one that has not begun are not flushed either.  The state behind the group
// goes to V.out (ncarry and the rebase are k_ogg_carry's).
__global__ __launch_bounds__(64) void k_ogg_plan(OggIn I, long nstreams, OggPage *__restrict__ pages, int64_t *__restrict__ file_bytes,
                                                 int32_t *__restrict__ npages, uint8_t *__restrict__ status, OggLiveIO V) {
  __shared__ int32_t sz[64], Bx[65], Sx[65];
  __shared__ int64_t gr[64];
  const long s = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t k0 = I.stream_start[s], k1 = I.stream_start[s + 1];
  const int64_t cap = I.header_slots + I.slots_per_packet * (k1 - k0);
  OggPage *out = pages + ogg_slot_base(I, s);
  unsigned st = 0;
  for (int64_t base = k0; base < k1 && !st; base += 64) {
    const int64_t k = base + lane;
    unsigned mine = 0;
    if (k < k1 && I.bits[k] < 0) mine = ((I.info[k] >> 2) & 3u) ? ((I.info[k] >> 2) & 3u) : 3u;
    const unsigned long long m = __ballot(mine != 0);
    if (m) st = (unsigned)__shfl((int)mine, __ffsll((long long)m) - 1, 64);
  }
  // every lane keeps the walk's state (it is the same in all of them); lane 0 alone writes pages
  const int64_t wcap = lane == 0 ? cap : 0;
  OggWalk w;
  ogg_walk_init(w, (int)s);
  const unsigned lf = V.in ? V.flags[s] : (unsigned)(OGG_LIVE_BEGIN | OGG_LIVE_CLOSE);
  const bool begin = lf & OGG_LIVE_BEGIN, absent = !begin && (lf & OGG_LIVE_ABSENT);
  uint32_t serial = I.serial[s];
  int ncarry = 0;
  if (V.in && !begin && !absent) {
    const OggLive old = V.in[s];
    w = old.w, w.npages = 0, w.pg.stream = (int32_t)s;
    serial = old.serial, ncarry = ogg_live_ncarry(V, s);
    if (!old.started) st = 0x80u;  // (an open stream without a state)
    if (old.dead) st = (unsigned)old.dead;
  }
  const int64_t gstart = w.file_off;
  const bool none = st || absent || (I.packet_total && *I.packet_total > I.cap);
  if (!none) {
    if (begin) {  // (header packet 1 is the stream's own comment where the group names one)
      const int32_t hb[3] = {I.hdr_bytes[0], ogg_comment_bytes(I, nstreams, s), I.hdr_bytes[2]};
      ogg_walk_headers(w, out, wcap, hb);
      ogg_run_begin(w, 2, 0);
    }
    for (int64_t base = k0; base < k1; base += 64) {
      const int64_t k = base + lane;
      const int n = k1 - base < 64 ? (int)(k1 - base) : 64;
      const int32_t bytes = k < k1 ? (I.bits[k] + 7) >> 3 : 0, segs = k < k1 ? ogg_segments(bytes) : 0;
      int ib = bytes, is = segs;  // inclusive scans over the wave
      for (int d = 1; d < 64; d <<= 1) {
        const int ub = __shfl_up(ib, d, 64), us = __shfl_up(is, d, 64);
        if (lane >= d) ib += ub, is += us;
      }
      __syncthreads();
      sz[lane] = bytes, gr[lane] = k < k1 ? I.gp[k] : 0;
      Bx[lane + 1] = ib, Sx[lane + 1] = is;
      if (lane == 0) Bx[0] = 0, Sx[0] = 0;
      __syncthreads();
      int c = 0, taken = 0;
      while (c < n) {
        const int why = lane >= c && lane < n ? ogg_stop_at(w.pg, Bx, Sx, sz, c, taken, lane) : 0;
        const unsigned long long m = __ballot(why != 0);
        const int j = m ? __ffsll((long long)m) - 1 : n;
        ogg_walk_join(w, out, wcap, ncarry + (int32_t)(base - k0), Bx, Sx, gr, &c, &taken, j, m ? __shfl(why, j, 64) : 0);
      }
    }
    if (lf & OGG_LIVE_CLOSE) ogg_run_end(w, out, wcap, 1);
    else if (lf & OGG_LIVE_FLUSH) ogg_flush(w, out, wcap);
  }
  int np = __shfl(w.npages, 0, 64);
  if (np > cap) np = 0, st |= 0x80u;  // (the slot bound did not hold: no file rather than a cut one)
  for (int64_t i = np + lane; i < cap; i += 64) out[i].run = -1;
  if (lane == 0) {
    file_bytes[s] = (none || (st & 0x80u)) ? 0 : w.file_off - gstart;
    npages[s] = (none || (st & 0x80u)) ? 0 : np;
    status[s] = (uint8_t)st;
    if (V.in) {
      const bool open = !absent && !(lf & OGG_LIVE_CLOSE);
      OggLive nx;
      nx.w = w, nx.serial = serial, nx.started = open, nx.dead = open ? (int32_t)st : 0, nx.ncarry = 0;
      V.out[s] = nx;
      V.gstart[s] = gstart;
    }
  }
}

// where the pages go: the pinned arena and the group's record beside it (host memory, mapped)
struct OggOut {
  int64_t *total, *stream_offset;  // [1], [nstreams + 1]
  int32_t *npages;                 // [nstreams]
  uint8_t *status;                 // [nstreams]
  uint8_t *bytes;
  int64_t cap;
};

// A wave per page slot.  The page is a virtual byte string V: header (27 bytes), lacing table, then the pieces of the
// packets on it, each piece a run of bytes of the mirror.  LDS holds header + lacing, the pieces' places in V and in the
// mirror, and the CRC table.
//   CRC: lane l sums its chunk of V byte by byte (ogg_crc_range), the tree joins the 64 sums in six steps.
//   Stores: the arena is host memory across the link, so only whole aligned dwords are written, consecutive lanes to
//   consecutive dwords.  A page starts wherever the one before ends; the dword that holds a page's last bytes belongs to
//   that page's wave, which fills it up with the bytes that follow -- always the next page's capture pattern "OggS" (or
//   nothing anyone reads, behind the arena's last page).  So no byte is written twice and no dword in parts.  A dword
//   inside one piece is two aligned words of the mirror joined by v_alignbyte; one that straddles pieces (packets of a
//   few bytes), the header or the page's end is put together byte by byte.
// A group with comment headers per stream (I.cmt set): header packet 1 of a stream with an entry lies in I.cmt, not
// in I.hdr -- the pieces' source and length change, lacing, CRC and stores do not.
// A live group (V.in set): a page's packets come from two sources -- the first ncarry of the stream's list lie in its
// carry, the others in the mirror -- the serial number is the stream's own, and the page goes where the group's range has it.
// A flushed page is a page like any other here: its packets are pg.first .. pg.first + npackets - 1 of the stream's list,
// whether all of them lie in the carry (a 0-frame piece: first = 0, npackets = ncarry, k never reaches the mirror), in
// the carry and then the mirror (the per-packet choice below), or it begins inside a packet of this group (byte0 > 0:
// the first piece starts byte0 into its packet, as on every continued page; a continued page that was CARRIED has
// byte0 = 0 and the flag 0x01 in pg.flags, its first packet being the carried rest).
__global__ __launch_bounds__(64) void k_ogg_pages(OggIn I, long nstreams, const OggPage *__restrict__ pages,
                                                  const int64_t *__restrict__ stream_off, const int32_t *__restrict__ npages,
                                                  const uint8_t *__restrict__ status, OggOut O, OggLiveIO V) {
  __shared__ uint32_t table[256];
  __shared__ __attribute__((aligned(8))) uint8_t head[OGG_HEADER + OGG_MAX_SEGS + 6];
  __shared__ int32_t pdst[OGG_MAX_SEGS + 1];
  __shared__ const uint8_t *psrc[OGG_MAX_SEGS];
  const int lane = threadIdx.x;
  {  // the group's record (the first (nstreams + 1 + 63) / 64 blocks; there are at least nstreams slots)
    const long t = (long)blockIdx.x * 64 + lane;
    if (t <= nstreams) O.stream_offset[t] = stream_off[t];
    if (t < nstreams) O.npages[t] = npages[t], O.status[t] = status[t];
    if (t == 0) *O.total = stream_off[nstreams];
  }
  const OggPage pg = pages[blockIdx.x];
  if (pg.run < 0 || pg.nseg < 1 || pg.nseg > OGG_MAX_SEGS || pg.npackets < 1 || pg.npackets > pg.nseg) return;
  const long s = pg.stream;
  for (int e = lane; e < 256; e += 64) table[e] = ogg_crc_entry((uint32_t)e);
  // the pieces and the lacing table
  const int ncarry = ogg_live_ncarry(V, s);
  const int64_t kbase = I.stream_start[s] + pg.first - ncarry, kend = I.stream_start[s + 1];
  int carry_s = 0, carry_b = 0;
  bool bad = false;
  int32_t own_bytes = -1;  // the stream's own comment header, where the group names one: the same for the whole wave
  const uint8_t *own_src = nullptr;
  if (pg.run == 1 && I.cmt) {
    own_bytes = ogg_comment_own(I, nstreams, s);
    own_src = I.cmt + ((const int64_t *)I.cmt)[s];
  }
  for (int j0 = 0; j0 < pg.npackets; j0 += 64) {
    const int j = j0 + lane;
    const bool valid = j < pg.npackets;
    int32_t bytes = 0;
    const uint8_t *src = I.bytes;
    if (valid) {
      if (pg.run == 2 && pg.first < 0) bad = true;
      else if (pg.run == 2 && pg.first + j < ncarry) {
        const int32_t *rec = V.rec_in + s * (2 * OGG_MAX_SEGS);
        const int32_t o = rec[OGG_MAX_SEGS + pg.first + j];
        bytes = rec[pg.first + j];
        if (bytes < 0 || o < 0 || o + bytes > OGG_CARRY_BYTES - 18) bad = true, bytes = 0;
        else src = V.bytes_in + s * OGG_CARRY_BYTES + o;
      } else if (pg.run == 2) {
        const int64_t k = kbase + j;
        if (k < I.stream_start[s] || k >= kend) bad = true;
        else {
          const int64_t o = I.off[k];
          bytes = (I.bits[k] + 7) >> 3;
          if (bytes < 0 || o < 0 || o + bytes > I.cap) bad = true, bytes = 0;
          else src = I.bytes + o;
        }
      } else {
        const int h = pg.first + j;
        if (h > 2) bad = true;
        else {
          bytes = I.hdr_bytes[h], src = I.hdr + I.hdr_off[h];
          if (h == 1 && own_bytes >= 0) bytes = own_bytes, src = own_src;  // (a packet like any other, continued over pages)
        }
      }
    }
    const int32_t start = j == 0 ? pg.byte0 : 0;
    const int32_t left = valid && start <= bytes ? ogg_segments(bytes) - start / 255 : 0;
    int incl = left;
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    const int before = carry_s + incl - left;
    int32_t take = pg.nseg - before < left ? pg.nseg - before : left;
    if (take < 0) take = 0;
    const int32_t len = valid && take > 0 ? ogg_piece_len(bytes, start, take) : 0;
    int incb = len;
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incb, d, 64);
      if (lane >= d) incb += up;
    }
    if (valid) {
      pdst[j] = carry_b + incb - len;
      psrc[j] = src + start;
      for (int q = 0; q < take; q++) head[OGG_HEADER + before + q] = (uint8_t)ogg_lace_value(bytes, start / 255 + q);
    }
    carry_s += __shfl(incl, 63, 64);
    carry_b += __shfl(incb, 63, 64);
  }
  if (carry_b != pg.body || carry_s < pg.nseg) bad = true;  // (the mirror and the page table disagree: nothing is written)
  if (__ballot(bad)) return;
  if (lane == 0) {
    pdst[pg.npackets] = pg.body;
    ogg_page_header(pg, V.in && !(V.flags[s] & OGG_LIVE_BEGIN) ? V.in[s].serial : I.serial[s], head);
  }
  __syncthreads();
  const int hlen = OGG_HEADER + pg.nseg, len = hlen + pg.body;
  auto piece_of = [&](int b) {  // the piece that holds body byte b: the last one that starts at or before it
    int lo = 0, hi = pg.npackets;
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (pdst[mid] <= b) lo = mid;
      else hi = mid;
    }
    return lo;
  };
  // CRC
  {
    const int64_t c = ogg_crc_chunk(len, OGG_CRC_LANES, OGG_CRC_MIN_CHUNK);
    int64_t lo, hi;
    ogg_crc_range(len, OGG_CRC_LANES, c, lane, &lo, &hi);
    uint32_t crc = 0;
    int v = (int)lo;
    for (; v < hi && v < hlen; v++) crc = ogg_crc_byte(table, crc, head[v]);
    if (v < hi) {
      int i = piece_of(v - hlen);
      for (; v < hi; v++) {
        const int b = v - hlen;
        while (b >= pdst[i + 1]) i++;
        crc = ogg_crc_byte(table, crc, psrc[i][b - pdst[i]]);
      }
    }
    uint32_t m = ogg_crc_xpow8(c);
    for (int d = 1; d < OGG_CRC_LANES; d <<= 1) {
      const uint32_t right = (uint32_t)__shfl_down((int)crc, d, 64);
      crc = ogg_crc_join(crc, right, m);
      m = ogg_crc_mul(m, m);
    }
    __syncthreads();
    if (lane == 0)
      for (int i = 0; i < 4; i++) head[22 + i] = (uint8_t)(crc >> (8 * i));
    __syncthreads();
  }
  // stores
  const int64_t g0 = stream_off[s] + pg.file_off - (V.in ? V.gstart[s] : 0), g1 = g0 + len;
  const int64_t a0 = (g0 + 3) & ~(int64_t)3, a1 = (g1 + 3) & ~(int64_t)3;
  if (a1 > O.cap) return;
  for (int64_t a = a0 + 4 * lane; a < a1; a += 256) {
    const int v = (int)(a - g0);
    uint32_t word = 0;
    bool whole = false;
    if (v >= hlen && v + 4 <= len) {
      const int b = v - hlen, i = piece_of(b);
      if (b + 4 <= pdst[i + 1]) {
        const uint8_t *p = psrc[i] + (b - pdst[i]);
        const uint32_t *wp = (const uint32_t *)((uintptr_t)p & ~(uintptr_t)3);
        const unsigned sh = (unsigned)((uintptr_t)p & 3);
        const uint32_t w0 = wp[0], w1 = sh ? wp[1] : 0u;
        word = __builtin_amdgcn_alignbyte(w1, w0, sh);
        whole = true;
      }
    }
    if (!whole) {
      for (int t = 0; t < 4; t++) {
        const int u = v + t;
        uint32_t x;
        if (u < hlen) x = head[u];
        else if (u >= len) x = (uint32_t)"OggS"[(u - len) & 3];
        else {
          const int b = u - hlen, i = piece_of(b);
          x = psrc[i][b - pdst[i]];
        }
        word |= x << (8 * t);
      }
    }
    *(uint32_t *)(O.bytes + a) = word;
  }
}

// A live group, behind k_ogg_pages (which has read the old carry by then), a wave per stream: what lies on the page still
// open -- of each of its packets the bytes and where they go, of a continued first packet the part from byte0 on -- out
// of the old carry and the mirror into the other carry; then the rebase and ncarry into the state k_ogg_plan left in V.out.
// A list that contradicts the page (never seen) costs the stream its state: status 0x80 from the next group on.
// Behind a flush the open page is empty (np = 0): bad0 is false, no loop runs, body = pg.body = 0, nothing is copied, and
// the state stays alive with ncarry = 0.
__global__ __launch_bounds__(64) void k_ogg_carry(OggIn I, long nstreams, OggLiveIO V) {
  __shared__ int32_t cb[OGG_MAX_SEGS], co[OGG_MAX_SEGS];
  __shared__ const uint8_t *cs[OGG_MAX_SEGS];
  const long s = blockIdx.x;
  const int lane = threadIdx.x;
  if (s >= nstreams || (I.packet_total && *I.packet_total > I.cap)) return;
  const OggLive nx = V.out[s];
  if (!nx.started || nx.dead) return;  // (ncarry is 0)
  const OggPage pg = nx.w.pg;
  const int ncarry = ogg_live_ncarry(V, s);
  const int64_t k0 = I.stream_start[s], k1 = I.stream_start[s + 1];
  const int np = pg.npackets;
  // (the same in every lane: with it false, every index below is inside its list)
  const bool bad0 = np < 0 || np > OGG_MAX_SEGS || pg.first < 0 || (np > 0 && pg.first + np != ncarry + (k1 - k0));
  bool bad = bad0;
  int at = 0, body = 0;
  for (int j0 = 0; j0 < np && !bad0; j0 += 64) {
    const int j = j0 + lane, v = pg.first + j;
    int32_t bytes = 0;
    const uint8_t *src = I.bytes;
    if (j < np) {
      if (v < ncarry) {
        const int32_t *rec = V.rec_in + s * (2 * OGG_MAX_SEGS);
        const int32_t o = rec[OGG_MAX_SEGS + v];
        bytes = rec[v];
        if (bytes < 0 || o < 0 || o + bytes > OGG_CARRY_BYTES - 18) bad = true, bytes = 0;
        else src = V.bytes_in + s * OGG_CARRY_BYTES + o;
      } else {
        const int64_t k = k0 + (v - ncarry), o = I.off[k];
        bytes = (I.bits[k] + 7) >> 3;
        if (bytes < 0 || o < 0 || o + bytes > I.cap) bad = true, bytes = 0;
        else src = I.bytes + o;
      }
      if (j == 0) {
        if (pg.byte0 < 0 || pg.byte0 > bytes) bad = true;
        else src += pg.byte0, bytes -= pg.byte0;
      }
    }
    const int room = (bytes + 3) & ~3;
    int incl = room, incb = bytes;
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64), ub = __shfl_up(incb, d, 64);
      if (lane >= d) incl += up, incb += ub;
    }
    if (j < np) cb[j] = bytes, co[j] = at + incl - room, cs[j] = src;
    at += __shfl(incl, 63, 64), body += __shfl(incb, 63, 64);
  }
  if (body != pg.body || at > OGG_CARRY_BYTES - 18) bad = true;
  bad = __ballot(bad) != 0;
  __syncthreads();
  int32_t *rec = V.rec_out + s * (2 * OGG_MAX_SEGS);
  uint32_t *dst = (uint32_t *)(V.bytes_out + s * OGG_CARRY_BYTES);
  if (!bad) {
    for (int j = lane; j < np; j += 64) rec[j] = cb[j], rec[OGG_MAX_SEGS + j] = co[j];
    for (int j = 0; j < np; j++) {  // whole words: a source word is two aligned words of the mirror (or the carry) joined
      const uintptr_t p = (uintptr_t)cs[j];
      const unsigned sh = (unsigned)(p & 3);
      const uint32_t *wp = (const uint32_t *)(p & ~(uintptr_t)3);
      for (int wd = lane; wd < (cb[j] + 3) >> 2; wd += 64) {
        const uint32_t w0 = wp[wd], w1 = sh ? wp[wd + 1] : 0u;
        dst[(co[j] >> 2) + wd] = __builtin_amdgcn_alignbyte(w1, w0, sh);
      }
    }
  }
  if (lane == 0) {
    OggLive *o = V.out + s;
    ogg_walk_rebase(o->w);
    o->ncarry = bad ? 0 : np;
    if (bad) o->dead = 0x80;
  }
}
#endif  // __HIPCC__ && !VAMD_OGG_NO_FEED_KERNELS

#if !defined(__HIP_DEVICE_COMPILE__)
// ---- host only: the chunked CRC as k_ogg_pages computes it, and the mux (the CPU suite; the GPU's files are held
// against the mux byte for byte) ----
inline uint32_t ogg_crc_chunked(const uint8_t *data, int64_t n, int min_chunk, int lanes) {
  uint32_t table[256], part[64], next[64];
  for (int e = 0; e < 256; e++) table[e] = ogg_crc_entry((uint32_t)e);
  if (lanes > 64) lanes = 64;
  const int64_t c = ogg_crc_chunk(n, lanes, min_chunk);
  for (int l = 0; l < lanes; l++) {
    int64_t lo, hi;
    ogg_crc_range(n, lanes, c, l, &lo, &hi);
    uint32_t crc = 0;
    for (int64_t v = lo; v < hi; v++) crc = ogg_crc_byte(table, crc, data[v]);
    part[l] = crc;
  }
  uint32_t m = ogg_crc_xpow8(c);
  for (int d = 1; d < lanes; d <<= 1) {
    for (int l = 0; l < lanes; l++) next[l] = ogg_crc_join(part[l], l + d < lanes ? part[l + d] : part[l], m);
    memcpy(part, next, sizeof(part));
    m = ogg_crc_mul(m, m);
  }
  return part[0];
}

// npackets more packets of the audio run, as k_ogg_plan takes them: 64 at a time, a page per step.  first: the place of
// packet 0 in the list that the pages' `first` counts in.
inline void ogg_walk_audio(OggWalk &w, OggPage *pages, int64_t cap, int32_t first, int64_t npackets, const int32_t *bytes,
                           const int64_t *granule) {
  for (int64_t base = 0; base < npackets; base += 64) {
    const int n = npackets - base < 64 ? (int)(npackets - base) : 64;
    int32_t Bx[65], Sx[65];
    Bx[0] = Sx[0] = 0;
    for (int j = 0; j < n; j++) Bx[j + 1] = Bx[j] + bytes[base + j], Sx[j + 1] = Sx[j] + ogg_segments(bytes[base + j]);
    int c = 0, taken = 0;
    while (c < n) {
      int j = c, why = 0;
      for (; j < n; j++)
        if ((why = ogg_stop_at(w.pg, Bx, Sx, bytes + base, c, taken, j)) != 0) break;
      ogg_walk_join(w, pages, cap, first + (int32_t)base, Bx, Sx, granule + base, &c, &taken, j, why);
    }
  }
}

// a stream's pages from its packet sizes: pages[] (up to cap of them) <- the walk; returns their number, *file_bytes the file's
inline int64_t ogg_plan_stream(const int32_t *header_bytes, int64_t npackets, const int32_t *bytes, const int64_t *granule,
                               OggPage *pages, int64_t cap, int64_t *file_bytes) {
  OggWalk w;
  ogg_walk_init(w, 0);
  if (header_bytes) ogg_walk_headers(w, pages, cap, header_bytes);
  ogg_run_begin(w, 2, 0);
  ogg_walk_audio(w, pages, cap, 0, npackets, bytes, granule);
  ogg_run_end(w, pages, cap, 1);
  if (file_bytes) *file_bytes = w.file_off;
  return w.npages;
}

// one page of a planned stream laid out at `dst` (header, lacing, body, checksum): list[] / bytes[] the packets of its run
inline void ogg_write_page(const OggPage &pg, uint32_t serial, const uint8_t *const *list, const int32_t *bytes, uint8_t *dst) {
  ogg_page_header(pg, serial, dst);
  uint8_t *lace = dst + OGG_HEADER, *body = lace + pg.nseg;
  int segs = 0;
  for (int j = 0; j < pg.npackets; j++) {
    const int32_t n = bytes[pg.first + j], start = j == 0 ? pg.byte0 : 0, left = ogg_segments(n) - start / 255;
    const int32_t take = left < pg.nseg - segs ? left : pg.nseg - segs, len = ogg_piece_len(n, start, take);
    for (int q = 0; q < take; q++) lace[segs + q] = (uint8_t)ogg_lace_value(n, start / 255 + q);
    if (len) memcpy(body, list[pg.first + j] + start, (size_t)len);
    segs += take, body += len;
  }
  const int64_t total = OGG_HEADER + pg.nseg + pg.body;
  const uint32_t crc = ogg_crc_chunked(dst, total, OGG_CRC_MIN_CHUNK, OGG_CRC_LANES);
  for (int i = 0; i < 4; i++) dst[22 + i] = (uint8_t)(crc >> (8 * i));
}

// a whole file: headers[3] (null: audio pages only, a bare run for the CPU suite), the audio packets.  Returns the file's
// bytes; writes them when they fit `cap`.
inline int64_t ogg_mux(const uint8_t *const *headers, const int32_t *header_bytes, int64_t npackets, const uint8_t *const *packets,
                       const int32_t *bytes, const int64_t *granule, uint32_t serial, uint8_t *out, int64_t cap, OggPage *pages,
                       int64_t page_cap, int64_t *npages) {
  int64_t total = 0;
  const int64_t np = ogg_plan_stream(headers ? header_bytes : nullptr, npackets, bytes, granule, pages, page_cap, &total);
  if (npages) *npages = np;
  if (np > page_cap || total > cap) return total;
  for (int64_t p = 0; p < np; p++) {
    const OggPage &pg = pages[p];
    if (pg.run == 2) ogg_write_page(pg, serial, packets, bytes, out + pg.file_off);
    else ogg_write_page(pg, serial, headers, header_bytes, out + pg.file_off);
  }
  return total;
}

// ---- a file in pieces (a live feed's groups; the second implementation k_ogg_plan / k_ogg_pages / k_ogg_carry are held
// against) ----
// A stream between two pieces: the walk with its open page, and the carried packets end to end
struct OggPieces {
  OggWalk w;
  int32_t ncarry;
  int32_t cbytes[OGG_MAX_SEGS];
  uint8_t cdata[OGG_CARRY_BODY];
};
// The resumed walk over one group: begin (the stream starts here: T is reset, the headers walked when header_bytes is
// given), npackets new packets behind the T.ncarry carried ones, close (the run ends).  pages[] <- the pages the group
// completes, their file_off absolute; returns their number; T.w is the walk at the group's end, not yet rebased.
// flush (without close): the open page leaves with the group (ogg_flush); T.w.pg is empty then.
inline int64_t ogg_plan_piece(OggPieces &T, int begin, const int32_t *header_bytes, int64_t npackets, const int32_t *bytes,
                              const int64_t *granule, int close, OggPage *pages, int64_t cap, int flush = 0) {
  if (begin) {
    ogg_walk_init(T.w, 0);
    T.ncarry = 0;
    if (header_bytes) ogg_walk_headers(T.w, pages, cap, header_bytes);
    ogg_run_begin(T.w, 2, 0);
  }
  ogg_walk_audio(T.w, pages, cap, T.ncarry, npackets, bytes, granule);
  if (close) ogg_run_end(T.w, pages, cap, 1);
  else if (flush) ogg_flush(T.w, pages, cap);
  return T.w.npages;
}
// One group of the mux in pieces: the bytes of the pages it completes into out (returned; written when they and the pages
// fit), the next state and carry into T.  *open_page (optional): the page left open, as it stood before the rebase.
// flush (default: none): the stream is flushed behind this group's packets -- the open page is among the group's pages,
// the page left open and the carry are empty.
inline int64_t ogg_mux_piece(OggPieces &T, int begin, const uint8_t *const *headers, const int32_t *header_bytes, int64_t npackets,
                             const uint8_t *const *packets, const int32_t *bytes, const int64_t *granule, int close, uint32_t serial,
                             uint8_t *out, int64_t cap, OggPage *pages, int64_t page_cap, int64_t *npages, OggPage *open_page,
                             int flush = 0) {
  const int64_t start = begin ? 0 : T.w.file_off;
  const int32_t nc = begin ? 0 : T.ncarry;
  const int64_t np = ogg_plan_piece(T, begin, headers ? header_bytes : nullptr, npackets, bytes, granule, close, pages, page_cap, flush);
  const int64_t total = T.w.file_off - start;
  if (npages) *npages = np;
  if (open_page) *open_page = T.w.pg;
  // the group's list: the carried packets, then its own
  std::vector<const uint8_t *> list((size_t)(nc + npackets));
  std::vector<int32_t> size((size_t)(nc + npackets));
  int64_t at = 0;
  for (int32_t v = 0; v < nc; v++) list[(size_t)v] = T.cdata + at, size[(size_t)v] = T.cbytes[v], at += T.cbytes[v];
  for (int64_t k = 0; k < npackets; k++) list[(size_t)(nc + k)] = packets[k], size[(size_t)(nc + k)] = bytes[k];
  if (np <= page_cap && total <= cap)
    for (int64_t p = 0; p < np; p++) {
      const OggPage &pg = pages[p];
      if (pg.run == 2) ogg_write_page(pg, serial, list.data(), size.data(), out + (pg.file_off - start));
      else ogg_write_page(pg, serial, headers, header_bytes, out + (pg.file_off - start));
    }
  // the next carry: what lies on the open page
  const OggPage &pg = T.w.pg;
  std::vector<uint8_t> data;
  int32_t nb[OGG_MAX_SEGS];
  for (int32_t j = 0; j < pg.npackets && j < OGG_MAX_SEGS; j++) {
    const int32_t skip = j == 0 ? pg.byte0 : 0;
    nb[j] = size[(size_t)(pg.first + j)] - skip;
    data.insert(data.end(), list[(size_t)(pg.first + j)] + skip, list[(size_t)(pg.first + j)] + skip + nb[j]);
  }
  T.ncarry = close ? 0 : pg.npackets;
  if (!close && data.size() <= (size_t)OGG_CARRY_BODY) {
    memcpy(T.cbytes, nb, sizeof(int32_t) * (size_t)pg.npackets);
    if (!data.empty()) memcpy(T.cdata, data.data(), data.size());
  }
  ogg_walk_rebase(T.w);
  return total;
}
#endif

}  // namespace vamd
