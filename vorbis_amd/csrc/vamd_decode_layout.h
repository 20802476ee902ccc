// vamd_decode_layout.h -- the plan image of a decoder call: where its parts lie and what the host writes into them.  No HIP
// header: decode_run (vamd_decode.h) lays out and fills its pinned buffer with the two functions below, and a host program
// (tests/c/decode_layout_host.cpp) holds them to what the kernels read.
// The image, one piece, every part on a 16-byte boundary (Arena): order | stream_start | src per size class | the packets'
// bits | frames | offset_out | the page table | a live call's list for k_unpack and its two carry tables | a live Ogg call's
// two byte-carry tables | a window call's first frames and channel strides | a marked plan's segment rows.  That much goes
// up (plan_bytes); behind it, on the host alone, the statuses come back: the blocks', then the pages'.
#pragma once
#include "vamd_arena.h"
#include "vamd_decode_live_plan.h"
#include "vamd_demux.h"

namespace vamd {

// how many of each a call has.  nb: the blocks that have a packet (k_unpack's); nlap: the blocks of order[] (a live call's
// carried blocks among them); ns: the plan's streams, or windows.
struct DecodeCounts {
  size_t nb = 0, nlap = 0, ns = 0, nsrc[2] = {0, 0}, npg = 0;
  bool live = false;   // k_unpack takes a list of its own (nb entries), not order[]
  size_t nin = 0, nout = 0, nbin = 0, nbout = 0;
  bool win = false;    // the windows' first frames and channel strides ([ns] each)
  size_t nseg = 0;
};

struct DecodeLayout {
  size_t order, start, src[2], bits, frames, off, pages, unpack, in, out, bin, bout, first, stride, seg;
  size_t plan_bytes;  // what the device reads
  size_t status;      // [nb + npg], in the pinned buffer alone
  size_t total;
};

inline DecodeLayout decode_layout(const DecodeCounts &n) {
  Arena a;
  DecodeLayout o;
  o.order = a.take(4 * n.nlap);
  o.start = a.take(8 * (n.ns + 1));
  o.src[0] = a.take(8 * n.nsrc[0] + 8);
  o.src[1] = a.take(8 * n.nsrc[1] + 8);
  o.bits = a.take(16 * n.nb);
  o.frames = a.take(8 * n.ns);
  o.off = a.take(8 * n.ns);
  o.pages = a.take(sizeof(OggDepage) * n.npg);
  o.unpack = n.live ? a.take(4 * n.nb) : o.order;
  o.in = a.take(sizeof(CarryRow) * n.nin);
  o.out = a.take(sizeof(CarryRow) * n.nout);
  o.bin = a.take(sizeof(OggCarryRow) * n.nbin);
  o.bout = a.take(sizeof(OggCarryRow) * n.nbout);
  o.first = a.take(n.win ? 8 * n.ns : 0);
  o.stride = a.take(n.win ? 8 * n.ns : 0);
  o.seg = a.take(sizeof(LapSegment) * n.nseg);
  o.plan_bytes = a.at;
  o.status = a.take(n.nb + n.npg);
  o.total = a.at;
  return o;
}

// what the image is written from: the plan's lists and the call's tables, each as long as its count says (a list whose
// count is 0 is not read and may be null)
struct DecodeImage {
  const int32_t *order = nullptr;        // [nlap]
  const int64_t *start = nullptr;        // [ns + 1]
  const int64_t *src[2] = {nullptr, nullptr};
  const int64_t *packet = nullptr;       // [nb] the packet of each block k_unpack takes
  const int64_t *offset = nullptr;       // [packets + 1] the packets' bytes; the arena begins at byte0 of this numbering
  const int64_t *begin = nullptr;        // or [packets]: where each packet begins (offset[] then gives the lengths alone)
  int64_t byte0 = 0;
  const int64_t *frames = nullptr;       // [ns]
  const int64_t *offset_out = nullptr;   // [ns] read where the stream has frames
  const OggDepage *pages = nullptr;      // [npg]
  const int32_t *unpack = nullptr;       // [nb] (live)
  const CarryRow *in = nullptr, *out = nullptr;
  const OggCarryRow *bin = nullptr, *bout = nullptr;
  const int64_t *first = nullptr, *stride = nullptr;  // [ns] (win)
  const DecodePlan::Segment *seg = nullptr;            // [nseg]
  int out_scale = 1;  // elements a frame of a segment's out_at: the channels under an interleaved format, else 1
};

inline void decode_image_put(unsigned char *h, size_t at, const void *from, size_t bytes) {
  if (bytes) memcpy(h + at, from, bytes);
}

inline void decode_image_fill(const DecodeCounts &n, const DecodeLayout &o, const DecodeImage &s, unsigned char *h) {
  decode_image_put(h, o.order, s.order, 4 * n.nlap);
  if (n.live) decode_image_put(h, o.unpack, s.unpack, 4 * n.nb);
  decode_image_put(h, o.in, s.in, sizeof(CarryRow) * n.nin);
  decode_image_put(h, o.out, s.out, sizeof(CarryRow) * n.nout);
  decode_image_put(h, o.bin, s.bin, sizeof(OggCarryRow) * n.nbin);
  decode_image_put(h, o.bout, s.bout, sizeof(OggCarryRow) * n.nbout);
  decode_image_put(h, o.start, s.start, 8 * (n.ns + 1));
  decode_image_put(h, o.src[0], s.src[0], 8 * n.nsrc[0]);
  decode_image_put(h, o.src[1], s.src[1], 8 * n.nsrc[1]);
  for (size_t k = 0; k < n.nb; k++) {
    const int64_t p = s.packet[k];
    const int64_t at = s.begin ? s.begin[p] : s.offset[p];
    const int64_t bits[2] = {8 * (at - s.byte0), 8 * (at + (s.offset[p + 1] - s.offset[p]) - s.byte0)};
    memcpy(h + o.bits + 16 * k, bits, 16);
  }
  decode_image_put(h, o.frames, s.frames, 8 * n.ns);
  for (size_t st = 0; st < n.ns; st++) {
    const int64_t off = s.frames[st] > 0 ? s.offset_out[st] : 0;
    memcpy(h + o.off + 8 * st, &off, 8);
  }
  decode_image_put(h, o.pages, s.pages, sizeof(OggDepage) * n.npg);
  if (n.win) decode_image_put(h, o.first, s.first, 8 * n.ns), decode_image_put(h, o.stride, s.stride, 8 * n.ns);
  for (size_t g = 0; g < n.nseg; g++) {  // (a stream's rows fill its [ch][frames] from 0 to frames, in order)
    const DecodePlan::Segment &e = s.seg[g];
    const LapSegment row = {e.k0, e.k1, e.first, e.count, s.frames[(size_t)e.stream], s.offset_out[e.stream] + e.out_at * s.out_scale};
    memcpy(h + o.seg + g * sizeof(LapSegment), &row, sizeof(row));
  }
}

}  // namespace vamd
