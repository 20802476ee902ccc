// decode_layout_host.cpp -- the decoder's plan image (vorbis_amd/csrc/vamd_decode_layout.h, the shipped header): where
// decode_layout puts the parts for every kind of call and every small count, and what decode_image_fill writes into them
// for a hand-made plan of three packets.  A program of its own for -fsanitize=address,undefined: the image is a heap block
// of exactly the layout's size between guard bytes, and every list handed in is a heap block of exactly its count, so a
// read or write past either end is the sanitizer's to report.  CPU only.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "vamd_bind.h"
#include "vamd_decode_layout.h"

using namespace vamd;

static long g_cases = 0, g_bad = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    g_cases++;                           \
    if (!(cond)) {                       \
      if (g_bad++ < 20) {                \
        printf("  FAILED %s: ", #cond);  \
        printf(__VA_ARGS__);             \
        printf("\n");                    \
      }                                  \
    }                                    \
  } while (0)

struct Part {
  const char *name;
  size_t at, bytes;
};

// the parts of a layout with the bytes each holds (a src list has its spare entry: LapP's pointers are never dangling)
static int parts_of(const DecodeCounts &n, const DecodeLayout &o, Part p[16]) {
  const Part all[16] = {
      {"order", o.order, 4 * n.nlap},
      {"start", o.start, 8 * (n.ns + 1)},
      {"src0", o.src[0], 8 * n.nsrc[0] + 8},
      {"src1", o.src[1], 8 * n.nsrc[1] + 8},
      {"bits", o.bits, 16 * n.nb},
      {"frames", o.frames, 8 * n.ns},
      {"off", o.off, 8 * n.ns},
      {"pages", o.pages, sizeof(OggDepage) * n.npg},
      {"in", o.in, sizeof(CarryRow) * n.nin},
      {"out", o.out, sizeof(CarryRow) * n.nout},
      {"bin", o.bin, sizeof(OggCarryRow) * n.nbin},
      {"bout", o.bout, sizeof(OggCarryRow) * n.nbout},
      {"first", o.first, n.win ? 8 * n.ns : 0},
      {"stride", o.stride, n.win ? 8 * n.ns : 0},
      {"seg", o.seg, sizeof(LapSegment) * n.nseg},
      {"unpack", o.unpack, 4 * n.nb},  // (a part of its own in a live call alone: else it is order)
  };
  const int count = n.live ? 16 : 15;
  for (int i = 0; i < count; i++) p[i] = all[i];
  return count;
}

static void layout_case(const DecodeCounts &n) {
  const DecodeLayout o = decode_layout(n);
  Part p[16];
  const int count = parts_of(n, o, p);
  unsigned bad = 0;
  for (int i = 0; i < count; i++) {
    if (p[i].at % 16) bad |= 1;
    if (!p[i].bytes) continue;
    if (p[i].at + p[i].bytes > o.plan_bytes) bad |= 2;
    for (int j = i + 1; j < count; j++)
      if (p[j].bytes && p[i].at < p[j].at + p[j].bytes && p[j].at < p[i].at + p[i].bytes) bad |= 4;
  }
  if (o.status % 16 || o.plan_bytes % 16) bad |= 1;
  if (o.status < o.plan_bytes || o.status + n.nb + n.npg > o.total) bad |= 8;
  if ((o.unpack == o.order) != !n.live) bad |= 16;
  CHECK(!bad, "bits %u (1 alignment, 2 beyond plan_bytes, 4 overlap, 8 statuses, 16 unpack / order) at nb %zu nlap %zu ns %zu src %zu %zu npg %zu live %d in %zu out %zu bin %zu bout %zu win %d nseg %zu",
        bad, n.nb, n.nlap, n.ns, n.nsrc[0], n.nsrc[1], n.npg, (int)n.live, n.nin, n.nout, n.nbin, n.nbout, (int)n.win, n.nseg);
}

// pages absent / present x live x byte carry (live and pages) x windows x segments, every count of a part that the call
// has in {0, 1, 3}; a call that is not live unpacks order[] itself, so nb is nlap there
static void layout_cases() {
  const size_t V[3] = {0, 1, 3}, none[1] = {0};
  for (int pages = 0; pages < 2; pages++)
    for (int live = 0; live < 2; live++)
      for (int carry = 0; carry < (live && pages ? 2 : 1); carry++)
        for (int win = 0; win < 2; win++)
          for (int seg = 0; seg < 2; seg++) {
            const size_t *Vpg = pages ? V : none, *Vlive = live ? V : none, *Vcarry = carry ? V : none, *Vseg = seg ? V : none;
            const int kpg = pages ? 3 : 1, klive = live ? 3 : 1, kcarry = carry ? 3 : 1, kseg = seg ? 3 : 1;
            DecodeCounts n;
            n.live = live != 0, n.win = win != 0;
            for (int a = 0; a < 3; a++)
              for (int b = 0; b < klive; b++)
                for (int c = 0; c < 3; c++)
                  for (int d = 0; d < 9; d++)
                    for (int e = 0; e < kpg; e++)
                      for (int f = 0; f < klive * klive; f++)
                        for (int g = 0; g < kcarry * kcarry; g++)
                          for (int h = 0; h < kseg; h++) {
                            n.nb = V[a], n.nlap = live ? Vlive[b] : n.nb, n.ns = V[c], n.nsrc[0] = V[d % 3], n.nsrc[1] = V[d / 3];
                            n.npg = Vpg[e], n.nin = Vlive[f % klive], n.nout = Vlive[f / klive];
                            n.nbin = Vcarry[g % kcarry], n.nbout = Vcarry[g / kcarry], n.nseg = Vseg[h];
                            layout_case(n);
                          }
          }
}

// a heap copy of exactly n elements (null for none): what is read beyond it is the sanitizer's to report
template <class T> static T *exact(const std::vector<T> &v) {
  if (v.empty()) return nullptr;
  T *p = (T *)malloc(v.size() * sizeof(T));
  memcpy(p, v.data(), v.size() * sizeof(T));
  return p;
}
template <class T> static bool holds(const unsigned char *h, size_t at, const std::vector<T> &v) {
  return v.empty() || !memcmp(h + at, v.data(), v.size() * sizeof(T));
}

// Three packets of 5, 0 and 9 bytes in an arena that begins at byte 100 of the caller's numbering, two streams (the second
// without frames), blocks in the order 2, 0, 1 of the packets; with `begin`, the packets lie apart and offset[] gives the
// lengths alone.  live: a list for k_unpack of its own and the four carry tables; win: the window lists; interleaved: the
// segment rows' out in elements of ch = 2 channels.
static void fill_case(bool with_begin, bool live, bool win, bool interleaved) {
  const int ch = 2;
  const std::vector<int64_t> offset = {100, 105, 105, 114}, begin = {140, 100, 120}, packet = {2, 0, 1};
  const std::vector<int32_t> order = {0, (1 << 30) | 0, 1, 2}, unpack = {(1 << 30) | 0, 1, 2};
  const std::vector<int64_t> start = {0, live ? 4 : 3, live ? 4 : 3}, src0 = {-64, 64, 192}, src1 = {-512}, frames = {777, 0}, offset_out = {32, -5};
  const std::vector<int64_t> first = {11, 12}, stride = {800, 900};
  std::vector<OggDepage> pages(2);
  memset(pages.data(), 0x5a, pages.size() * sizeof(OggDepage));
  std::vector<CarryRow> in = {{1, 0, 3}}, out = {{2, 1, 0}, {1, 0, 2}};
  std::vector<OggCarryRow> bin(1), bout(3);
  memset(bin.data(), 0x21, bin.size() * sizeof(OggCarryRow));
  memset(bout.data(), 0x43, bout.size() * sizeof(OggCarryRow));
  const std::vector<DecodePlan::Segment> seg = {{0, 0, 4, 7, 300, 0}, {0, 0, 4, 400, 477, 300}};

  DecodeCounts n;
  n.live = live, n.win = win;
  n.nb = packet.size(), n.nlap = live ? order.size() : packet.size(), n.ns = 2, n.nsrc[0] = src0.size(), n.nsrc[1] = src1.size();
  n.npg = pages.size(), n.nseg = seg.size();
  if (live) n.nin = in.size(), n.nout = out.size(), n.nbin = bin.size(), n.nbout = bout.size();
  const std::vector<int32_t> lap(order.begin(), order.begin() + (long)n.nlap);
  const DecodeLayout o = decode_layout(n);

  DecodeImage s;
  s.order = exact(lap), s.start = exact(start), s.src[0] = exact(src0), s.src[1] = exact(src1), s.packet = exact(packet);
  s.offset = exact(offset), s.begin = with_begin ? exact(begin) : nullptr, s.byte0 = 100;
  s.frames = exact(frames), s.offset_out = exact(offset_out), s.pages = exact(pages);
  if (live) s.unpack = exact(unpack), s.in = exact(in), s.out = exact(out), s.bin = exact(bin), s.bout = exact(bout);
  if (win) s.first = exact(first), s.stride = exact(stride);
  s.seg = exact(seg), s.out_scale = interleaved ? ch : 1;

  const size_t guard = 64;
  unsigned char *block = (unsigned char *)malloc(o.total + 2 * guard), *h = block + guard;
  memset(block, 0xa5, o.total + 2 * guard);
  decode_image_fill(n, o, s, h);

  const char *what = with_begin ? (live ? "begin, live" : "begin") : (live ? "live" : "plain");
  bool guards = true;
  for (size_t i = 0; i < guard; i++) guards = guards && block[i] == 0xa5 && h[o.total + i] == 0xa5;
  for (size_t i = o.status; i < o.total; i++) guards = guards && h[i] == 0xa5;  // (the statuses are the device's to write)
  CHECK(guards, "%s: a byte outside the image's parts was written", what);
  CHECK(holds(h, o.order, lap) && holds(h, o.start, start) && holds(h, o.src[0], src0) && holds(h, o.src[1], src1), "%s: order / start / src", what);
  CHECK(holds(h, o.frames, frames) && holds(h, o.pages, pages), "%s: frames / pages", what);
  CHECK((o.unpack == o.order) == !live && (!live || holds(h, o.unpack, unpack)), "%s: the list for k_unpack", what);
  if (live) CHECK(holds(h, o.in, in) && holds(h, o.out, out) && holds(h, o.bin, bin) && holds(h, o.bout, bout), "%s: the carry tables", what);
  if (win) CHECK(holds(h, o.first, first) && holds(h, o.stride, stride), "%s: the window lists", what);
  for (size_t k = 0; k < packet.size(); k++) {
    const int64_t p = packet[k], at = with_begin ? begin[(size_t)p] : offset[(size_t)p], len = offset[(size_t)p + 1] - offset[(size_t)p];
    int64_t bits[2];
    memcpy(bits, h + o.bits + 16 * k, 16);
    CHECK(bits[0] == 8 * (at - 100) && bits[1] == 8 * (at + len - 100), "%s: block %zu has bits [%lld, %lld)", what, k, (long long)bits[0], (long long)bits[1]);
  }
  int64_t off[2];
  memcpy(off, h + o.off, 16);
  CHECK(off[0] == 32 && off[1] == 0, "%s: offset_out of a stream with frames as given, of one without 0 (%lld, %lld)", what, (long long)off[0], (long long)off[1]);
  for (size_t g = 0; g < seg.size(); g++) {
    LapSegment row;
    memcpy(&row, h + o.seg + g * sizeof(LapSegment), sizeof(row));
    const DecodePlan::Segment &e = seg[g];
    CHECK(row.k0 == e.k0 && row.k1 == e.k1 && row.first == e.first && row.count == e.count && row.stride == 777, "%s: segment %zu's blocks, frames and stride", what, g);
    CHECK(row.out == 32 + e.out_at * (interleaved ? ch : 1), "%s: segment %zu's out %lld under %s", what, g, row.out, interleaved ? "interleaving" : "planar rows");
  }

  free(block);
  const void *lists[] = {s.order, s.start, s.src[0], s.src[1], s.packet, s.offset, s.begin, s.frames, s.offset_out, s.pages, s.unpack,
                         s.in, s.out, s.bin, s.bout, s.first, s.stride, s.seg};
  for (const void *l : lists) free((void *)l);
}

int main() {
  layout_cases();
  const long layouts = g_cases;
  for (int m = 0; m < 16; m++) fill_case(m & 1, m & 2, m & 4, m & 8);
  printf("%ld layouts, %ld checks: %s\n", layouts, g_cases, g_bad ? "FAILED" : "ok");
  return g_bad ? 1 : 0;
}
