// feed_host_cases.cpp -- the feed's host arithmetic (vorbis_amd/csrc/vamd_feed_host.h, the shipped header) on crafted cases:
// plan_slices against a brute-force restatement per slice, the comment table's image, the two record layouts, the live
// mirror's two steps.  A program of its own for -fsanitize=address,undefined: every array is a heap block of exactly the
// size visited, so a read or write past either end is the sanitizer's to report.  CPU only.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "vamd_feed_host.h"

using namespace vamd;

static int g_cases = 0, g_bad = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    g_cases++;                           \
    if (!(cond)) {                       \
      g_bad++;                           \
      printf("  FAILED %s: ", #cond);    \
      printf(__VA_ARGS__);               \
      printf("\n");                      \
    }                                    \
  } while (0)

// ---- plan_slices ----
static void slices_case(long S) {
  const long counts[5] = {0, 1, 11, 3, 0}, ns = 5;
  long nb = 0;
  std::vector<int64_t> start((size_t)ns + 1);
  for (long s = 0; s < ns; s++) start[(size_t)s] = nb, nb += counts[s];
  start[(size_t)ns] = nb;
  // the two size classes interleaved: block k is of class k & 1 but for a run of three long ones, numbered in stream order
  std::vector<int32_t> plan((size_t)nb), sid((size_t)nb);
  {
    int seen[2] = {0, 0};
    for (long k = 0; k < nb; k++) {
      const int W = (k >= 5 && k < 8) ? 1 : (int)(k & 1);
      plan[(size_t)k] = (W << 30) | seen[W]++;
    }
    for (long s = 0; s < ns; s++)
      for (int64_t k = start[(size_t)s]; k < start[(size_t)s + 1]; k++) sid[(size_t)k] = (int32_t)s;
  }
  std::vector<int32_t> order(plan.begin(), plan.end());
  std::vector<int64_t> starts;
  const char *why = nullptr;
  const std::vector<Slice> sl = plan_slices(order, start, ns, nb, S, starts, &why);
  CHECK(!why, "S %ld: %s", S, why);
  CHECK((long)sl.size() == (nb + S - 1) / S, "S %ld: %zu slices", S, sl.size());
  size_t at = 0;
  for (size_t j = 0; j < sl.size(); j++) {
    const Slice &x = sl[j];
    const long k0 = (long)j * S, k1 = k0 + S < nb ? k0 + S : nb;
    CHECK(x.k0 == k0 && x.k1 == k1, "S %ld slice %zu: [%ld, %ld), expected [%ld, %ld)", S, j, x.k0, x.k1, k0, k1);
    const long s0 = sid[(size_t)k0], s1 = sid[(size_t)k1 - 1] + 1;  // the streams of its first and last block
    CHECK(x.s0 == s0 && x.s1 == s1, "S %ld slice %zu: streams [%ld, %ld), expected [%ld, %ld)", S, j, x.s0, x.s1, s0, s1);
    int64_t i0[2] = {0, 0}, n[2] = {0, 0};
    for (long k = 0; k < k1; k++) {
      const int W = (plan[(size_t)k] >> 30) & 1;
      if (k < k0) i0[W]++;
      else n[W]++;
    }
    for (int W = 0; W < 2; W++)
      CHECK(x.i0[W] == i0[W] && x.n[W] == n[W], "S %ld slice %zu class %d: i0 %ld n %ld, expected %ld %ld", S, j, W, (long)x.i0[W], (long)x.n[W],
            (long)i0[W], (long)n[W]);
    for (long k = k0; k < k1; k++) {
      const int W = (plan[(size_t)k] >> 30) & 1;
      const int32_t want = (W << 30) | (int32_t)((plan[(size_t)k] & 0x3fffffff) - i0[W]);
      CHECK(order[(size_t)k] == want, "S %ld slice %zu: order[%ld] = %x, expected %x", S, j, k, order[(size_t)k], want);
    }
    CHECK(x.starts == at, "S %ld slice %zu: its stream_start lies at %zu, expected %zu", S, j, x.starts, at);
    for (long s = s0; s <= s1; s++, at++) {  // stream_start[s - s0]: the slice's blocks in streams before s
      int64_t before = 0;
      for (long k = k0; k < k1; k++) before += sid[(size_t)k] < s;
      CHECK(at < starts.size() && starts[at] == before, "S %ld slice %zu: stream_start[%ld] = %ld, expected %ld", S, j, s - s0,
            at < starts.size() ? (long)starts[at] : -1L, (long)before);
    }
  }
  CHECK(at == starts.size(), "S %ld: %zu entries of starts, expected %zu", S, starts.size(), at);
}

static void slices_out_of_order() {
  const long ns = 1, nb = 4;
  const int64_t st[2] = {0, 4};
  const int32_t o[4] = {0, 2, 1, 3};  // class 0's blocks not numbered in stream order
  std::vector<int64_t> start(st, st + ns + 1), starts;
  std::vector<int32_t> order(o, o + nb);
  const char *why = nullptr;
  (void)plan_slices(order, start, ns, nb, 3, starts, &why);
  CHECK(why != nullptr, "a plan out of stream order is not refused");
}

// ---- the comment table ----
static std::vector<uint8_t> bytes_of(size_t n, uint8_t first) {
  std::vector<uint8_t> v(n);
  for (size_t i = 0; i < n; i++) v[i] = (uint8_t)(first + i);
  return v;
}

static void comment_case(const std::vector<std::vector<uint8_t>> &comments, long ns, int32_t shared, size_t want_bytes, int32_t want_longest,
                         int64_t want_sum, const int64_t *want_off, const int32_t *want_len, const char *name) {
  const CommentTable T = comment_table(comments, ns, shared);
  CHECK(T.bytes == want_bytes && T.longest == want_longest && T.sum == want_sum, "%s: bytes %zu longest %d sum %ld, expected %zu %d %ld", name, T.bytes,
        T.longest, (long)T.sum, want_bytes, want_longest, (long)want_sum);
  uint8_t *img = (uint8_t *)malloc(T.bytes);
  memset(img, 0xee, T.bytes);
  comment_table_image(comments, ns, T, img);
  int64_t *off = (int64_t *)malloc((size_t)ns * 8);
  int32_t *len = (int32_t *)malloc((size_t)ns * 4);
  memcpy(off, img, (size_t)ns * 8);
  memcpy(len, img + (size_t)ns * 8, (size_t)ns * 4);
  for (long s = 0; s < ns; s++) {
    CHECK(off[s] == want_off[s] && len[s] == want_len[s], "%s stream %ld: off %ld len %d, expected %ld %d", name, s, (long)off[s], len[s],
          (long)want_off[s], want_len[s]);
    CHECK(off[s] % 4 == 0, "%s stream %ld: offset %ld is no multiple of 4", name, s, (long)off[s]);
    if (len[s] < 0) continue;
    CHECK((size_t)off[s] + (size_t)len[s] + 8 <= T.bytes && !memcmp(img + off[s], comments[(size_t)s].data(), (size_t)len[s]), "%s stream %ld: its bytes",
          name, s);
  }
  free(img), free(off), free(len);
}

static void comment_cases() {
  {  // own comments of 1 and 7 bytes on streams 0 and 2, none on stream 1; the table takes al(3 * 12, 8) = 40 bytes
    const std::vector<std::vector<uint8_t>> c = {bytes_of(1, 0x10), {}, bytes_of(7, 0x20)};
    const int64_t off[3] = {40, 44, 44};
    const int32_t len[3] = {1, -1, 7};
    comment_case(c, 3, 5, 40 + 4 + 8 + 8, 7, 1 + 5 + 7, off, len, "own 1 / shared 5 / own 7");
    comment_case(c, 3, 9, 40 + 4 + 8 + 8, 9, 1 + 9 + 7, off, len, "own 1 / shared 9 / own 7");  // (the shared one is the longest)
  }
  {  // a vector shorter than ns: the streams beyond it have the shared comment
    const std::vector<std::vector<uint8_t>> c = {bytes_of(3, 0x30)};
    const int64_t off[3] = {40, 44, 44};
    const int32_t len[3] = {3, -1, -1};
    comment_case(c, 3, 6, 40 + 4 + 8, 6, 3 + 6 + 6, off, len, "own 3 / beyond the vector / beyond the vector");
  }
}

// ---- the two record layouts ----
struct Field {
  const char *name;
  size_t at, elems, size;
};

// the fields lie inside the record, in order without overlap, each aligned as its type needs; and every element of every
// field can be written and read back through the pointers point() sets, in a heap block of exactly `bytes`
static void fields_check(const char *what, long ns, long nb, const Field *fl, int nf, size_t bytes) {
  size_t end = 8;  // (the total)
  for (int i = 0; i < nf; i++) {
    CHECK(fl[i].at >= end, "%s (%ld, %ld): %s at %zu overlaps what lies before it (ends at %zu)", what, ns, nb, fl[i].name, fl[i].at, end);
    CHECK(fl[i].at % fl[i].size == 0, "%s (%ld, %ld): %s at %zu is not aligned to %zu", what, ns, nb, fl[i].name, fl[i].at, fl[i].size);
    end = fl[i].at + fl[i].elems * fl[i].size;
  }
  CHECK(end <= bytes && bytes % 16 == 0, "%s (%ld, %ld): fields end at %zu, the record has %zu bytes", what, ns, nb, end, bytes);
}

struct RecView {
  int64_t *stream_start, *offset, *granulepos;
  int32_t *bits;
  uint8_t *info;
};
struct OggRecView {
  int64_t *stream_offset;
  int32_t *npages;
  uint8_t *status;
};

static void layout_case(long ns, long nb) {
  {
    const RecLayout R(ns, nb);
    const Field fl[5] = {{"stream_start", R.start, (size_t)ns + 1, 8}, {"offset", R.offset, (size_t)nb, 8}, {"granulepos", R.granulepos, (size_t)nb, 8},
                         {"bits", R.bits, (size_t)nb, 4}, {"info", R.info, (size_t)nb, 1}};
    fields_check("group record", ns, nb, fl, 5, R.bytes);
    uint8_t *rec = (uint8_t *)malloc(R.bytes);
    RecView v;
    R.point(rec, v);
    *(int64_t *)rec = -1;
    for (long s = 0; s <= ns; s++) v.stream_start[s] = 100 + s;
    for (long k = 0; k < nb; k++) v.offset[k] = 200 + k, v.granulepos[k] = 300 + k, v.bits[k] = 400 + (int32_t)k, v.info[k] = (uint8_t)(50 + k);
    bool same = *(int64_t *)rec == -1;
    for (long s = 0; s <= ns; s++) same &= v.stream_start[s] == 100 + s;
    for (long k = 0; k < nb; k++) same &= v.offset[k] == 200 + k && v.granulepos[k] == 300 + k && v.bits[k] == 400 + k && v.info[k] == 50 + k;
    CHECK(same, "group record (%ld, %ld): a field's write changed another's", ns, nb);
    free(rec);
  }
  {
    const OggRecLayout R(ns);
    const Field fl[3] = {{"stream_offset", R.offset, (size_t)ns + 1, 8}, {"npages", R.npages, (size_t)ns, 4}, {"status", R.status, (size_t)ns, 1}};
    fields_check("Ogg record", ns, nb, fl, 3, R.bytes);
    uint8_t *rec = (uint8_t *)malloc(R.bytes);
    OggRecView v;
    R.point(rec, v);
    *(int64_t *)rec = -1;
    for (long s = 0; s <= ns; s++) v.stream_offset[s] = 100 + s;
    for (long s = 0; s < ns; s++) v.npages[s] = 200 + (int32_t)s, v.status[s] = (uint8_t)(30 + s);
    bool same = *(int64_t *)rec == -1;
    for (long s = 0; s <= ns; s++) same &= v.stream_offset[s] == 100 + s;
    for (long s = 0; s < ns; s++) same &= v.npages[s] == 200 + s && v.status[s] == 30 + s;
    CHECK(same, "Ogg record (%ld): a field's write changed another's", ns);
    free(rec);
  }
}

// ---- the live mirror: block sizes 256 / 2048, 777 frames per write ----
// head room 1024, end-of-stream padding 6144, detector step 64; the backward extrapolation waits for (2048 / 777 + 1) * 777 =
// 2331 frames (lib/block.c:525-526)
struct Piece {
  LiveIn *in;
  vamd_live_geo *g;
  int64_t quads = 0;
  const char *why = nullptr;
  Piece() : in((LiveIn *)malloc(sizeof(LiveIn))), g((vamd_live_geo *)malloc(sizeof(vamd_live_geo))) {}
  ~Piece() { free(in), free(g); }
  void take(const LiveShape &G, LiveStream &m, int64_t n, bool cl) { why = live_piece(G, m, 7, n, cl, *in, *g, &quads); }
};

static void live_cases() {
  const long cs = 20000;
  const LiveShape G(2048, 777, cs);
  CHECK(G.head == 1024 && G.pad == 6144 && G.step == 64 && G.n_head == 2331 && G.cs == cs, "the shape: head %d pad %d step %d n_head %ld", G.head, G.pad,
        G.step, G.n_head);
  {  // a fresh stream with 0 frames is absent and nothing is carried
    LiveStream m;
    Piece p;
    p.take(G, m, 0, false);
    CHECK(!p.why && p.in->fresh == 1 && p.in->frames == 0 && p.in->keep == 0 && p.in->shift == 0 && p.in->eof == LIVE_OPEN && p.in->close == 0,
          "absent stream: its LiveIn");
    CHECK(p.g->fresh == 1 && p.g->have == 0 && p.g->kept == 0 && p.g->c1 == 0 && p.g->c2 == 0 && p.g->n_head == 0 && p.g->close == 0, "absent stream: its geo");
    CHECK(!m.open && !m.headed && m.have == 0 && m.total == 0 && m.steps == 0 && m.origin == 0 && p.quads == 0, "absent stream: something is carried");
    CHECK(!live_planned(m, false, 0, 100) && !m.open, "absent stream: after the plan");
  }
  {  // a 1-frame piece, then an empty piece of the stream now open
    LiveStream m;
    Piece p;
    p.take(G, m, 1, false);
    CHECK(!p.why && p.in->first == 7 && p.in->fresh == 1 && p.in->frames == 1 && p.in->keep == 1024 && p.in->shift == 0 && p.in->origin == 0 &&
              p.in->eof == LIVE_OPEN && p.in->close == 0,
          "1-frame piece: its LiveIn");
    CHECK(p.g->have == 1025 && p.g->kept == 0 && p.g->c1 == 0 && p.g->c2 == 0 && p.g->n_head == 0 && p.g->fresh == 1 && p.g->close == 0, "1-frame piece: its geo");
    CHECK(p.quads == (1024 + 1 + 6144 + 256 + 3) / 4, "1-frame piece: %ld quads", (long)p.quads);
    CHECK(m.open && !m.headed && m.have == 1025 && m.total == 1 && m.steps == 0, "1-frame piece: the mirror");
    CHECK(!live_planned(m, false, 0, 4096) && m.shift == 0, "1-frame piece: after the plan");
    Piece q;
    q.take(G, m, 0, false);
    CHECK(!q.why && q.in->fresh == 0 && q.in->keep == 1025 && q.in->frames == 0 && q.g->have == 1025 && q.g->fresh == 0 && m.total == 1, "an open stream's empty piece");
  }
  {  // a close on the first piece with fewer than n_head frames: the head runs over `total` frames; the stream reopened is fresh
    LiveStream m;
    Piece p;
    p.take(G, m, 500, true);
    CHECK(!p.why && p.g->n_head == 500 && p.g->have == 1524 && p.g->kept == 0 && p.g->fresh == 1 && p.g->close == 1, "early close: n_head %d have %ld",
          p.g->n_head, (long)p.g->have);
    CHECK(p.g->c1 == 1524 / 64 - 4 && p.g->c2 == (1524 + 6144) / 64 - 4 - p.g->c1, "early close: c1 %ld c2 %ld", (long)p.g->c1, (long)p.g->c2);
    CHECK(p.in->close == 1 && p.in->eof == 1524 && p.in->keep == 1024, "early close: its LiveIn");
    CHECK(!live_planned(m, true, 12345, 0) && !m.open && m.have == 0 && m.total == 0 && m.steps == 0 && m.shift == 0, "early close: the mirror is not reset");
    Piece q;
    q.take(G, m, 10, false);
    CHECK(!q.why && q.in->fresh == 1 && q.in->keep == 1024 && q.in->origin == 0 && q.in->shift == 0 && q.g->have == 1034 && q.g->n_head == 0 && q.g->kept == 0 &&
              m.total == 10 && !m.headed,
          "reopened stream: not fresh");
  }
  {  // the head decision at n_head frames, and a rebase carried into the next piece
    LiveStream m;
    Piece p;
    p.take(G, m, 2400, false);
    CHECK(!p.why && p.g->n_head == 2331 && p.g->have == 3424 && p.g->c1 == 3424 / 64 - 4 && p.g->c2 == 0 && m.steps == 49 && m.headed, "head at n_head: n_head %d c1 %ld",
          p.g->n_head, (long)p.g->c1);
    CHECK(!live_planned(m, false, 640, 4096) && m.shift == 640, "head at n_head: after the plan");
    Piece q;
    q.take(G, m, 10, false);
    CHECK(!q.why && q.in->fresh == 0 && q.in->shift == 640 && q.in->keep == 3424 - 640 && q.in->origin == 640 && q.g->kept == 49 - 10 && q.g->have == 2794 &&
              q.g->n_head == 0 && q.g->c1 == 0 && m.origin == 640 && m.shift == 0 && m.total == 2410,
          "rebased piece: shift %ld keep %ld origin %ld kept %ld c1 %ld", (long)q.in->shift, (long)q.in->keep, (long)q.in->origin, (long)q.g->kept, (long)q.g->c1);
  }
  {  // a piece that makes keep + n + pad + 256 > cs is refused; one that just fits is not
    const LiveShape T(2048, 777, 1024 + 100 + 6144 + 256);
    LiveStream a, b;
    Piece p, q;
    p.take(T, a, 100, false);
    q.take(T, b, 101, false);
    CHECK(!p.why, "a piece that just fits its buffer is refused: %s", p.why);
    CHECK(q.why && strstr(q.why, "exceed its buffer"), "a piece beyond its buffer is not refused");
  }
  {  // a shift outside [0, have], or one that keeps more than the retention bound, is refused
    LiveStream m;
    Piece p;
    p.take(G, m, 3000, false);  // have 4024
    LiveStream a = m, b = m, c = m, d = m, e = m;
    CHECK(live_planned(a, false, -64, 8192) != nullptr, "a negative shift is not refused");
    CHECK(live_planned(b, false, 4025, 8192) != nullptr, "a shift beyond the samples held is not refused");
    CHECK(live_planned(c, false, 4024, 8192) == nullptr && live_planned(d, false, 0, 4024) == nullptr, "a shift at either end of [0, have] is refused");
    const char *why = live_planned(e, false, 0, 4023);
    CHECK(why && strstr(why, "retention bound"), "keeping more than the retention bound is not refused");
  }
}

int main() {
  const long nb = 15, S[7] = {1, 2, 5, 7, nb - 1, nb, nb + 1};
  for (int i = 0; i < 7; i++) slices_case(S[i]);
  slices_out_of_order();
  comment_cases();
  const long shapes[3][2] = {{1, 0}, {1, 1}, {3, 5}};
  for (int i = 0; i < 3; i++) layout_case(shapes[i][0], shapes[i][1]);
  live_cases();
  printf("%d checks: %s\n", g_cases, g_bad ? "FAILED" : "ok");
  return g_bad ? 1 : 0;
}
