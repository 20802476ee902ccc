// tests/c/chase_regs_cases.cpp -- TEST BUILD ONLY (tests/test_chase_regs_cases.py; built with
// -fsanitize=address,undefined against the one-lane vocabulary of tests/emul).  tone_chase_regs<8> of k_tone.h -- the
// stack walk with its window as a bit mask and seven values, no ring -- against a plain walk written here (seed_chase's
// stack discipline, lib/psy.c:454-487, on a list that simply grows) and against tone_chase_ring<8>: the survivor list,
// the count, and that nothing is written past the count (the ring walk writes nothing there either) nor past the row.
// Rows and survivor lists are heap blocks of exactly the padded sizes, so a step outside is the sanitizer's to report.
//   exit 0 = every case agreed
//   chase_regs_cases census FILE: FILE holds rows of seed lines (int32 rows, int32 lines, then rows x lines floats);
//   prints the pops per line of the walk, per row and as the slowest of each 64 consecutive rows (the lanes of a wave)
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "vamd_bind.h"
#include "k_tone.h"

using namespace vamd;

static long g_bad = 0, g_cases = 0;

// the walk on an unbounded stack; returns the surviving lines, ascending.  pops_out (optional): pops at each line
static int plain_walk(const float *v, int linesper, int n, int *pos_out, int *pops_out = nullptr) {
  std::vector<int> pos;
  std::vector<float> amp;
  pos.reserve(n), amp.reserve(n);
  for (int i = 0; i < n; i++) {
    int pops = 0;
    for (;;) {
      const size_t d = pos.size();
      if (d < 2) break;
      const bool below = v[i] < amp[d - 1];
      const bool near_top = i < pos[d - 1] + linesper, near_under = i < pos[d - 2] + linesper;
      if (below || !near_top || !(amp[d - 1] <= amp[d - 2]) || !near_under) break;
      pos.pop_back(), amp.pop_back(), pops++;
    }
    pos.push_back(i), amp.push_back(v[i]);
    if (pops_out) pops_out[i] = pops;
  }
  for (size_t k = 0; k < pos.size(); k++) pos_out[k] = pos[k];
  return (int)pos.size();
}

// a row in whole 32-line pieces (it is read a cache line at a time), survivor lists of the same padded length
struct Bufs {
  float *row;
  float *ring_amp;
  int *ring_pos;
  unsigned short *surv, *surv_ring;
  int nlp;
  explicit Bufs(int n) {
    nlp = VAMD_LINES_PAD(n);
    row = (float *)aligned_alloc(16, (size_t)nlp * 4);
    ring_amp = (float *)aligned_alloc(16, 8 * 4);
    ring_pos = (int *)aligned_alloc(16, 8 * 4);
    surv = (unsigned short *)aligned_alloc(16, (size_t)nlp * 2);
    surv_ring = (unsigned short *)aligned_alloc(16, (size_t)nlp * 2);
    for (int i = 0; i < nlp; i++) row[i] = VAMD_NEGINF;
  }
  ~Bufs() { free(row), free(ring_amp), free(ring_pos), free(surv), free(surv_ring); }
};

static void check(Bufs &B, int n, const char *what, long id) {
  static std::vector<int> want;
  if ((int)want.size() < n) want.resize(n);
  const unsigned short sentinel = 0xa5a5;
  for (int k = 0; k < B.nlp; k++) B.surv[k] = B.surv_ring[k] = sentinel;
  const int nw = plain_walk(B.row, 8, n, want.data());
  const int ng = tone_chase_regs<8>(B.row, n, B.surv);
  const int nr = tone_chase_ring<8>(B.row, 8, n, B.ring_amp, B.ring_pos, 1, 0, B.surv_ring);
  bool bad = ng != nw || nr != nw;
  for (int k = 0; !bad && k < nw; k++) bad = B.surv[k] != want[k];
  for (int k = nw; !bad && k < B.nlp; k++) bad = B.surv[k] != sentinel;  // nothing beyond the count
  bad = bad || memcmp(B.surv, B.surv_ring, (size_t)B.nlp * 2) != 0;      // byte for byte the ring walk's
  g_cases++;
  if (bad && g_bad++ < 8) printf("MISMATCH n %d %s #%ld: %d survivors, the ring walk %d, want %d\n", n, what, id, ng, nr, nw);
}

static uint32_t g_rng = 0x9e3779b9u;
static uint32_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 17, g_rng ^= g_rng << 5;
  return g_rng;
}

// one seeded random row: few levels (many ties) on odd ids, no ties on even ones; every eighth id mixes in stretches of
// VAMD_NEGINF
static void fill_random(float *row, int n, long id) {
  for (int i = 0; i < n; i++) row[i] = (id & 1) ? (float)(rnd() % (2 + id % 7)) : (float)(rnd() % 100000) * 0.001f;
  if (id % 8 == 7)
    for (int i = 0; i < n;) {
      const int gap = rnd() % 50, len = 1 + rnd() % 12;
      for (int k = 0; k < gap && i < n; k++, i++) row[i] = VAMD_NEGINF;
      i += len;
    }
}

static int census(const char *path) {
  FILE *f = fopen(path, "rb");
  int32_t hdr[2];
  if (!f || fread(hdr, 4, 2, f) != 2 || hdr[0] <= 0 || hdr[1] <= 0 || hdr[1] > 4096) return printf("census: cannot read %s\n", path), 1;
  const int rows = hdr[0], n = hdr[1];
  std::vector<float> row(n);
  std::vector<int> pos(n), pops(n), worst(n, 0);
  long lane_pops = 0, wave_pops = 0, wave_lines = 0, hist[8] = {0}, whist[8] = {0}, surv = 0;
  auto close_wave = [&]() {
    for (int i = 0; i < n; i++) wave_pops += worst[i], whist[worst[i] < 7 ? worst[i] : 7]++, worst[i] = 0;
    wave_lines += n;
  };
  for (int r = 0; r < rows; r++) {
    if (fread(row.data(), 4, (size_t)n, f) != (size_t)n) return printf("census: short file\n"), 1;
    surv += plain_walk(row.data(), 8, n, pos.data(), pops.data());
    for (int i = 0; i < n; i++) {
      lane_pops += pops[i], hist[pops[i] < 7 ? pops[i] : 7]++;
      if (pops[i] > worst[i]) worst[i] = pops[i];
    }
    if (r % 64 == 63 || r == rows - 1) close_wave();
  }
  fclose(f);
  printf("census: %d rows of %d lines, %.1f survivors a row\n", rows, n, (double)surv / rows);
  printf("  pops per line, a lane on its own : %.4f   lines with 0..6 pops:", (double)lane_pops / ((double)rows * n));
  for (int k = 0; k < 7; k++) printf(" %ld", hist[k]);
  printf("\n  pops per line, slowest of 64     : %.4f   lines with 0..6 pops:", (double)wave_pops / (double)wave_lines);
  for (int k = 0; k < 7; k++) printf(" %ld", whist[k]);
  printf("\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "census")) return census(argv[2]);
  // ---- every sequence of 14 lines over three values
  {
    const int n = 14;
    Bufs b(n);
    long total = 1;
    for (int k = 0; k < n; k++) total *= 3;
    for (long c = 0; c < total; c++) {
      long r = c;
      for (int k = 0; k < n; k++, r /= 3) b.row[k] = (float)(r % 3);
      check(b, n, "exhaustive", c);
    }
    printf("exhaustive: %ld sequences of %d lines over three values: %ld mismatches\n", total, n, g_bad);
  }
  // ---- seeded random rows of the two line counts the setups have, and of every length from 1 to 40 (the `i < n` edge inside
  // a trip of 32 lines; fewer lines than the window)
  {
    const int ns[2] = {777, 585};
    for (int which = 0; which < 2; which++) {
      Bufs b(ns[which]);
      for (long id = 0; id < 400; id++) fill_random(b.row, ns[which], id), check(b, ns[which], "random", id);
    }
    for (int n = 1; n <= 40; n++) {
      Bufs b(n);
      for (long id = 0; id < 64; id++) fill_random(b.row, n, id), check(b, n, "short random", id);
    }
    printf("random: rows of 777, 585 and 1..40 lines: %ld cases so far, %ld mismatches\n", g_cases, g_bad);
  }
  // ---- shapes
  const int ns[4] = {777, 585, 40, 7};
  for (int which = 0; which < 4; which++) {
    const int n = ns[which];
    Bufs b(n);
    for (int i = 0; i < n; i++) b.row[i] = VAMD_NEGINF;  // the silent block: all lines equal
    check(b, n, "all equal", 0);
    for (int i = 0; i < n; i++) b.row[i] = (float)i * 0.25f - 90.f;  // strictly rising
    check(b, n, "rising", 0);
    for (int i = 0; i < n; i++) b.row[i] = 90.f - (float)i * 0.25f;  // strictly falling
    check(b, n, "falling", 0);
    // sawteeth: a fall of period-1 lines, then a line above all of them.  Period 8: the pops reach exactly to the window's
    // edge; 9: one line of the fall is out of reach; 7: one short of the edge.  Both with the jump above the previous
    // tooth's top and below it, and with a flat fall (ties).
    for (int period = 7; period <= 9; period++)
      for (int form = 0; form < 4; form++) {
        for (int i = 0; i < n; i++) {
          const int ph = i % period, tooth = i / period;
          const float top = (form & 1) ? 50.f + (float)tooth : 50.f - (float)tooth * 0.5f;
          b.row[i] = ph == 0 ? top : ((form & 2) ? top - 10.f : top - 10.f - (float)ph);
        }
        check(b, n, "sawtooth", period * 10 + form);
        for (int i = 0; i < n; i++) b.row[i] = -b.row[i];  // rises of period-1 lines, then a drop
        check(b, n, "inverted sawtooth", period * 10 + form);
      }
  }
  printf("chase_regs_cases: %ld cases, %ld mismatches: %s\n", g_cases, g_bad, g_bad ? "FAILED" : "ok");
  return g_bad ? 1 : 0;
}
