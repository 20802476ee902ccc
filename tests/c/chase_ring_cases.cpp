// tests/c/chase_ring_cases.cpp -- TEST BUILD ONLY (tests/test_chase_ring_cases.py; built with
// -fsanitize=address,undefined against the one-lane vocabulary of tests/emul).  tone_chase_ring of k_tone.h with a ring of
// 8 and of 16 slots against a plain walk written here: seed_chase's stack discipline (lib/psy.c:454-487) on a stack
// that simply grows -- a line is pushed after the entries it makes irrelevant have been taken off, and an entry comes
// off while the line is not below it, it is not above the entry under it, and the line is within `linesper` of both.
// The library is compiled here with VAMD_CHASE_GUARD=1: the read-back of the second-from-top entry tests whether its slot
// has been reused and counts when it has (k_tone.h argues that it never has for linesper <= ring).
//   exit 0 = every case agreed and the guard never decided a step
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
static long g_guard_hits = 0;
#define VAMD_CHASE_GUARD 1
#define VAMD_CHASE_GUARD_HIT() (++g_guard_hits)
#include "vamd_bind.h"
#include "k_tone.h"

using namespace vamd;

static long g_bad = 0, g_cases = 0;

// the walk on an unbounded stack; returns the surviving lines, ascending
static int plain_walk(const float *v, int linesper, int n, int *pos_out) {
  std::vector<int> pos;
  std::vector<float> amp;
  pos.reserve(n), amp.reserve(n);
  for (int i = 0; i < n; i++) {
    for (;;) {
      const size_t d = pos.size();
      if (d < 2) break;
      const bool below = v[i] < amp[d - 1];
      const bool near_top = i < pos[d - 1] + linesper, near_under = i < pos[d - 2] + linesper;
      if (below || !near_top || !(amp[d - 1] <= amp[d - 2]) || !near_under) break;
      pos.pop_back(), amp.pop_back();
    }
    pos.push_back(i), amp.push_back(v[i]);
  }
  for (size_t k = 0; k < pos.size(); k++) pos_out[k] = pos[k];
  return (int)pos.size();
}

// buffers of exactly the sizes the walk may touch: the row in whole 32-line pieces (it is read a cache line at a time),
// rings of `ring` slots at `rstride`, survivors in whole stores of eight
struct Bufs {
  float *row;
  float *ring_amp;
  int *ring_pos;
  unsigned short *surv;
  int nring;
  Bufs(int n, int ring, int rstride) {
    const int nlp = VAMD_LINES_PAD(n);
    nring = ring * rstride;
    row = (float *)aligned_alloc(16, (size_t)nlp * 4);
    ring_amp = (float *)aligned_alloc(16, (size_t)nring * 4);
    ring_pos = (int *)aligned_alloc(16, (size_t)nring * 4);
    surv = (unsigned short *)aligned_alloc(16, (size_t)nlp * 2);
    for (int i = 0; i < nlp; i++) row[i] = VAMD_NEGINF;
  }
  ~Bufs() { free(row), free(ring_amp), free(ring_pos), free(surv); }
};

template <int RING>
static void check(Bufs &B, int linesper, int n, int rstride, int rlane, const char *what, long id) {
  static std::vector<int> want;
  if ((int)want.size() < n) want.resize(n);
  const float sent_a = 12345.f;
  const int sent_p = -77;
  if (rstride > 1)
    for (int k = 0; k < B.nring; k++) B.ring_amp[k] = sent_a, B.ring_pos[k] = sent_p;
  const int nw = plain_walk(B.row, linesper, n, want.data());
  const int ng = tone_chase_ring<RING>(B.row, linesper, n, B.ring_amp, B.ring_pos, rstride, rlane, B.surv);
  bool bad = ng != nw;
  for (int k = 0; !bad && k < nw; k++) bad = B.surv[k] != want[k];
  if (rstride > 1)  // a lane keeps to its own column of [slot][lane]
    for (int k = 0; !bad && k < B.nring; k++) bad = k % rstride != rlane && (B.ring_amp[k] != sent_a || B.ring_pos[k] != sent_p);
  g_cases++;
  if (bad && g_bad++ < 8) printf("MISMATCH ring %d linesper %d n %d stride %d lane %d %s #%ld: %d survivors, want %d\n", RING, linesper, n, rstride, rlane, what, id, ng, nw);
}

static uint32_t g_rng = 0x2545f491u;
static uint32_t rnd() {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 17, g_rng ^= g_rng << 5;
  return g_rng;
}

// one seeded row of n lines, kind by kind
static void fill(float *row, int n, int kind, long id) {
  int i = 0;
  switch (kind) {
    case 0:  // random values, many ties (few levels) or none
      for (; i < n; i++) row[i] = (id & 1) ? (float)(rnd() % (2 + id % 7)) : (float)(rnd() % 100000) * 0.001f;
      break;
    case 1:  // descending staircases of random length, each followed by a rise of random height
      while (i < n) {
        const int len = 1 + rnd() % 30;
        float a = (float)(rnd() % 50);
        for (int k = 0; k < len && i < n; k++, i++) row[i] = a, a -= (float)(rnd() % 3);
      }
      break;
    case 2:  // ascending staircases
      while (i < n) {
        const int len = 1 + rnd() % 30;
        float a = (float)(rnd() % 50) - 60.f;
        for (int k = 0; k < len && i < n; k++, i++) row[i] = a, a += (float)(rnd() % 3);
      }
      break;
    case 3:  // plateaus of 1 to 40 equal values
      while (i < n) {
        const int len = 1 + rnd() % 40;
        const float a = (float)(rnd() % 9);
        for (int k = 0; k < len && i < n; k++, i++) row[i] = a;
      }
      break;
    case 4:  // stretches no curve reached between short real ones
      while (i < n) {
        const int gap = rnd() % 50, len = 1 + rnd() % 12;
        for (int k = 0; k < gap && i < n; k++, i++) row[i] = VAMD_NEGINF;
        for (int k = 0; k < len && i < n; k++, i++) row[i] = (float)(rnd() % 40) - 20.f;
      }
      break;
    default:  // the stack driven up, then taken down on consecutive lines, as deep as the windows allow: a long descent
              // (every line pushes; runs of equal values in two rows of three), then lines that each exceed a few of the
              // entries left, or all of them
      while (i < n) {
        const int down = 9 + rnd() % 40, up = 1 + rnd() % 9, step = id % 3;
        float a = 1000.f;
        for (int k = 0; k < down && i < n; k++, i++) row[i] = a, a -= (k % (1 + step)) ? 0.f : 1.f;
        for (int k = 0; k < up && i < n; k++, i++) row[i] = a + ((rnd() & 3) ? (float)(rnd() % 10) : 2000.f);  // (2000: above every entry)
      }
      break;
  }
}

int main() {
  // ---- every sequence of 14 lines over three values, eight lines per window (-DCHASE_CASES_SEEDED_ONLY: left to the build
  // of the other setting of VAMD_CHASE_PREFETCH, which differs in how a row is fetched, not in the walk)
#ifndef CHASE_CASES_SEEDED_ONLY
  {
    const int n = 14, lp = 8;
    Bufs b8(n, 8, 1), b16(n, 16, 1);
    long total = 1;
    for (int k = 0; k < n; k++) total *= 3;
    for (long c = 0; c < total; c++) {
      long r = c;
      for (int k = 0; k < n; k++, r /= 3) b8.row[k] = b16.row[k] = (float)(r % 3);
      check<8>(b8, lp, n, 1, 0, "exhaustive", c);
      check<16>(b16, lp, n, 1, 0, "exhaustive", c);
    }
    printf("exhaustive: %ld sequences of %d lines over three values, rings of 8 and 16: %ld mismatches, guard hits %ld\n", total, n, g_bad, g_guard_hits);
  }
#endif
  // ---- seeded rows of the two line counts the setups have (777: long blocks, 585: short)
  const int ns[2] = {777, 585};
  long deepest = 0;
  for (int which = 0; which < 2; which++) {
    const int n = ns[which];
    Bufs b8(n, 8, 1), b16(n, 16, 1), s8(n, 8, 64), s16(n, 16, 64);
    for (int kind = 0; kind < 6; kind++)
      for (long id = 0; id < 400; id++) {
        fill(b8.row, n, kind, id);
        memcpy(b16.row, b8.row, (size_t)n * 4), memcpy(s8.row, b8.row, (size_t)n * 4), memcpy(s16.row, b8.row, (size_t)n * 4);
        check<8>(b8, 8, n, 1, 0, "seeded", kind * 1000 + id);
        check<16>(b16, 8, n, 1, 0, "seeded", kind * 1000 + id);
        if (id < 40) {
          // [slot][lane] at the kernel's stride, first and last lane
          check<8>(s8, 8, n, 64, 0, "stride 64", kind * 1000 + id);
          check<8>(s8, 8, n, 64, 63, "stride 64", kind * 1000 + id);
          check<16>(s16, 8, n, 64, 0, "stride 64", kind * 1000 + id);
          check<16>(s16, 8, n, 64, 63, "stride 64", kind * 1000 + id);
          // shorter windows on eight slots, longer ones (which keep sixteen), and the choice tone_chase_thread makes itself
          for (int lp = 1; lp <= 7; lp += 2) check<8>(b8, lp, n, 1, 0, "short windows", kind * 1000 + id);
          for (int lp = 9; lp <= 16; lp += 7) check<16>(b16, lp, n, 1, 0, "long windows", kind * 1000 + id);
          for (int lp = 7; lp <= 9; lp++) {
            std::vector<int> want(n);
            const int nw = plain_walk(b16.row, lp, n, want.data());
            const int ng = tone_chase_thread(b16.row, lp, n, b16.ring_amp, b16.ring_pos, 1, 0, b16.surv);
            bool bad = ng != nw;
            for (int k = 0; !bad && k < nw; k++) bad = b16.surv[k] != want[k];
            g_cases++;
            if (bad && g_bad++ < 8) printf("MISMATCH tone_chase_thread linesper %d n %d #%ld\n", lp, n, kind * 1000 + id);
          }
        }
        if (kind == 5) {  // how deep a single line took the stack down in the rows built for it
          std::vector<int> pos;
          std::vector<float> amp;
          for (int i = 0; i < n; i++) {
            long pops = 0;
            while (pos.size() >= 2 && !(b8.row[i] < amp.back()) && i < pos.back() + 8 && amp.back() <= amp[amp.size() - 2] && i < pos[pos.size() - 2] + 8)
              pos.pop_back(), amp.pop_back(), pops++;
            pos.push_back(i), amp.push_back(b8.row[i]);
            if (pops > deepest) deepest = pops;
          }
        }
      }
  }
  printf("seeded: rows of 777 and 585 lines, six kinds x 400, rings of 8 and 16, stride 64 lanes 0 and 63: %ld cases so far, %ld mismatches\n", g_cases, g_bad);
  printf("deepest take-down on one line in the rows built for it: %ld entries (6 is the most eight-line windows allow)\n", deepest);
  const long hits = g_guard_hits;
  printf("guard: decided %ld steps over everything above\n", hits);
  // ---- the counter is alive: sixteen-line windows on eight slots (a combination the library never runs) do reuse slots
  {
    const int n = 777;
    Bufs b8(n, 8, 1);
    for (long id = 0; id < 40; id++) {
      fill(b8.row, n, 5, id);
      (void)tone_chase_ring<8>(b8.row, 16, n, b8.ring_amp, b8.ring_pos, 1, 0, b8.surv);
    }
    printf("guard, windows of 16 lines on 8 slots (not a supported pair; the counter's own check): %ld\n", g_guard_hits - hits);
    if (g_guard_hits == hits) g_bad++, printf("the guard's counter never moved where it must\n");
  }
  if (deepest < 6) g_bad++, printf("no line took the stack down 6 deep\n");
  if (hits != 0) g_bad++, printf("the guard decided a step with linesper <= ring: k_tone.h's argument is wrong\n");
  printf("chase_ring_cases: %ld cases, %ld mismatches, guard %s: %s\n", g_cases, g_bad,
         hits == 0 ? "never decided a step (unreachable, as k_tone.h argues; the library is built without it)" : "DECIDED STEPS", g_bad ? "FAILED" : "ok");
  return g_bad ? 1 : 0;
}
