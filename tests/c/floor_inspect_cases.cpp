// tests/c/floor_inspect_cases.cpp -- TEST BUILD ONLY (tests/test_floor_inspect_cases.py; built with
// -fsanitize=address,undefined against the one-lane vocabulary of tests/emul).  inspect_error_wave of k_floor.inc, called
// directly on crafted qc[] arrays, against a serial restatement of inspect_error (lib/floor1.c:516-565) written here:
// the line stepped point by point with its running remainder, a return at the first failing point, else the three
// closing tests in the reference's own float expressions.  In this build a chunk of the wave form is one point; the
// 64-lane form is the GPU suite's (tests/test_floor_split_gpu.py).   exit 0 = every case agreed
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "vamd_bind.h"
#include "k_floor.h"

using namespace vamd;

static int g_bad = 0, g_cases = 0, g_ones = 0, g_zeros = 0;

struct Tests {
  float maxover, maxunder, maxerr;
};

// inspect_error as the reference walks it.  qc: bits 0-9 the quantised mask, bit 15 the class "mdct + twofitatten >= mask".
static int serial_inspect(int x0, int x1, int y0, int y1, const unsigned short *qc, const Tests &t, long *failed_at) {
  const int dy = y1 - y0, adx = x1 - x0;
  int ady = abs(dy);
  const int base = dy / adx, sy = dy < 0 ? base - 1 : base + 1;
  int x = x0, y = y0, err = 0, n = 0;
  long mse = 0;
  ady -= abs(base * adx);
  *failed_at = -1;
  for (;;) {
    const int val = qc[x] & 0x7fff;
    mse += (long)(y - val) * (y - val);
    n++;
    if ((qc[x] & 0x8000) && (x == x0 || val)) {
      if ((float)y + t.maxover < (float)val || (float)y - t.maxunder > (float)val) {
        *failed_at = x - x0;
        return 1;
      }
    }
    if (++x >= x1) break;
    err += ady;
    if (err >= adx) {
      err -= adx;
      y += sy;
    } else {
      y += base;
    }
  }
  if (t.maxover * t.maxover / (float)n > t.maxerr) return 0;
  if (t.maxunder * t.maxunder / (float)n > t.maxerr) return 0;
  if ((float)(mse / n) > t.maxerr) return 1;
  return 0;
}

static int line_at(int x0, int x1, int y0, int y1, int k) {  // the y the walk above reaches after k steps
  const int dy = y1 - y0, adx = x1 - x0;
  return y0 + (dy < 0 ? -1 : 1) * (int)((long)k * abs(dy) / adx);
}

struct Harness {
  FloorP F;
  Tests t;
  std::vector<uint32_t> magic;
  explicit Harness(const Tests &tt) : t(tt), magic(derive_div_magic()) {
    memset(&F, 0, sizeof(F));
    F.maxover = t.maxover, F.maxunder = t.maxunder, F.maxerr = t.maxerr;
    F.div_magic = magic.data();
    floor_derive_tests(&F);
  }
  // runs both forms on qc[x0 .. x1) (a heap copy of exactly the points visited, so that the sanitizer sees a read past
  // either end) and compares
  void check(const char *what, int x0, int n, int y0, int y1, const std::vector<unsigned short> &pts, int expect = -1,
             long expect_at = -2) {
    const int x1 = x0 + n;
    const int visited = n > 1 ? n : 1;
    unsigned short *heap = (unsigned short *)malloc(sizeof(unsigned short) * (size_t)visited);
    for (int i = 0; i < visited; i++) heap[i] = pts[(size_t)i];
    const unsigned short *qc = heap - x0;  // qc[x0] is heap[0]
    PhaseClock pc;
    long at = -1;
    const int want = serial_inspect(x0, x1, y0, y1, qc, t, &at);
    const int got = inspect_error_wave(x0, x1, y0, y1, qc, F, pc);
    free(heap);
    g_cases++;
    (want ? g_ones : g_zeros)++;
    if (got != want || (expect >= 0 && want != expect) || (expect_at >= -1 && at != expect_at)) {
      if (g_bad++ < 20)
        printf("  FAILED %s: n %d x0 %d line %d..%d int_tests %d: wave form %d, serial %d (first failing point %ld), expected %d at %ld\n",
               what, n, x0, y0, y1, F.int_tests, got, want, at, expect, expect_at);
    }
  }
};

static const int kRanges[] = {1, 2, 63, 64, 65, 128, 1024};

// points that follow the line at a distance inside both tolerances, class bit on every second one
static std::vector<unsigned short> near_line(int x0, int n, int y0, int y1, int slack) {
  const int visited = n > 1 ? n : 1;
  std::vector<unsigned short> p((size_t)visited);
  for (int k = 0; k < visited; k++) {
    const int y = line_at(x0, x0 + n, y0, y1, k);
    const int d = slack > 0 ? (k * 7 + 3) % (2 * slack + 1) - slack : 0;
    p[(size_t)k] = (unsigned short)((y + d) | ((k & 1) ? 0 : 0x8000));
  }
  return p;
}

static void run_tests(const Tests &tt) {
  Harness h(tt);
  const int over = (int)floorf(tt.maxover) + 1, under = (int)floorf(tt.maxunder) + 1;  // the smallest distances that fail
  const int slack = (over < under ? over : under) - 1;
  const bool counts_idle = h.F.cnt_over == 0 && h.F.cnt_under == 0;  // mse decides at every range
  for (int n : kRanges) {
    const int visited = n > 1 ? n : 1;
    const int lines[3][2] = {{200, 200 + (n > 600 ? 600 : n / 2 + 1)}, {512, 512}, {800, 800 - (n > 600 ? 600 : n / 2 + 1)}};
    for (int x0 : {0, 37}) {
      for (const auto &ln : lines) {
        const int y0 = ln[0], y1 = ln[1];
        // -- the only failing point at the first, the last and an interior place of every chunk of 64
        for (int c0 = 0; c0 < visited; c0 += 64) {
          for (int place : {c0, c0 + 17, (c0 + 63 < visited ? c0 + 63 : visited - 1)}) {
            if (place >= visited) continue;
            for (int dir = 0; dir < 2; dir++) {
              std::vector<unsigned short> p = near_line(x0, n, y0, y1, slack);
              const int y = line_at(x0, x0 + n, y0, y1, place);
              p[(size_t)place] = (unsigned short)((dir ? y - under : y + over) | 0x8000);
              h.check("lone failing point", x0, n, y0, y1, p, 1, place);
              // the same distance, class bit clear: does not count
              p[(size_t)place] &= 0x7fff;
              h.check("class bit clear", x0, n, y0, y1, p, -1, -1);
              // a zero that is not the first point: does not count, however far under the line
              if (place > 0) {
                p[(size_t)place] = 0x8000;
                h.check("zero past the first point", x0, n, y0, y1, p, -1, -1);
              }
            }
          }
        }
        // -- a zero first point counts (class bit set), and does not with the bit clear
        {
          std::vector<unsigned short> p = near_line(x0, n, y0, y1, slack);
          p[0] = 0x8000;
          h.check("zero first point", x0, n, y0, y1, p, 1, 0);
          p[0] = 0;
          h.check("zero first point, class bit clear", x0, n, y0, y1, p, -1, -1);
        }
        // -- no failing point: the walk runs to the end and the closing tests decide
        h.check("near the line", x0, n, y0, y1, near_line(x0, n, y0, y1, slack), -1, -1);
        h.check("on the line", x0, n, y0, y1, near_line(x0, n, y0, y1, 0), 0, -1);
        // -- mse one below, at and one above (floor(maxerr) + 1) * cnt, no failing point, where no count test holds
        if (counts_idle && n >= 63) {
          const long T = ((long)floorf(tt.maxerr) + 1) * visited;
          for (long target : {T - 1, T, T + 1}) {
            std::vector<unsigned short> p = near_line(x0, n, y0, y1, 0);
            long left = target;
            for (int k = 0; k < visited && left > 0; k++) {  // largest squares first, a class-b point each (never point-tested)
              int d = 40;
              while ((long)d * d > left) d--;
              const int y = line_at(x0, x0 + n, y0, y1, k);
              p[(size_t)k] = (unsigned short)(y + ((k & 1) ? d : -d));
              left -= (long)d * d;
            }
            if (left) {
              printf("  FAILED to lay out mse %ld over %d points\n", target, n);
              g_bad++;
              continue;
            }
            h.check("mse at the bound", x0, n, y0, y1, p, target >= T ? 1 : 0, -1);
          }
        }
        // -- a large mse on class-b points: 0 while cnt <= cnt_over or cnt_under, 1 past them
        {
          std::vector<unsigned short> p = near_line(x0, n, y0, y1, 0);
          for (size_t k = 0; k < p.size(); k++) p[k] = (unsigned short)((p[k] & 0x7fff) + 150);
          const bool count_holds = visited <= h.F.cnt_over || visited <= h.F.cnt_under;
          h.check("large mse against the count tests", x0, n, y0, y1, p, count_holds ? 0 : 1, -1);
        }
      }
    }
  }
}

int main() {
  // the integer form of the point tests (maxover / maxunder whole numbers, as the shipped setups have them) with an
  // maxerr under which no count test ever holds (the mse decides) and one under which they hold up to 127 points; the
  // float form (values that are no multiple of 2^-13) likewise; a tolerance of zero on one side
  const Tests sets[] = {{8.f, 8.f, 100.f}, {8.f, 12.f, 0.5f}, {7.3f, 5.7f, 60.f}, {7.3f, 5.7f, 0.5f}, {0.f, 3.f, 20.f}};
  const int want_int[] = {1, 1, 0, 0, 1};
  for (size_t i = 0; i < sizeof(sets) / sizeof(sets[0]); i++) {
    Harness h(sets[i]);
    if (h.F.int_tests != want_int[i]) {
      printf("  FAILED: set %zu takes int_tests %d\n", i, h.F.int_tests);
      g_bad++;
    }
    run_tests(sets[i]);
  }
  printf("%d cases (%d return 1, %d return 0): %s\n", g_cases, g_ones, g_zeros, g_bad ? "FAILED" : "ok");
  return g_bad ? 1 : 0;
}
