// tests/c/tone_fold_groups.cpp -- TEST BUILD ONLY (tests/test_tone_fold_groups_cpu.py; built with
// -fsanitize=address,undefined).  The per-group tables of vamd_derive.h (group_p0, bin_group, line_slot, and
// line_group beside them) held against max_seeds' own walk (lib/psy.c:512-545), replayed here from the blob's octave[]
// without a look at derive_psy's loop.   usage: tone_fold_groups setup.bin...   exit 0 = every check of every look held
#include <stdio.h>
#include <string.h>
#include <vector>
#include "vamd_derive.h"

using namespace vamd;

static int g_bad = 0;
#define REQUIRE(cond, ...)                                  \
  do {                                                      \
    if (!(cond)) {                                          \
      if (g_bad++ < 20) {                                   \
        printf("  FAILED %s: ", #cond), printf(__VA_ARGS__), printf("\n"); \
      }                                                     \
    }                                                       \
  } while (0)

static void check_look(const vamd_psy_tab &t, const unsigned char *blob, const char *what) {
  const PsyDerived d = derive_psy(t, blob);
  const int n = t.n, nl = t.total_octave_lines;
  const int32_t *octave = (const int32_t *)(blob + t.off_octave);
  REQUIRE((int)d.group_p0.size() == d.ngroups + 1, "%s: %zu entries for %d groups", what, d.group_p0.size(), d.ngroups);
  REQUIRE((int)d.bin_group.size() == ((n + 7) & ~7), "%s: bin_group holds %zu", what, d.bin_group.size());
  REQUIRE((int)d.line_slot.size() == ((nl + 15) & ~15) && d.line_slot.size() == d.line_group.size(), "%s: line_slot holds %zu",
          what, d.line_slot.size());
  REQUIRE(d.ngroups < 0xffff, "%s: %d groups do not fit 16 bits", what, d.ngroups);
  if (g_bad) return;
  std::vector<int> owner((size_t)nl, -1);  // the group whose scan covers a line, from the walk
  // the walk, as the reference writes it
  const int linesper = t.eighth_octave_lines;
  long linpos = 0, pos = octave[0] - t.firstoc - (linesper >> 1);
  int g = 0;
  long last_end = -1;  // the last line the groups so far have scanned
  while (linpos + 1 < n) {
    const long p0 = pos;  // minV = seeds[pos]
    long end = ((octave[linpos] + octave[linpos + 1]) >> 1) - t.firstoc;
    while (pos + 1 <= end) pos++;  // lines p0 + 1 .. pos are scanned
    end = pos + t.firstoc;
    REQUIRE(g < d.ngroups, "%s: the walk has more than %d groups", what, d.ngroups);
    if (g >= d.ngroups) return;
    REQUIRE(p0 >= 0 && pos < nl, "%s: group %d scans (%ld, %ld] outside the %d lines", what, g, p0, pos, nl);
    REQUIRE(d.group_p0[(size_t)g] == p0, "%s: group %d starts from line %d, the walk from %ld", what, g, d.group_p0[(size_t)g], p0);
    REQUIRE(p0 >= last_end, "%s: group %d starts at line %ld, inside the lines scanned before (to %ld)", what, g, p0, last_end);
    for (long p = p0 + 1; p <= pos && p < nl; p++) owner[(size_t)p] = g;
    if (pos > p0) last_end = pos;
    int nbins = 0;
    for (; linpos < n && octave[linpos] <= end; linpos++, nbins++) {
      const int bg = d.bin_group[(size_t)linpos];
      REQUIRE(bg == g, "%s: bin %ld is in group %d, the walk has it in %d", what, linpos, bg, g);
      REQUIRE(bg < d.ngroups && d.group_p0[(size_t)bg] == p0, "%s: bin %ld reads line %d, the walk line %ld", what, linpos,
              bg <= d.ngroups ? d.group_p0[(size_t)bg] : -1, p0);
      REQUIRE((d.bin_fold[(size_t)linpos] & 0xffff) == p0 && (d.bin_fold[(size_t)linpos] >> 16) == g, "%s: bin_fold[%ld]", what, linpos);
    }
    REQUIRE(nbins >= 1, "%s: group %d has no bin", what, g);
    g++;
  }
  REQUIRE(g == d.ngroups, "%s: %d groups derived, the walk has %d", what, d.ngroups, g);
  REQUIRE(linpos == d.tail_linpos, "%s: the tail begins at bin %d, the walk's at %ld", what, d.tail_linpos, linpos);
  // the tail loop: minV = seeds[p->total_octave_lines - 1] for every bin that is left
  REQUIRE(d.group_p0[(size_t)d.ngroups] == nl - 1, "%s: the tail group reads line %d of %d", what, d.group_p0[(size_t)d.ngroups], nl);
  for (size_t b = (size_t)linpos; b < d.bin_group.size(); b++)
    REQUIRE(d.bin_group[b] == d.ngroups, "%s: tail bin %zu is in group %d, not in the tail group %d", what, b, d.bin_group[b], d.ngroups);
  // the lines: line_group / line_slot agree with the groups' ranges; a group's lines are one ascending run
  int prev = -1;
  for (size_t p = 0; p < d.line_slot.size(); p++) {
    const int own = p < (size_t)nl ? owner[p] : -1;
    REQUIRE(d.line_group[p] == (own < 0 ? 0xffff : own), "%s: line %zu is group %d's, line_group says %d", what, p, own, d.line_group[p]);
    REQUIRE(d.line_slot[p] == 4 * (own < 0 ? d.ngroups : own), "%s: line %zu is group %d's, line_slot says %d", what, p, own, d.line_slot[p]);
    if (own >= 0) {
      REQUIRE(own >= prev, "%s: line %zu belongs to group %d after group %d", what, p, own, prev);
      prev = own;
    }
  }
}

int main(int argc, char **argv) {
  for (int a = 1; a < argc; a++) {
    FILE *f = fopen(argv[a], "rb");
    if (!f) {
      printf("cannot open %s\n", argv[a]);
      return 2;
    }
    std::vector<unsigned char> blob;
    unsigned char buf[65536];
    for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) blob.insert(blob.end(), buf, buf + k);
    fclose(f);
    if (blob.size() < sizeof(vamd_setup_header)) {
      printf("%s: truncated\n", argv[a]);
      return 2;
    }
    vamd_setup_header h;
    memcpy(&h, blob.data(), sizeof(h));
    for (int p = 0; p < 4; p++) {
      char what[512];
      snprintf(what, sizeof(what), "%s psy %d", argv[a], p);
      check_look(h.psy[p], blob.data(), what);
    }
    printf("%s: %s\n", argv[a], g_bad ? "FAILED" : "ok");
  }
  return g_bad ? 1 : 0;
}
