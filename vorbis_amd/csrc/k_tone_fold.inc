// k_tone_fold.inc -- the tone chain's last step (seed_chase's paint, lib/psy.c:489-503, and max_seeds' fold, :512-545) as
// the floor stage takes it with it.  No include guard, no namespace of its own: included by k_tone.h inside namespace vamd
// (the wave vocabulary) and once more by k_floor.h inside vamd::pair (two channel-blocks per wave, vamd_wave_pair.h).
struct SurvHead {
  int p1, np1, p2, np2;  // entries LANE, LANE + 1, LANE + NLANES, LANE + NLANES + 1, whatever the list's length
};
// (a block's list row is nlines entries long whatever the count, so reading past the count stays in the row: callers
// keep two chunks + 1 entries readable)
VAMD_DEV SurvHead surv_head_load(const unsigned short *__restrict__ posstack) {
  SurvHead h;
  h.p1 = posstack[LANE], h.np1 = posstack[LANE + 1];
  h.p2 = posstack[LANE + NLANES], h.np2 = posstack[LANE + NLANES + 1];
  return h;
}
VAMD_DEV void seed_chase_paint(float *seeds, const float *src, int linesper, int n, int stack,
                               const unsigned short *__restrict__ posstack, const SurvHead *head = nullptr) {
  int carry = 0;
  // Software pipeline over the chunks of 64 survivors: the list entries are fetched two chunks ahead and the
  // amplitudes they point at one chunk ahead, so that a chunk finds both in registers.
  auto at = [&](int k) { return k < stack ? (int)posstack[k] : 0; };
  int pos1, npos1, pos2, npos2;
  if (head) {
    pos1 = LANE < stack ? head->p1 : 0, npos1 = LANE + 1 < stack ? head->np1 : 0;
    pos2 = LANE + NLANES < stack ? head->p2 : 0, npos2 = LANE + NLANES + 1 < stack ? head->np2 : 0;
  } else {
    pos1 = at(LANE), npos1 = at(LANE + 1);                    // chunk 0
    pos2 = at(LANE + NLANES), npos2 = at(LANE + NLANES + 1);  // chunk 1
  }
  float a1 = src[pos1], an1 = src[npos1];
  for (int base = 0; base < stack; base += NLANES) {
    const int k = base + LANE;
    const int pos = pos1, npos = npos1;
    const float a = a1, an = an1;
    pos1 = pos2, npos1 = npos2;
    a1 = src[pos1], an1 = src[npos1];
    pos2 = at(k + 2 * NLANES), npos2 = at(k + 2 * NLANES + 1);
    int endpos = 0;
    if (k < stack) {
      endpos = pos + linesper + 1;
      if (k < stack - 1 && an > a) endpos = npos;
      if (endpos > n) endpos = n;
    }
    const int incl = wave_scan_max(endpos);
    int start = wave_shift_up1(incl, 0);
    if (start < carry) start = carry;
    // (a wave's LDS accesses keep their order: the next chunk's amplitudes, asked for above, are read before this
    // chunk's paint lands)
    if (k < stack)
      for (int p = start; p < endpos; p++) seeds[p] = a;
    const int last = wave_last(incl);
    if (last > carry) carry = last;
  }
}

// paint + fold half: seed[] (LDS, unpainted on entry), its unpainted HBM copy, the survivor
// list -> tone curve
// ... in two steps, so that a caller can take the curve quad by quad (k_floor mixes it without a trip through memory):
// tone_fold_prepare leaves the painted lines and the groups' minima in LDS, tone_fold_quad forms four bins from them.
//
// max_seeds' fold, lib/psy.c:522-543.  Each outer-loop iteration ("group") of the reference starts from seed[p0]
// (capped at tone_abs_limit) and then keeps the lowest real (> NEGINF) value among the lines it scans -- a min, hence
// order-free -- and every bin the iteration covers takes that value.  Static tables (vamd_derive.h):
//   line_slot[line]  the group whose scan covers the line (`ngroups` where none does), as a byte offset into gmin[]
//   bin_fold[bin]    p0 | group << 16 (bins below tail_linpos; the bins of the tail loop, :539-543, take seed[nlines - 1])
// (group_p0, bin_group and line_group, which the setup image also holds, are read by no kernel.)
// gmin[ngroups + 1] (LDS): the groups' scanned minima; slot `ngroups` takes the lines that no group scans.
// A lane takes TONE_RUN_LINES consecutive lines, reduces them in registers and sends one LDS float min per group its run
// touches (a group's lines are one run, so a change of group ends a segment).  With one line a lane, a group of the low
// octaves -- up to 101 lines -- has all 64 lanes of an instruction hit one or two addresses, which the LDS unit takes one
// after the other.  No test for a line without a group: its slot is nobody's.  (profiles/r17_tone_fold_groups.txt; DESIGN.md
// "Decided variants" for the forms this one was measured against.)
VAMD_DEV void tone_group_minima(const PsyP &P, const float *seed, float *gmin) {
  constexpr int R = TONE_RUN_LINES;
  static_assert(R == 4 || R == 8, "a run is one or two 16-byte LDS reads");
  const float inf = f_from_bits(0x7f800000u);
  const int nruns = (P.total_octave_lines + R - 1) / R;  // (seed[] and line_slot[] are padded to whole runs)
  // (two trips of the loop at 777 lines: not unrolled, eight ends of a segment are code enough)
  VAMD_TF_RUN_LOOP for (int r = LANE; r < nruns; r += NLANES) {
    float s[R];
    int g[R];  // the lines' slots as byte offsets into gmin[]
    f4_get(((const F4 *)seed)[(R / 4) * r], s);
    const I4 w0 = dm_load_i4(P.line_slot, (unsigned)r * (4u * R));
    g[0] = w0.x, g[1] = w0.y, g[2] = w0.z, g[3] = w0.w;
    if (R == 8) {
      f4_get(((const F4 *)seed)[2 * r + 1], s + R - 4);
      const I4 w1 = dm_load_i4(P.line_slot, (unsigned)r * (4u * R) + 16u);
      g[R - 4] = w1.x, g[R - 3] = w1.y, g[R - 2] = w1.z, g[R - 1] = w1.w;
    }
    float acc = inf;
#pragma unroll
    for (int c = 0; c < R; c++) {
      const float v = s[c] > VAMD_NEGINF ? s[c] : inf;
      acc = c == 0 ? v : tone_min(acc, v);
      if (c == R - 1 || g[c] != g[c + 1]) {  // the last of this group's lines in the run (+inf: nothing real, a no-op)
        lds_atomic_min((float *)((char *)gmin + g[c]), acc);
        acc = inf;
      }
    }
  }
}
VAMD_DEV void tone_fold_prepare(const PsyP &P, float *seed, const float *seed_src,
                                const unsigned short *__restrict__ surv, int nsurv, float *gmin /* LDS [ngroups + 1] */,
                                PhaseClock &pc, int slot = 3, const SurvHead *head = nullptr) {
  const int nlines = P.total_octave_lines;
  seed_chase_paint(seed, seed_src, P.eighth_octave_lines, nlines, nsurv, surv, head);
  WAVE_SYNC();
  pc.mark(slot);

  // the groups' minima: work is balanced over lines instead of leaving the few low bins with 70-line spans to
  // single lanes
  WAVE_FOR(g, P.ngroups + 1) gmin[g] = f_from_bits(0x7f800000u);  // +inf = "no real value scanned"
  WAVE_SYNC();
  tone_group_minima(P, seed, gmin);
  WAVE_SYNC();
  pc.mark(slot + 1);
}
VAMD_DEV float tone_ath_att(const PsyP &P, float local_ampmax) {
  float att = local_ampmax + P.ath_adjatt;
  return att < P.ath_maxatt ? P.ath_maxatt : att;
}
VAMD_DEV void tone_fold_quad(const PsyP &P, float att, const float *seed, const float *gmin, int q, float *o) {
  const int nlines = P.total_octave_lines;
  const I4 bf = dm_load_i4(P.bin_fold, (unsigned)q << 4);
  const int bfs[4] = {bf.x, bf.y, bf.z, bf.w};
  float av[4];
  f4_get(dm_load_f4(P.ath, (unsigned)q << 4), av);
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const int i = (q << 2) + c;
    float minV;
    if (i >= P.tail_linpos) {
      minV = seed[nlines - 1];
    } else {
      minV = seed[bfs[c] & 0xffff];
      if (minV > P.tone_abs_limit) minV = P.tone_abs_limit;
      const float rest = gmin[bfs[c] >> 16];
      if (rest < f_from_bits(0x7f800000u)) {
        if (minV == VAMD_NEGINF || rest < minV) minV = rest;
      }
    }
    float v = av[c] + att;
    if (v < minV) v = minV;
    o[c] = v;
  }
}
