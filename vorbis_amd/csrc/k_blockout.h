// k_blockout.h -- the block-size decisions of vorbis_analysis_blockout() (reference lib/block.c:534-693) and
// the integer half of _ve_envelope_search() / _ve_envelope_mark() (lib/envelope.c:241-353), device-resident:
// one WAVE per stream walks its whole mark sequence (sixty-four marks per look) and emits the stream's block list, so
// that a set of streams goes from PCM to analysed blocks without a host round trip per block.
//
// The reference keeps a sliding PCM buffer and shifts every position by the block advance after each block
// (lib/block.c:649-685, _ve_envelope_shift); here every position is an ABSOLUTE sample index into the stream's
// buffer as the encoder would hold it had nothing been shifted out (what vorbis_analysis_buffer/_wrote
// accumulate, including the start-of-stream pre-extrapolation of lib/block.c:398-458, which is host code in
// the reference and stays the caller's).  Shifting subtracts the same amount from both sides of every
// comparison, so the decisions are the same.  The one asymmetry -- ve->curmark stops being shifted once it
// is negative, lib/envelope.c:372 -- only ever makes an already out-of-range mark stay out of range.
//
// What a plan covers: with BlockoutP::eof == 0 the blocks the reference would hand out while the data given suffices,
// i.e. with v->eofflag == 0 throughout.  With eof > 0 the stream ENDS at that sample (v->eofflag of
// vorbis_analysis_wrote(v, 0), lib/block.c:474-488, as an absolute index) and the buffer holds the reference's
// three long blocks of LPC padding behind it (k_lpc.h): a cursor walk that runs out of steps then forces a short
// next block instead of waiting (lib/block.c:558-563), and the block whose centre lies at or beyond eof is the
// stream's last (:664-670).
#pragma once
#include "vamd_wave.h"

namespace vamd {

#define VAMD_VE_WIN 4   // lib/envelope.h:23
#define VAMD_VE_POST 2  // lib/envelope.h:24

struct BlockoutP {
  int bs[2];        // blocksizes
  int searchstep;   // 64
  long nsamples;    // samples per channel in each stream's buffer
  long nsteps;      // detector steps available per stream (flags[s][0 .. nsteps))
  int maxblocks;    // capacity of a stream's row in `blocks`
  long eof;         // 0: the stream goes on (more data may come); > 0: v->eofflag as an absolute sample index
  int lstep;        // log2(searchstep) where that is a power of two (libvorbis: 64), else -1 (blockout_set_step)
};
// positions / searchstep for positions >= 0 (every one the walk divides): a shift where the step allows it -- a 64-bit
// division by a run-time value is some eighty vector instructions, and the walk made three or four per block
VAMD_DEV long blockout_div_step(const BlockoutP &B, long x) { return B.lstep >= 0 ? x >> B.lstep : x / B.searchstep; }
VAMD_HOSTDEV void blockout_set_step(BlockoutP &B, int searchstep) {
  B.searchstep = searchstep;
  B.lstep = -1;
  for (int l = 0; l < 30; l++)
    if ((1 << l) == searchstep) B.lstep = l;
}

// one planned block: W | lW << 1 | nW << 2 | blocktype << 3 in `kind`, and where its window starts
struct PlannedBlock {
  int kind;
  int begin;  // first sample of the block's window in the stream's buffer (centerW - blocksize/2)
};

// ve->mark[p] once every step that can touch it has run (lib/envelope.c:241-258): step j clears mark[j+2],
// then a pre-echo flag (1) marks j and j+1, a post-echo flag (2) marks j and j-1.  The clear of p happens at
// step p-2, before any of its setters (steps p-1, p, p+1), so the final value is the OR of those.
VAMD_DEV int mark_at(const unsigned char *__restrict__ flags, long nsteps, long p) {
  int m = 0;
  if (p < 0) return 0;
  if (p >= 1 && p - 1 < nsteps) m |= flags[p - 1] & 1;
  if (p < nsteps) m |= flags[p] & 3;
  if (p + 1 < nsteps) m |= flags[p + 1] & 2;
  return m != 0;
}

VAMD_DEV long blockout_steps(const BlockoutP &B) {
  long last = blockout_div_step(B, B.nsamples) - VAMD_VE_WIN;
  if (last > B.nsteps) last = B.nsteps;
  return last < 0 ? 0 : last;
}

// What the walk carries from one call to the next (v->W, v->lW, v->centerW, ve->cursor, ve->curmark), positions in the
// stream buffer's coordinates.  A stream that is fed in pieces (the live feed) resumes from it.
struct WalkState {
  long centerW, cursor, curmark;
  int W, lW;
};
// vorbis_analysis_init / _ve_envelope_init: lib/block.c:211-213, lib/envelope.c:41
VAMD_HOSTDEV WalkState walk_fresh(const BlockoutP &B) {
  WalkState s;
  s.centerW = s.cursor = B.bs[1] / 2;
  s.curmark = 0;
  s.W = s.lW = 0;
  return s;
}
// The live feed's rebase after a walk that stopped in front of the block centred at centerW: the reference's memmove
// leaves its buffer starting at centerW - blocksizes[1]/2 (lib/block.c:657-690); one step more is kept, whose detector flag
// still feeds the first kept mark (mark_at).  A multiple of the step: marks and detector steps keep their grid.
VAMD_HOSTDEV long walk_rebase(const BlockoutP &B, long centerW) {
  long sh = centerW - B.bs[1] / 2 - B.searchstep;
  if (sh < 0) sh = 0;
  return sh / B.searchstep * B.searchstep;
}

// ---- where the walk reads its marks: a MARK SOURCE has need(keep, lo, hi), called with wave-uniform arguments before every
// group of reads -- the marks [lo, hi) are about to be read, and no mark below `keep` will be asked for again -- and at(i).

// The whole of ve->mark[] at once: the steps [0, last) as bytes (mark_at applied by the caller; entries at and beyond
// `last` are 0: steps not taken yet).  The live feed's piece, the host-compiled tests.
struct MarkArray {
  const unsigned char *m;
  VAMD_MEM void need(long, long, long) {}
  VAMD_MEM int at(long i) const { return m[i]; }
};

// The smallest window a MarkWindow may have.  The walk reads marks in two places; with kc = cursor / step and
// kw = (centerW - blocksizes[0]/2) / step, the lowest mark it can still need is keep = min(kc, kw): the cursor walk never goes
// back behind the cursor, _ve_envelope_mark's span begins at kw for the block in hand and further on for every later one
// (centerW only grows).  A refill puts the window's first mark there, so a group of reads [lo, hi) must satisfy
// hi - keep <= size, i.e. both hi - kc <= size and hi - kw <= size:
//  (a) a trip of the cursor walk, lo = base / step, hi <= lo + 64, and no further than the horizon: hi <= ceil(testW / step)
//      with testW = centerW + blocksizes[W]/4 + blocksizes[1]/2 + blocksizes[0]/4.  The first trip starts on the cursor and
//      every later one a step behind it (a trip that does not stop leaves the cursor on its last lane): hi - kc <= 65,
//      however far the cursor lags -- a short block chosen while W is long leaves it up to blocksizes[1]/4 +
//      blocksizes[0]/4 behind the next centre, far behind that centre's kw, and the trips simply start there.
//      hi - kw <= ceil(testW / step) - floor((centerW - blocksizes[0]/2) / step)
//              <= ceil((3 * blocksizes[1]/4 + 3 * blocksizes[0]/4) / step) + 1   (W long at worst).
//  (b) _ve_envelope_mark's span of a short block, [kw, (centerW + blocksizes[0]/2) / step) cut at `last`:
//      hi - kw <= ceil(blocksizes[0] / step) + 1, less than (a).  It runs after the block's cursor walk, which left the
//      cursor beyond centerW (stopped on a mark), within a step of testW (stopped at the horizon) -- kc >= kw in both -- or
//      on the last step it could visit, kc >= last - 2 >= hi - 2: the forced short blocks at the end of a stream, whose
//      centres run on while the cursor stands, read nothing at or beyond `last`.
// (The +1s: a floor and a ceiling on the two ends.)  With libvorbis' block sizes the second term is 28 (256 / 2048) or 55
// (512 / 4096) and the horizon cuts every trip short of 64 lanes, so 65 -- the width of a trip, which holds whatever the
// sizes -- is the minimum in practice; with block sizes 64 / 8192 the second term (98) is, and it is tight: the host build
// sees reads outside a window one mark smaller (tests/test_plan_window_cpu.py).
VAMD_HOSTDEV long plan_window_min(const BlockoutP &B) {
  const long a = (3 * (long)(B.bs[0] + B.bs[1]) / 4 + B.searchstep - 1) / B.searchstep + 1;
  return a > 65 ? a : 65;
}
VAMD_HOSTDEV long plan_window_clamp(const BlockoutP &B, long marks) {
  const long lo = plan_window_min(B);
  return marks < lo ? lo : marks;
}
#define VAMD_PLAN_WINDOW_DEFAULT 32768  // marks: two million samples between refills (DESIGN.md section 5 has the measurement)

// every read inside the window: the test build's check on plan_window_min (tests/plan_window_host.py counts instead of aborting)
#ifndef VAMD_WINDOW_CHECK
#if VAMD_GPU
#define VAMD_WINDOW_CHECK(ok) ((void)0)
#else
#include <assert.h>
#define VAMD_WINDOW_CHECK(ok) assert(ok)
#endif
#endif

// ve->mark[] through a window of `size` bytes (LDS on the device) over a stream of any length: w[i - base] is mark i for
// base <= i < base + size.  The marks are made from the detector's flags when the window fills (mark_at, over the two
// pieces: f holds the flags of the steps [0, split), f2 those from split on; steps at and beyond `last` have not been taken);
// a read outside the window refills all of it from `keep` on -- coalesced reads of the flag rows by the whole wave.
struct MarkWindow {
  unsigned char *w;
  long size, base, refills;
  const unsigned char *f, *f2;
  long split, last;
  VAMD_MEM void open(unsigned char *window, long size_, const unsigned char *flags, long split_, const unsigned char *flags2, long last_) {
    w = window, size = size_, f = flags, f2 = flags2, split = split_, last = last_;
    refills = -1;
    fill(0);
  }
  VAMD_MEM int flag(long p) const { return p < split ? f[p] : f2[p - split]; }
  VAMD_MEM void fill(long from) {
    WAVE_SYNC();  // (the reads out of the window as it was)
    base = from;
    refills++;
    for (long k = LANE; k < size; k += NLANES) {
      const long p = base + k;
      int m = 0;  // mark_at()
      if (p < last) {
        if (p >= 1) m |= flag(p - 1) & 1;
        m |= flag(p) & 3;
        if (p + 1 < last) m |= flag(p + 1) & 2;
      }
      w[k] = (unsigned char)(m != 0);
    }
    WAVE_SYNC();
  }
  VAMD_MEM void need(long keep, long lo, long hi) {
    if (lo < base || hi > base + size) fill(keep);
    VAMD_WINDOW_CHECK(lo >= base && hi <= base + size);
  }
  VAMD_MEM int at(long i) const {
    VAMD_WINDOW_CHECK(i >= base && i < base + size);
    return w[i - base];
  }
};

// The walk for one stream.  Returns the number of blocks planned (<= maxblocks) and counts per size class.
//   marks  where ve->mark[] of the steps [0, last) is read (a mark source, above)
//   pending_center  (optional) centerW of the block the walk stopped in front of: where the reference's buffer would
//          begin (centerW - blocksizes[1]/2) when vorbis_analysis_wrote(v, 0) pads the stream
//   state  (optional, in/out) where the walk starts (null: a fresh stream) and, on return, where it stands
template <class Marks>
VAMD_DEV int plan_walk(const BlockoutP &B, Marks &marks, PlannedBlock *__restrict__ out, int *count_short, int *count_long,
                         long *pending_center = nullptr, WalkState *state = nullptr) {
  const long step = B.searchstep;
  const int bs0 = B.bs[0], bs1 = B.bs[1];  // (selected, not indexed, by W: an indexed copy of B would live in scratch memory)
  const WalkState s0 = state ? *state : walk_fresh(B);
  int W = s0.W, lW = s0.lW;
  long centerW = s0.centerW, cursor = s0.cursor, curmark = s0.curmark;
  // what _ve_envelope_search has marked: steps [0, last), last = pcm_current/searchstep - VE_WIN (:223-224)
  const long last = blockout_steps(B);
  const long current = last * step;
  int n = 0, n0 = 0, n1 = 0;
  while (n < B.maxblocks) {
    // ---- _ve_envelope_search's cursor walk, lib/envelope.c:262-325
    const long testW = centerW + (W ? bs1 : bs0) / 4 + bs1 / 2 + bs0 / 4;
    // the lowest mark still needed from here on (plan_window_min); the marks a trip reads end in front of the horizon
    // and of the last step a walk visits (j < testW, j < current - step)
    const long kw = blockout_div_step(B, centerW - bs0 / 2);
    long top = blockout_div_step(B, testW + step - 1);
    if (top > last - 1) top = last - 1;
    int bp = -1;
    // The walk sixty-four steps at a time: a trip looks at j = base + l * step, l < 64.  The walk stops at the first j that
    // is past the horizon (j >= testW: long block, cursor stays on the last j visited before it) or marked beyond the
    // block's centre (short block, cursor and curmark on it); a j at or past current - step is not visited at all, and a
    // walk that runs out of them leaves the cursor on the last one it did visit.
    for (long base = cursor;; base += 64 * step) {
      const long i0 = blockout_div_step(B, base), kc = blockout_div_step(B, cursor);
      const long i1 = i0 + 64 < top ? i0 + 64 : top;
      if (i0 < i1) marks.need(kc < kw ? kc : kw, i0, i1);
#if VAMD_GPU
      // (every lane of the wave runs plan_stream; all its values are wave-uniform): lane l looks at j = base + l * step
      const long j = base + (long)LANE * step;
      const bool visited = j < current - step;  // (the visited lanes are a prefix of the wave)
      const bool past = visited && j >= testW;
      const bool marked = visited && !past && marks.at(i0 + LANE) && j > centerW;
      const unsigned long long stop = __ballot(past || marked);
      if (stop) {
        const int l = __builtin_ctzll(stop);
        if ((__ballot(past) >> l) & 1) {
          bp = 1;
          if (l > 0) cursor = base + (long)(l - 1) * step;  // (else: where the previous trip, or the caller, left it)
        } else {
          bp = 0;
          cursor = curmark = base + (long)l * step;
        }
        break;
      }
      const int nvis = __builtin_popcountll(__ballot(visited));
      if (nvis > 0) cursor = base + (long)(nvis - 1) * step;
      if (nvis < 64) break;  // ran out of steps: bp stays -1
#else
      int l = 0;
      for (; l < 64; l++) {
        const long j = base + (long)l * step;
        if (!(j < current - step)) break;  // ran out of steps: bp stays -1
        if (j >= testW) {
          bp = 1;
          break;
        }
        cursor = j;
        if (marks.at(i0 + l) && j > centerW) {
          curmark = j;
          bp = 0;
          break;
        }
      }
      if (l < 64) break;
#endif
    }
    if (bp < 0 && !B.eof) break;  // "not enough data currently to search for a full long block", lib/block.c:558-560
    const int nW = (bp < 0 || bs0 == bs1) ? 0 : bp;  // (at the end of a stream: nW = 0, :561)
    const long centerNext = centerW + (W ? bs1 : bs0) / 4 + (nW ? bs1 : bs0) / 4;
    if (B.nsamples < centerNext + (nW ? bs1 : bs0) / 2) break;  // lib/block.c:574-583
    // ---- the block, lib/block.c:589-611
    int blocktype;
    if (W) {
      blocktype = (!lW || !nW) ? 0 /* BLOCKTYPE_TRANSITION */ : 1 /* BLOCKTYPE_LONG */;
    } else {
      // _ve_envelope_mark, lib/envelope.c:329-353 (W == 0: both neighbours count as short)
      const long beginW = centerW - bs0 / 4 - bs0 / 4, endW = centerW + bs0 / 4 + bs0 / 4;
      int hit = curmark >= beginW && curmark < endW;
      long i_begin = blockout_div_step(B, beginW), i_end = blockout_div_step(B, endW);  // (beginW >= 0: centerW >= blocksizes[1] / 2)
      if (i_begin < 0) i_begin = 0;
      if (i_end > last) i_end = last;
      if (!hit && i_begin < i_end) {
        const long kc = blockout_div_step(B, cursor);
        marks.need(kc < i_begin ? kc : i_begin, i_begin, i_end);
      }
#if VAMD_GPU
      for (long i0 = i_begin; !hit && i0 < i_end; i0 += 64) {  // (a short block's span is a handful of steps: one trip)
        const long i = i0 + LANE;
        hit = __ballot(i < i_end && marks.at(i)) != 0;
      }
#else
      for (long i = i_begin; !hit && i < i_end; i++) hit = marks.at(i);
#endif
      blocktype = hit ? 0 /* BLOCKTYPE_IMPULSE */ : 1 /* BLOCKTYPE_PADDING */;
    }
    if (LANE == 0 && out) {
      out[n].kind = W | (lW << 1) | (nW << 2) | (blocktype << 3);
      out[n].begin = (int)(centerW - (W ? bs1 : bs0) / 2);
    }
    n++;
    if (W) n1++; else n0++;
    if (B.eof && centerW >= B.eof) {  // the stream's last block (vb->eofflag = 1), lib/block.c:664-670
      centerW = -1;
      break;
    }
    // ---- advance, lib/block.c:649-685 (positions stay absolute: nothing to shift)
    lW = W;
    W = nW;
    centerW = centerNext;
  }
  *count_short = n0;
  *count_long = n1;
  if (pending_center) *pending_center = centerW;  // (-1: the stream is over)
  if (state) {
    state->W = W, state->lW = lW;
    state->centerW = centerW, state->cursor = cursor, state->curmark = curmark;
  }
  return n;
}
// the walk over a whole mark array (MarkArray)
VAMD_DEV int plan_stream(const BlockoutP &B, const unsigned char *marks, PlannedBlock *__restrict__ out, int *count_short,
                         int *count_long, long *pending_center = nullptr, WalkState *state = nullptr) {
  MarkArray m = {marks};
  return plan_walk(B, m, out, count_short, count_long, pending_center, state);
}
// the walk through a window (MarkWindow)
VAMD_DEV int plan_stream(const BlockoutP &B, MarkWindow &marks, PlannedBlock *__restrict__ out, int *count_short, int *count_long,
                         long *pending_center = nullptr, WalkState *state = nullptr) {
  return plan_walk(B, marks, out, count_short, count_long, pending_center, state);
}

}  // namespace vamd
