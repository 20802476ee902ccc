// k_floor.h -- _vp_offset_and_mix (reference lib/psy.c:779-835), floor1_fit
// (lib/floor1.c:576-729) and the post-quantise + render_line0 half of
// floor1_encode (lib/floor1.c:766-831,923-946); SURVEY.md 8a rows a11-a13.  One
// wavefront per channel-block.
//
// Parallel form: the mix is per bin.  accumulate_fit's integer sums take one
// lane per post interval.  The greedy split loop is inherently ordered (each
// decision moves the neighbours of later posts); every lane runs it uniformly
// with the small state in LDS, while inspect_error -- the only part that
// touches O(n) bins -- is evaluated by all 64 lanes at once: the Bresenham line
// has the closed form y(x) = y0 + k*base + sgn*floor(k*ady'/adx), the squared
// error is an integer wave sum and the early-outs are an any().  fit_line's
// fp64 sums run in the reference's term order on every lane.
//
// LDS: qc[n] 16-bit words -- everything the fit reads per bin: the mask quantised by vorbis_dBquant
// (bits 0-9; the fit never looks at the float mask) and the "mdct + twofitatten >= mask" class
// (bit 15; the only thing the fit reads logmdct for) --, FloorScratch (interval accumulators + the
// rendered segment list).
#pragma once
#include "vamd_wave.h"
#include "vamd_params.h"
#include "k_tone.h"

namespace vamd {

#define VAMD_MAXPOSTS 32

// What depends on the setup alone is not redone per channel-block (profiles/r12_floor_phases.txt; DESIGN.md "Decided
// variants"): one set of post tables per channel-block (PostTables), handed from the fit to the quantiser to the curve; the
// tables behind PsyP / FloorP addressed as device memory (vamd_wave.h); the fit's work-list loop rolled (floor_fit_posts), so
// that no value is spilt to scratch round it; and fold_and_mix_wave asks for a quad's noise offsets together with its noise and
// spectrum.
#if VAMD_GPU
#define VAMD_FL_SEG_LOOP _Pragma("unroll 1")
#else
#define VAMD_FL_SEG_LOOP
#endif
// VAMD_FL_INSPECT_STOP (profiles/r19_floor_split.txt; -D...=0 restores the earlier code, which tests/test_floor_inspect_cases.py
// holds beside this one): inspect_error_wave asks after every chunk of NLANES points whether a point of it failed the over /
// under test and returns 1 there, as the reference's inspect_error does at the point itself (lib/floor1.c:537-538); it used to
// walk the whole range and ask once.  A call without a failing point runs every trip and reaches the count thresholds and the
// mse sum as before.  How many trips run after the outcome is settled: no expression changes.
#ifndef VAMD_FL_INSPECT_STOP
#define VAMD_FL_INSPECT_STOP 1
#endif
// scratch builds for the phase profile (tools/fl_phases_pmc.sh): -DVAMD_COUNT_CALLS turns the stopwatch's slots into event
// counters, summed over the waves -- slot 0 inspect_error_wave calls, slot 1 fit_line_pair calls of the split loop (= calls
// that return 1), slot 2 chunks of NLANES points walked by inspect_error_wave, slot 3 its returns of 1 on the point test,
// slot 4 its returns of 0 on the count thresholds, slot 5 split-loop trips that end at the memo test, slot 6 the sum of
// `most` over the split loop's fit_line_pair calls (tools/fl_calls.py)
#if VAMD_GPU && defined(VAMD_COUNT_CALLS)
#define VAMD_FL_COUNT(pc, k) ((pc).acc[(k)] += 1)
#define VAMD_FL_COUNT_N(pc, k, n) ((pc).acc[(k)] += (unsigned int)(n))
#else
#define VAMD_FL_COUNT(pc, k) ((void)0)
#define VAMD_FL_COUNT_N(pc, k, n) ((void)0)
#endif

#include "k_floor.inc"

}  // namespace vamd
