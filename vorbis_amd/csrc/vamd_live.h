// vamd_live.h -- the live feed's plan (vamd_feed_create_live), internal to the library: vamd_plan.h (a part of vamd_hip.hip's translation unit) implements it, the
// feed (vamd_feed.hip) is its only caller.  Not part of the public ABI.
#pragma once
#include <stdint.h>
#include "vorbis_amd.h"

// One stream of a live group as the feed's host mirror sees it, in the group's buffer coordinates (k_plan_live's LiveGeo)
struct vamd_live_geo {
  long long have;  // samples in the buffer: those kept from earlier groups and this group's piece
  long long kept;  // detector steps already taken whose flags the stream's row holds (steps [0, kept))
  long long c1;    // steps this group's first detector pass takes (steps [kept, kept + c1))
  long long c2;    // a closing stream: steps of the second pass, over the end-of-stream padding
  int n_head;      // > 0: the backward extrapolation runs in this group, over the stream's first n_head frames
  int fresh;       // the stream starts in this group
  int close;       // the stream ends in this group
};

extern "C" {
#define VAMD_LIVE_WALK_BYTES 32  // sizeof(vamd::WalkState): one per stream, device memory owned by the caller

// Samples a continuing stream keeps in its buffer from one group to the next, at most: the walk
// stops in front of a block centred at c when (a) it runs out of detector steps, so the data end lies less than
// (VE_WIN + 3) steps past the block's horizon c + bs[W]/4 + bs1/2 + bs0/4, or (b) the next block's window does not fit, so
// the data end lies less than bs1 past c; the buffer then begins at c - bs1/2 - one step.  Before the backward
// extrapolation has run a stream keeps everything: the head room and fewer than n_head frames.
long vamd_live_retain(const vamd_ctx *c, int write_frames);
// 0, or why a live feed cannot run this write cadence / piece length on this context (the extrapolations' and the
// walk's LDS)
const char *vamd_live_check(const vamd_ctx *c, int write_frames, long max_frames);
// One group of a live lane, after the ingest: both stream ends where due, the detector over each stream's new steps,
// the resumed walk and the rebase; then the plan as vamd_plan_streams_whole hands it out.  pcm: [nstreams][ch][cs]
// (stream stride ss), each channel with `pad` = 3 * blocksizes[1] zeroed samples behind `have`; geo: host; walk: device
// [nstreams] walk states; rows: device [nstreams][row_stride] carried detector flags; shift (host, [nstreams]): where each
// continuing stream's next buffer begins, fetched with the block counts (the one wait).
int vamd_live_plan(vamd_ctx *c, float *pcm, long ss, long cs, long nstreams, const vamd_live_geo *geo, int n_head,
                   void *walk, unsigned char *rows, long row_stride, vamd_envelope_state *states, long long *shift,
                   vamd_stream_plan *plan);
}  // extern "C"
