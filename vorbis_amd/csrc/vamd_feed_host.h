// vamd_feed_host.h -- the feed's host arithmetic that touches neither the device nor the lane: the slices of a managed group,
// the layouts of the two records the kernels write into pinned memory, the comment table the pager reads, and the host
// mirror of a live lane's streams.  A part of vamd_feed.hip's translation unit (and of k_feed.h: LiveIn is what the mirror
// builds and the live kernels read).  It includes no HIP header, so the host compiler builds these very functions for the
// CPU suite (tests/c/feed_host_cases.cpp, tests/live_host.py), as it does k_ogg.h, k_feed_src.h and k_blockout.h.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <vector>
#include "vamd_live.h"

namespace vamd {

inline size_t al(size_t x, size_t a) { return (x + a - 1) / a * a; }
inline size_t nz(long n) { return (size_t)(n ? n : 1); }  // a list of n entries is sized for one at least: no empty buffer

// ---- a bitrate-managed group's slices ----
struct Slice {
  long k0, k1, s0, s1;  // [k0, k1) of order[]; its first stream, and one past its last
  int64_t i0[2], n[2];  // its classes' first blocks in the plan's batches, and their counts
  size_t starts;        // where its stream_start lies in `starts` (one list behind the other)
};

// The slices of a group of nb = order.size() blocks in ns streams (start[]), at most S blocks each, in order[] order -- so a
// slice holds the end of one stream, whole streams, the start of another.  order[] is rebased in place to each slice's own
// batches; starts receives every slice's stream_start over its pieces of streams, relative to its first block.  Host
// arithmetic only.  *why set: the plan is not what the slices rely on.
inline std::vector<Slice> plan_slices(std::vector<int32_t> &order, const std::vector<int64_t> &start, long ns, long nb, long S,
                                      std::vector<int64_t> &starts, const char **why) {
  std::vector<Slice> sl;
  int64_t seen[2] = {0, 0};
  long s = 0;
  for (long k0 = 0; k0 < nb; k0 += S) {
    Slice x;
    x.k0 = k0, x.k1 = k0 + S < nb ? k0 + S : nb;
    while (start[(size_t)s + 1] <= k0) s++;
    x.s0 = s;
    x.s1 = s;
    while (x.s1 < ns && start[(size_t)x.s1] < x.k1) x.s1++;
    x.i0[0] = seen[0], x.i0[1] = seen[1];
    for (long k = x.k0; k < x.k1; k++) {
      const int o = order[(size_t)k], W = (o >> 30) & 1, i = o & 0x3fffffff;
      if (i != seen[W]) {  // (the plan numbers each class's blocks in stream order: vamd_plan_streams)
        *why = "stream plan: a size class's blocks are not numbered in stream order";
        return sl;
      }
      seen[W]++;
      order[(size_t)k] = (W << 30) | (int)(i - x.i0[W]);
    }
    for (int W = 0; W < 2; W++) x.n[W] = seen[W] - x.i0[W];
    x.starts = starts.size();
    for (long j = x.s0; j <= x.s1; j++) {
      const int64_t a = j == x.s0 ? x.k0 : (j == x.s1 ? x.k1 : start[(size_t)j]);
      starts.push_back((a < x.k0 ? x.k0 : (a > x.k1 ? x.k1 : a)) - x.k0);
    }
    sl.push_back(x);
  }
  return sl;
}

// ---- the two records in pinned memory: where their fields lie, for the device's view of the block and for the host's ----
// The group's record, which the copy kernels write and vamd_feed_packets hands out:
// [total | stream_start (ns + 1) | offset (nb) | granulepos (nb) | bits (nb) | info (nb)]
struct RecLayout {
  size_t start, offset, granulepos, bits, info, bytes;
  RecLayout(long ns, long nb) {
    start = 8, offset = start + (size_t)(ns + 1) * 8, granulepos = offset + (size_t)nb * 8, bits = granulepos + (size_t)nb * 8;
    info = bits + (size_t)nb * 4, bytes = al(info + (size_t)nb, 16);
  }
  // o's pointers into the record at rec (FeedOut: rec as the device sees it; vamd_feed_result: as the host does); the total is
  // the record's first word
  template <typename T>
  void point(uint8_t *rec, T &o) const {
    o.stream_start = (int64_t *)(rec + start), o.offset = (int64_t *)(rec + offset), o.granulepos = (int64_t *)(rec + granulepos);
    o.bits = (int32_t *)(rec + bits), o.info = rec + info;
  }
};

// An Ogg group's record of its files, which the pager writes and vamd_feed_ogg hands out:
// [total | stream_offset (ns + 1) | npages (ns) | status (ns)]
struct OggRecLayout {
  size_t offset, npages, status, bytes;
  explicit OggRecLayout(long ns) {
    offset = 8, npages = offset + (size_t)(ns + 1) * 8, status = npages + (size_t)ns * 4, bytes = al(status + (size_t)ns, 16);
  }
  // (OggOut: rec as the device sees it; vamd_feed_ogg_result: as the host does)
  template <typename T>
  void point(uint8_t *rec, T &o) const {
    o.stream_offset = (int64_t *)(rec + offset), o.npages = (int32_t *)(rec + npages), o.status = rec + status;
  }
};

// ---- a group's own comment headers as the pager reads them (k_ogg.h) ----
// [off (ns, 8 bytes each) | bytes (ns, 4 each) | the comments, each at a multiple of 4]; comments[s] empty, or beyond the
// vector's end: stream s has the feed's shared comment header (`shared` bytes) and bytes[s] = -1.
struct CommentTable {
  size_t bytes;     // of the image (8 beyond the last comment: the pager reads whole words)
  int32_t longest;  // the group's longest comment header: its streams' header slots are sized by it
  int64_t sum;      // ... and their sum: the file arena is (ogg_file_bound_v)
};
inline const std::vector<uint8_t> *comment_of(const std::vector<std::vector<uint8_t>> &comments, long s) {
  return (size_t)s < comments.size() && !comments[(size_t)s].empty() ? &comments[(size_t)s] : nullptr;
}
inline CommentTable comment_table(const std::vector<std::vector<uint8_t>> &comments, long ns, int32_t shared) {
  CommentTable T;
  T.bytes = al((size_t)ns * 12, 8), T.longest = 0, T.sum = 0;
  for (long s = 0; s < ns; s++) {
    const std::vector<uint8_t> *own = comment_of(comments, s);
    const size_t n = own ? own->size() : (size_t)shared;
    if (own) T.bytes += al(n, 4);
    T.sum += (int64_t)n;
    if ((int32_t)n > T.longest) T.longest = (int32_t)n;
  }
  T.bytes += 8;
  return T;
}
// ... and the image itself, T.bytes of it
inline void comment_table_image(const std::vector<std::vector<uint8_t>> &comments, long ns, const CommentTable &T, uint8_t *img) {
  int64_t *off = (int64_t *)img;
  int32_t *len = (int32_t *)(img + (size_t)ns * 8);
  memset(img, 0, T.bytes);
  size_t at = al((size_t)ns * 12, 8);
  for (long s = 0; s < ns; s++) {
    const std::vector<uint8_t> *own = comment_of(comments, s);
    off[s] = (int64_t)at, len[s] = -1;
    if (!own) continue;
    len[s] = (int32_t)own->size();
    memcpy(img + at, own->data(), own->size());
    at += al(own->size(), 4);
  }
}

// ---- the live feed (vamd_feed_create_live): continuing streams, their state on the device between groups ----
// A live lane keeps every stream in one of two buffers [stream][channel][cs], swapped each group: a stream's samples from
// where the reference's buffer begins (walk_rebase) on, then the group's piece, then zeroes (the end-of-stream padding's
// room and the detector's reads).  Per stream and group, built by the lane's host mirror:
struct LiveIn {
  int64_t first, frames;  // the piece: its first frame in the arena, its frames
  int64_t keep, shift;    // samples carried over from the other buffer, taken from sample `shift` of it on
  int64_t origin;         // the stream's position (head room included) of buffer sample 0: granule positions go on from it
  int64_t eof;            // a closing stream: its end in buffer coordinates; else LIVE_OPEN
  int32_t fresh, close;   // the stream starts / ends in this group
};
#define LIVE_OPEN (1LL << 60)
#define LIVE_NO_NAN (~0ull)

// the host's mirror of one stream of a live lane: what the device holds of it
struct LiveStream {
  bool open = false, headed = false;
  int64_t origin = 0;           // the stream's position (head room included) of buffer sample 0
  int64_t have = 0, total = 0;  // samples in the buffer; frames received
  int64_t steps = 0;            // detector steps taken (buffer coordinates)
  int64_t shift = 0;            // where the next buffer begins (the last walk's rebase)
};

// what the mirror's arithmetic takes of the feed: the long block's head room and end-of-stream padding, the detector's
// step, the frames the backward extrapolation waits for, a stream buffer's samples per channel
struct LiveShape {
  int head, pad, step;
  long n_head, cs;
  LiveShape(int bs1, int write_frames, long cs_) {
    head = bs1 / 2, pad = 3 * bs1, step = 64, cs = cs_;
    n_head = ((long)bs1 / write_frames + 1) * write_frames;  // lib/block.c:525-526
  }
};

// The mirror's step before the plan: stream m takes a piece of n frames (first: the piece's place, LiveIn::first) and closes
// with it or not.  -> the stream's LiveIn and vamd_live_geo for this group; *quads raised to the four-sample columns its
// ingest takes.  Returns 0, or why the group cannot run.
inline const char *live_piece(const LiveShape &G, LiveStream &m, int64_t first, int64_t n, bool cl, LiveIn &in, vamd_live_geo &g,
                              int64_t *quads) {
  memset(&in, 0, sizeof(in));
  memset(&g, 0, sizeof(g));
  in.first = first, in.frames = n;
  in.fresh = !m.open;
  if (!m.open && !n) {  // (a stream starts with its first frame: until then it is not there, and nothing of it is planned)
    in.eof = LIVE_OPEN;
    g.fresh = 1;
    return nullptr;
  }
  if (!m.open) {
    m = LiveStream();
    m.open = true, m.have = G.head;
    in.keep = G.head;
  } else {  // the rebase the last walk asked for
    in.shift = m.shift, in.keep = m.have - m.shift;
    m.origin += m.shift, m.steps -= m.shift / G.step, m.have = in.keep, m.shift = 0;
  }
  in.origin = m.origin;
  m.have += n, m.total += n;
  if (!m.headed && (m.total >= G.n_head || cl)) {  // the backward extrapolation: lib/block.c:524-528, or the close (:480-481)
    m.headed = true;
    g.n_head = (int)(m.total < G.n_head ? m.total : G.n_head);
  }
  g.have = m.have, g.kept = m.steps;
  if (m.headed) {
    const int64_t last = m.have / G.step - 4;  // lib/envelope.c:223-224
    g.c1 = last > m.steps ? last - m.steps : 0;
  }
  if (cl) {
    const int64_t s1 = m.steps + g.c1, sa = (m.have + G.pad) / G.step - 4;
    g.c2 = sa > s1 ? sa - s1 : 0;
  }
  g.fresh = in.fresh, g.close = cl;
  in.close = cl, in.eof = cl ? m.have : LIVE_OPEN;
  m.steps += g.c1;
  if (in.keep + n + G.pad + 256 > G.cs) return "live feed: a stream's kept samples and piece exceed its buffer (the retention bound does not hold)";
  const int64_t q = (in.keep + n + G.pad + 256 + 3) / 4;
  if (q > *quads) *quads = q;
  return nullptr;
}

// ... and its step after the plan: a stream that closed is gone (its next piece starts a fresh stream), one that goes on
// begins its next buffer at `shift`, the walk's rebase.  Returns 0, or why the stream cannot go on.
inline const char *live_planned(LiveStream &m, bool closed, int64_t shift, long retain) {
  if (closed) {
    m = LiveStream();
    return nullptr;
  }
  m.shift = shift;
  if (m.shift < 0 || m.shift > m.have || m.have - m.shift > retain) return "live feed: a stream would keep more samples than the retention bound allows";
  return nullptr;
}

}  // namespace vamd
