// vamd_decode_window_plan.h -- the host half of the window decoder (include/vorbis_amd.h: vamd_decode_window,
// vamd_ogg_index_create, vamd_decode_ogg_window; vamd_decode_window.h): out of the block plan of whole streams
// (vamd_decode_plan.h) the plan of WINDOWS of them -- per window the fewest blocks that give its frames -- and, for files,
// the seek index a walk leaves behind (vamd_demux.h) and the pages a window's blocks lie in.  Plain C++, no HIP: the
// library and the one-lane test program (tests/c/decode_window_host.cpp) share it.
//
// A window (stream, start, count) of a stream of T frames holds frames [a, b): a = min(start, T), b = min(start + count, T).
// With the stream's block centres C_0 = 0 < C_1 < ... (decode_step apart) and kA, kB the first k with C_k > a and
// C_k > b - 1, it takes blocks kA - 1 .. kB: lap_sample (k_synth.h) reads, for a frame between C_{k-1} and C_k, those two
// blocks and no other.  T <= the last centre, so kB exists; an empty window takes nothing.
#pragma once
#include "vamd_decode_plan.h"
#include "vamd_demux.h"

namespace vamd {

struct WindowPlan {
  DecodePlan P;                 // the windows as its "streams": lap_start per window; src[] in the STREAM's coordinates (its
                                // first centre at 0); packet[k] = k, the window's own copy of a block (no work is shared)
  std::vector<int64_t> first;   // [nwindows] a: the window's first frame in its stream
  std::vector<int64_t> source;  // [blocks] the packet of each block of P.order[], in the whole plan's numbering
};

// the centre of block j of `whole.order[]`
inline int64_t window_centre(const DecodePlan &whole, const int bs[2], int64_t j) {
  const int32_t o = whole.order[(size_t)j];
  const int W = (o >> 30) & 1;
  return whole.src[W][(size_t)(o & 0x3fffffff)] + bs[W] / 2;
}

// what every window list must hold -> false with a reason
inline bool window_args_check(int64_t nstreams, int64_t nwindows, const int64_t *stream, const int64_t *start, const int64_t *count, std::string *err) {
  if (nwindows < 0) return *err = "decode_window: negative window count", false;
  if (nwindows > 0x7fffffff) return *err = "decode_window: more than 2^31 windows", false;
  if (nwindows && (!stream || !start || !count)) return *err = "decode_window: null stream / start / count", false;
  const int64_t top = (int64_t)1 << 62;
  for (int64_t w = 0; w < nwindows; w++) {
    if (stream[w] < 0 || stream[w] >= nstreams) return *err = "decode_window: a window's stream is out of range", false;
    if (start[w] < 0 || start[w] > top) return *err = "decode_window: a window's start is negative or above 2^62", false;
    if (count[w] < 0 || count[w] > top) return *err = "decode_window: a window's count is negative or above 2^62", false;
  }
  return true;
}

// `whole`: decode_plan_build's plan of the streams (with the statuses the caller has or-ed in: such a stream must have no
// frames).  -> false with a reason for a bad window list.
inline bool window_plan_build(const DecodePlan &whole, const int bs[2], int64_t nwindows, const int64_t *stream, const int64_t *start,
                              const int64_t *count, WindowPlan *out, std::string *err) {
  *out = WindowPlan();
  const int64_t nstreams = (int64_t)whole.frames.size();
  if (!window_args_check(nstreams, nwindows, stream, start, count, err)) return false;
  DecodePlan &P = out->P;
  P.frames.assign((size_t)nwindows, 0);
  P.status.assign((size_t)nwindows, 0);
  P.lap_start.assign((size_t)nwindows + 1, 0);
  out->first.assign((size_t)nwindows, 0);
  for (int64_t w = 0; w < nwindows; w++) {
    const size_t s = (size_t)stream[w];
    const int64_t T = whole.status[s] ? 0 : whole.frames[s];
    const int64_t a = std::min(start[w], T), b = a + std::min(count[w], T - a);  // (= min(start + count, T), without the sum: it may pass 2^63)
    P.status[(size_t)w] = whole.status[s];
    P.frames[(size_t)w] = b - a;
    out->first[(size_t)w] = a;
    if (b > a) {
      const int64_t j0 = whole.lap_start[s], j1 = whole.lap_start[s + 1];
      auto above = [&](int64_t at) {  // the first block of [j0, j1) whose centre is > at, or j1
        int64_t lo = j0, hi = j1;
        while (lo < hi) {
          const int64_t mid = (lo + hi) >> 1;
          if (window_centre(whole, bs, mid) > at) hi = mid; else lo = mid + 1;
        }
        return lo;
      };
      const int64_t kA = above(a), kB = above(b - 1);
      if (kA <= j0 || kB >= j1) return *err = "decode_window: a window outside its stream's blocks", false;  // (never: 0 <= a, b <= T <= the last centre)
      for (int64_t j = kA - 1; j <= kB; j++) {
        const int32_t o = whole.order[(size_t)j];
        const int W = (o >> 30) & 1;
        if (P.nblocks[W] >= (1 << 30)) return *err = "decode_window: more than 2^30 blocks of a size class", false;
        P.order.push_back((int32_t)(W << 30) | (int32_t)P.nblocks[W]++);
        P.src[W].push_back(whole.src[W][(size_t)(o & 0x3fffffff)]);
        P.packet.push_back((int64_t)out->source.size());
        out->source.push_back(whole.packet[(size_t)j]);
      }
      P.max_frames = std::max(P.max_frames, b - a);
    }
    P.lap_start[(size_t)w + 1] = (int64_t)P.order.size();
  }
  return true;
}

// The packet entry's gather: the packets of the windows' blocks, back to back in plan order -> offs[blocks + 1].
inline void window_packet_layout(const WindowPlan &WP, const int64_t *offset, std::vector<int64_t> *offs) {
  offs->assign(WP.source.size() + 1, 0);
  for (size_t k = 0; k < WP.source.size(); k++) (*offs)[k + 1] = (*offs)[k] + (offset[WP.source[k] + 1] - offset[WP.source[k]]);
}
inline void window_packet_gather(const WindowPlan &WP, const uint8_t *bytes, const int64_t *offset, const std::vector<int64_t> &offs, uint8_t *stage) {
  for (size_t k = 0; k < WP.source.size();) {  // a window's packets lie back to back in the caller's bytes too: one copy a run
    size_t e = k + 1;
    while (e < WP.source.size() && WP.source[e] == WP.source[e - 1] + 1) e++;
    const int64_t n = offs[e] - offs[k];
    if (n) memcpy(stage + offs[k], bytes + offset[WP.source[k]], (size_t)n);
    k = e;
  }
}

// ---- the seek index of a group of Ogg files -------------------------------------------------------------------------------
// What one walk (demux_scan) and one block plan leave: per stream the status, T, the file's length, its page rows (src
// counted from the FILE's first byte) and the packet table with the centres.  No pointer into the caller's bytes.
struct OggIndex {
  std::vector<int64_t> file_bytes;  // [nstreams]
  DemuxScan X;
  DecodePlan whole;
};

inline bool ogg_index_build(const int bs[2], int modes, int modebits, int64_t nstreams, const uint8_t *bytes, const int64_t *file_offset,
                            const DemuxSetup &S, OggIndex *out, std::string *err) {
  *out = OggIndex();
  if (!demux_scan(nstreams, bytes, file_offset, S, &out->X, err)) return false;
  DemuxScan &X = out->X;
  if (X.pages.size() > 0x7fffffffu) return *err = "ogg_index: more than 2^31 pages", false;
  if (!decode_plan_build(bs, modes, modebits, nstreams, (int64_t)X.first.size(), nullptr, X.offset.data(), X.stream_start.data(), X.end_granule.data(),
                         &out->whole, err, X.first.data()))
    return false;
  out->file_bytes.resize((size_t)nstreams);
  for (int64_t s = 0; s < nstreams; s++) {
    out->whole.status[(size_t)s] |= X.status[(size_t)s];
    if (out->whole.status[(size_t)s]) out->whole.frames[(size_t)s] = 0;
    out->file_bytes[(size_t)s] = file_offset[s + 1] - file_offset[s];
    for (int64_t p = X.page_start[(size_t)s]; p < X.page_start[(size_t)s + 1]; p++) X.pages[(size_t)p].src -= file_offset[s] - file_offset[0];
  }
  return true;
}

// the files handed again -> false with a reason
inline bool ogg_window_files_check(const OggIndex &I, const uint8_t *bytes, const int64_t *file_offset, std::string *err) {
  const int64_t nstreams = (int64_t)I.file_bytes.size();
  if (!file_offset) return *err = "decode_ogg_window: null file_offset", false;
  if (file_offset[0] < 0) return *err = "decode_ogg_window: negative file offset", false;
  for (int64_t s = 0; s < nstreams; s++)
    if (file_offset[s + 1] < file_offset[s]) return *err = "decode_ogg_window: file offsets are not monotone", false;
  for (int64_t s = 0; s < nstreams; s++)
    if (file_offset[s + 1] - file_offset[s] != I.file_bytes[(size_t)s]) return *err = "decode_ogg_window: a file's length differs from the index's", false;
  if (file_offset[nstreams] > file_offset[0] && !bytes) return *err = "decode_ogg_window: null bytes", false;
  return true;
}

// What a window call stages and lays out: per non-empty window ONE run of its file -- the pages from the one in which its
// first packet begins through the one that holds its last packet's last byte -- copied to stage[stage_at ..]; the rows of
// those pages with src rebased into the staging buffer, dst into the call's arena (whole page bodies, window after
// window) and stream = the window; and where each block's packet begins in that arena (lengths: offs[k + 1] - offs[k]).
struct OggWindowStage {
  struct Run {
    int64_t stream, from, bytes, stage_at;  // file `stream`, its bytes [from, from + bytes)
  };
  std::vector<Run> runs;
  std::vector<OggDepage> pages;
  std::vector<int64_t> begin, offs;  // [blocks], [blocks + 1]
  int64_t stage_bytes = 0, arena_bytes = 0;
};

inline bool ogg_window_stage(const OggIndex &I, const WindowPlan &WP, const int64_t *stream, OggWindowStage *out, std::string *err) {
  *out = OggWindowStage();
  const DemuxScan &X = I.X;
  const size_t nw = WP.first.size();
  out->begin.assign(WP.source.size(), 0);
  out->offs.assign(WP.source.size() + 1, 0);
  for (size_t w = 0; w < nw; w++) {
    const int64_t k0 = WP.P.lap_start[w], k1 = WP.P.lap_start[w + 1];
    if (k1 == k0) continue;
    const size_t s = (size_t)stream[w];
    const OggDepage *pg0 = X.pages.data() + X.page_start[s], *pg1 = X.pages.data() + X.page_start[s + 1];
    const int64_t pa = WP.source[(size_t)k0], pb = WP.source[(size_t)k1 - 1];  // the first and the last packet
    auto holds = [&](int64_t byte) {  // the page of the stream whose audio bytes hold arena byte `byte`: the last with dst <= byte
      return std::upper_bound(pg0, pg1, byte, [](int64_t v, const OggDepage &p) { return v < p.dst; }) - 1;
    };
    if (X.offset[(size_t)pb + 1] <= X.offset[(size_t)pa]) return *err = "decode_ogg_window: a window of empty packets", false;  // (never: such a stream is flagged)
    const OggDepage *p0 = holds(X.offset[(size_t)pa]), *p1 = holds(X.offset[(size_t)pb + 1] - 1);
    if (p0 < pg0 || p1 < p0) return *err = "decode_ogg_window: a packet outside its stream's pages", false;  // (never)
    OggWindowStage::Run run;
    run.stream = (int64_t)s, run.from = p0->src, run.bytes = p1->src + OGG_HEADER + p1->nseg + p1->body - p0->src, run.stage_at = out->stage_bytes;
    if (run.from < 0 || run.bytes < 0 || run.from + run.bytes > I.file_bytes[s]) return *err = "decode_ogg_window: pages outside the file", false;  // (never)
    const int64_t arena0 = out->arena_bytes;
    for (const OggDepage *p = p0; p <= p1; p++) {
      OggDepage row = *p;
      row.src = run.stage_at + (p->src - p0->src), row.dst = arena0 + (p->dst - p0->dst), row.stream = (int32_t)w;
      out->pages.push_back(row);
    }
    out->runs.push_back(run);
    out->stage_bytes += run.bytes;
    out->arena_bytes += p1->dst + (p1->body - p1->skip) - p0->dst;
    for (int64_t k = k0; k < k1; k++) {
      const int64_t p = WP.source[(size_t)k];
      out->begin[(size_t)k] = arena0 + (X.offset[(size_t)p] - p0->dst);
      out->offs[(size_t)k + 1] = out->offs[(size_t)k] + (X.offset[(size_t)p + 1] - X.offset[(size_t)p]);
    }
  }
  for (size_t k = 0; k < WP.source.size(); k++) {
    const int64_t len = out->offs[k + 1] - out->offs[k];
    if (out->begin[k] < 0 || len < 0 || out->begin[k] + len > out->arena_bytes) return *err = "decode_ogg_window: a packet outside the arena", false;  // (never)
  }
  for (const OggDepage &row : out->pages)
    if (!ogg_depage_inside(row, out->stage_bytes, out->arena_bytes)) return *err = "decode_ogg_window: a page outside its buffers", false;  // (never)
  return true;
}

inline void ogg_window_gather(const OggWindowStage &G, const uint8_t *bytes, const int64_t *file_offset, uint8_t *stage) {
  for (const OggWindowStage::Run &r : G.runs)
    if (r.bytes) memcpy(stage + r.stage_at, bytes + file_offset[r.stream] + r.from, (size_t)r.bytes);
}

}  // namespace vamd
