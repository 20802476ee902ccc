// vamd_feed.hip -- the host-fed farm: whole streams in from host memory (16-bit interleaved, as
// examples/encoder_example.c:179-202 reads them), finished packets back to host memory, over one or several GPUs
// (include/vorbis_amd.h, "the host-fed farm"; SURVEY.md 8d "H2D/D2H-inclusive", 8e).
//
// Every figure the library reported up to round 5 was for samples already resident in HBM.  A caller's samples are
// in host memory, and the link is the narrowest pipe on the way: a long stereo block advances its stream by 1024
// frames = 4 KB of 16-bit samples, so a 64 GB/s link feeds at most ~14 M blocks/s -- IF it is busy all the time and
// carries nothing but samples up and packet bytes down.  Hence the shape:
//   * LANES.  A lane is a context, a HIP stream, a thread of the library's, a pinned input arena, a pinned output
//     arena and the HBM buffers of one group of streams.  A group's life on its lane: one copy command up (the pinned
//     arena is what the copy engine reads: no staging copy on the host) -> k_feed_ingest (16-bit -> float, planar, with
//     the room either end that vamd_plan_streams_whole fills) -> the plan (LPC ends, detector, block walk; its block
//     counts are the lane thread's one wait in mid-flight) -> vamd_analyze_streams_mixed with packet output, blocks read
//     where they lie (50 % overlap never copied) -> three small kernels that lay the packets end to end: per-stream
//     sizes (a wave per stream), a scan over the streams, and a wave per packet that copies its words STRAIGHT INTO the
//     pinned output arena (mapped into the device's address space: the packets cross the link inside that kernel, no
//     copy command, no second wait).  Lanes are independent: while one computes, another's upload is on the wire.
//   * the call sequence is libvorbis' own, for a group: vamd_feed_buffer / _wrote / _packets / _release.
// Built on the public C ABI only (a context is used by one thread: its lane's), like vamd_batcher.hip.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <memory>
#include <condition_variable>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "vorbis_amd.h"
#include "vamd_knobs.h"
#include "vamd_live.h"
#include "k_ogg.h"

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
size_t al(size_t x, size_t a) { return (x + a - 1) / a * a; }

// ---- kernels ------------------------------------------------------------------------------------------------

// in [s][frame][c] (int16 or float) -> pcm[s * ss + c * cs + head + frame]; the room in front (head samples) and behind
// (pad samples) zeroed, as the reference's calloc'ed / not yet written buffer is.  A thread takes four frames of every
// channel: one 8 ch-byte (16-bit) or 16 ch-byte read, one 16-byte store per channel.
// frames_of / first_of (optional): streams of unequal length laid back to back -- stream s has frames_of[s] <= frames frames
// starting at frame first_of[s] of the arena; the rest of its buffer (laid out for `frames`) is zeroed.
template <typename T>
__global__ void k_feed_ingest(const T *__restrict__ in, int ch, long nstreams, long frames, int head, int pad,
                              float *__restrict__ pcm, long ss, long cs, float *__restrict__ amp,
                              vamd_envelope_state *__restrict__ states, const long long *__restrict__ frames_of,
                              const long long *__restrict__ first_of) {
  const long quads = (frames + 3) >> 2, hq = head >> 2, pq = pad >> 2, per = hq + quads + pq, total = nstreams * per;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
    const long s = t / per, q = t - s * per;
    float *row = pcm + s * ss;
    const long mine = frames_of ? (long)frames_of[s] : frames, first = first_of ? (long)first_of[s] : s * frames;
    if (q < hq) {
      for (int c = 0; c < ch; c++) ((float4 *)(row + (long)c * cs))[q] = make_float4(0.f, 0.f, 0.f, 0.f);
      if (q == 0) amp[s] = VAMD_AMPMAX_FLOOR;
    } else if (q < hq + quads) {
      const long f0 = (q - hq) << 2;
      const T *src = in + (first + f0) * ch;
      const int live = mine - f0 < 4 ? (mine > f0 ? (int)(mine - f0) : 0) : 4;
      for (int c = 0; c < ch; c++) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          float x = 0.f;
          if (k < live) {
            if (sizeof(T) == 2) x = (float)(int)src[k * ch + c] / 32768.f;  // examples/encoder_example.c:197-202
            else x = (float)src[k * ch + c];
          }
          v[k] = x;
        }
        ((float4 *)(row + (long)c * cs + head))[q - hq] = make_float4(v[0], v[1], v[2], v[3]);
      }
    } else {
      const long f0 = (quads << 2) + ((q - hq - quads) << 2);
      for (int c = 0; c < ch; c++) ((float4 *)(row + (long)c * cs + head + f0))[0] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  // a fresh detector state per stream (all-zero == a stream's start, include/vorbis_amd.h)
  const long words = nstreams * (long)(sizeof(vamd_envelope_state) / 4);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < words; t += (long)gridDim.x * blockDim.x) ((uint32_t *)states)[t] = 0u;
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

// a fresh stream's states: the detector's (all zero), the ampmax chain's, the bitrate manager's (a copy of `tmpl`), no
// non-finite sample yet.  A stream that goes on keeps all of them.
__global__ void k_live_begin(long nstreams, const LiveIn *__restrict__ li, vamd_envelope_state *__restrict__ states,
                             float *__restrict__ amp, vamd_bitrate_state *__restrict__ bst, const vamd_bitrate_state *__restrict__ tmpl,
                             unsigned long long *__restrict__ nan) {
  const long words = (long)(sizeof(vamd_envelope_state) / 4);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < nstreams * words; t += (long)gridDim.x * blockDim.x) {
    const long s = t / words;
    if (!li[s].fresh) continue;
    ((uint32_t *)states)[t] = 0u;
    if (t - s * words == 0) {
      amp[s] = VAMD_AMPMAX_FLOOR;
      if (bst) bst[s] = *tmpl;
      nan[s] = LIVE_NO_NAN;
    }
  }
}

// the group's buffer, a thread per four samples of every channel of a stream (one 16-byte store per channel): the kept
// samples out of the other buffer (a fresh stream: the zeroed head room), the piece behind them (x / 32768.f for 16-bit
// input, examples/encoder_example.c:197-202), zeroes up to `room` samples past the piece.  Float input: the first
// non-finite sample of each stream is recorded (absolute position, nan[]).  A stream whose samples would not fit its
// buffer is left alone and flagged in *status (the lane reports it; never written past the buffer).
template <typename T>
__global__ void k_live_ingest(const T *__restrict__ in, int ch, long nstreams, long quads, int room, const LiveIn *__restrict__ li,
                              const float *__restrict__ old, float *__restrict__ pcm, long ss, long cs,
                              unsigned long long *__restrict__ nan, int *__restrict__ status) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < nstreams * quads; t += (long)gridDim.x * blockDim.x) {
    const long s = t / quads, p0 = (t - s * quads) << 2;
    const LiveIn L = li[s];
    const long data = L.keep + L.frames, end = data + room < cs ? data + room : cs;
    if (data + room > cs || L.keep < 0 || L.shift < 0 || L.shift + L.keep > cs) {
      if (p0 == 0) *(volatile int *)status = 1;  // (host memory, mapped: a plain store)
      continue;
    }
    if (p0 >= end) continue;
    for (int c = 0; c < ch; c++) {
      float v[4];
      bool bad = false;
      long badp = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const long p = p0 + k;
        float x = 0.f;
        if (p < L.keep) {
          if (!L.fresh) x = old[s * ss + (long)c * cs + L.shift + p];
        } else if (p < data) {
          const T y = in[(L.first + p - L.keep) * ch + c];
          if (sizeof(T) == 2) x = (float)(int)y / 32768.f;
          else {
            x = (float)y;
            if (!bad && (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u) bad = true, badp = p;
          }
        }
        v[k] = x;
      }
      ((float4 *)(pcm + s * ss + (long)c * cs))[p0 >> 2] = make_float4(v[0], v[1], v[2], v[3]);
      if (bad) atomicMin(nan + s, (unsigned long long)(L.origin + badp));
    }
  }
}

// what a live group adds to a packet's record: its granule position goes on from the stream's origin, e_o_s only where the
// stream closes, and from the block that holds a stream's first non-finite sample on no packet (VAMD_STATUS_NONFINITE)
struct FeedLive {
  const LiveIn *in;
  const unsigned long long *nan;
};
__device__ __forceinline__ unsigned live_status(const FeedLive &V, long s, int64_t begin, int bs) {
  return V.in && (unsigned long long)(V.in[s].origin + begin + bs) > V.nan[s] ? VAMD_STATUS_NONFINITE : 0u;
}

struct FeedPlan {  // what the packing kernels need of a vamd_stream_plan and of the analysis' outputs
  const int32_t *order;
  const int64_t *stream_start;
  const int64_t *src[2];
  const int32_t *bits[2];
  const uint8_t *status[2];
  const uint8_t *packets[2];
  int64_t stride[2];
  int bs[2];
  int ch;
  int64_t stream_stride, eof;  // eof: first sample past the stream's real ones, in its buffer's coordinates
  const long long *frames_of;  // streams of unequal length: eof = head + frames_of[s]
  int head;
  FeedLive live;               // a live group's streams (in == null: whole streams)
};

// a wave per stream: rel[k] = bytes (each packet rounded up to 4) of the stream's packets before packet k
__global__ __launch_bounds__(64) void k_feed_sizes(FeedPlan P, long nstreams, int64_t *__restrict__ rel, int64_t *__restrict__ stream_bytes) {
  const long s = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t k0 = P.stream_start[s], k1 = P.stream_start[s + 1];
  int64_t run = 0;
  for (int64_t base = k0; base < k1; base += 64) {
    const int64_t k = base + lane;
    int bytes = 0;
    if (k < k1) {
      const int o = P.order[k], W = (o >> 30) & 1, i = o & 0x3fffffff;
      unsigned st = 0;
      for (int c = 0; c < P.ch; c++) st |= P.status[W][(int64_t)i * P.ch + c];
      st |= live_status(P.live, s, P.src[W][i] - s * P.stream_stride, P.bs[W]);
      bytes = st ? 0 : (((P.bits[W][i] + 7) >> 3) + 3) & ~3;
    }
    int incl = bytes;  // inclusive scan over the wave
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (k < k1) rel[k] = run + incl - bytes;
    run += __shfl(incl, 63, 64);
  }
  if (lane == 0) stream_bytes[s] = run;
}

// one workgroup: stream_off[s] = bytes of all streams before s; stream_off[nstreams] = the total
__global__ __launch_bounds__(1024) void k_feed_scan(long nstreams, const int64_t *__restrict__ stream_bytes, int64_t *__restrict__ stream_off) {
  __shared__ int64_t part[1024];
  const int t = threadIdx.x;
  const long per = (nstreams + 1023) / 1024, lo = (long)t * per, hi = lo + per < nstreams ? lo + per : nstreams;
  int64_t sum = 0;
  for (long s = lo; s < hi; s++) sum += stream_bytes[s];
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < 1024; d <<= 1) {
    const int64_t v = t >= d ? part[t - d] : 0;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  int64_t run = part[t] - sum;
  for (long s = lo; s < hi; s++) {
    stream_off[s] = run;
    run += stream_bytes[s];
  }
  if (t == 1023) stream_off[nstreams] = part[1023];
}

// a wave per packet: its words into the output arena (host memory, mapped), its record beside them
struct FeedOut {
  int64_t *stream_start, *offset, *granulepos, *total;
  int32_t *bits;
  uint8_t *info, *bytes;
  int64_t cap;  // bytes the arena holds
  // an Ogg feed (m_bytes set): the device mirror of the arena and of the records, which the pager reads (k_ogg.h)
  uint8_t *m_bytes, *m_info;
  int64_t *m_off, *m_gp;
  int32_t *m_bits;
};
__global__ __launch_bounds__(256) void k_feed_copy(FeedPlan P, long nstreams, long nblocks, const int64_t *__restrict__ rel,
                                                   const int64_t *__restrict__ stream_off, const int32_t *__restrict__ sid,
                                                   FeedOut O) {
  const long k = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k == 0 && lane == 0) *O.total = stream_off[nstreams];
  if (k <= nstreams && lane == 1) O.stream_start[k] = P.stream_start[k];  // (nstreams + 1 <= nblocks + 1 entries; see the launch)
  if (k >= nblocks) return;
  const int s = sid[k];
  const int o = P.order[k], W = (o >> 30) & 1, i = o & 0x3fffffff;
  unsigned st = 0;
  for (int c = 0; c < P.ch; c++) st |= P.status[W][(int64_t)i * P.ch + c];
  st |= live_status(P.live, s, P.src[W][i] - (int64_t)s * P.stream_stride, P.bs[W]);
  const int bits = P.bits[W][i], words = st ? 0 : (((bits + 7) >> 3) + 3) >> 2;
  const int64_t off = stream_off[s] + rel[k];
  const bool fits = off + 4 * (int64_t)words <= O.cap;
  if (fits) {
    const uint32_t *src = (const uint32_t *)(P.packets[W] + (int64_t)i * P.stride[W]);
    uint32_t *dst = (uint32_t *)(O.bytes + off);
    uint32_t *mir = O.m_bytes ? (uint32_t *)(O.m_bytes + off) : nullptr;
    for (int w = lane; w < words; w += 64) {
      const uint32_t v = src[w];
      dst[w] = v;
      if (mir) mir[w] = v;
    }
  }
  if (lane == 0) {
    const int64_t begin = P.src[W][i] - (int64_t)s * P.stream_stride, center = begin + P.bs[W] / 2;
    const bool last = k + 1 == P.stream_start[s + 1] && (!P.live.in || P.live.in[s].close);
    O.offset[k] = off;
    O.bits[k] = st ? -1 : bits;
    const int64_t eof = P.live.in ? P.live.in[s].eof : (P.frames_of ? (int64_t)P.head + P.frames_of[s] : P.eof);
    const int64_t gp = (center < eof ? center : eof) - P.bs[1] / 2 + (P.live.in ? P.live.in[s].origin : 0);
    const uint8_t info = (uint8_t)(W | (last ? 2 : 0) | ((st & 3) << 2));
    O.granulepos[k] = gp;
    O.info[k] = info;
    if (O.m_bytes) O.m_off[k] = off, O.m_bits[k] = st ? -1 : bits, O.m_gp[k] = gp, O.m_info[k] = info;
  }
}

// sid[k] = the stream packet k belongs to (a wave per stream)
__global__ __launch_bounds__(64) void k_feed_sid(const int64_t *__restrict__ stream_start, int32_t *__restrict__ sid) {
  const long s = blockIdx.x;
  for (int64_t k = stream_start[s] + threadIdx.x; k < stream_start[s + 1]; k += 64) sid[k] = (int32_t)s;
}

// ---- bitrate-managed setups: a slice of the group's blocks at a time (run_group_managed) ----
// What the two kernels below need of a slice: its blocks in stream order (order[] rebased to the slice's own batches,
// stream_start over the slice's pieces of streams), the walk's choice / final_bits, the candidates' rows and bit counts
// -- and of the group: the plan's stream_start, src and the streams' lengths, for the records.
struct FeedSlice {
  const int32_t *order;          // [slice blocks] W << 30 | index in the slice's batch of class W
  const int64_t *stream_start;   // [slice streams + 1] into order[]
  const int64_t *g_start;        // the plan's stream_start (whole group)
  const int64_t *src[2];         // the plan's src[W] (whole group)
  const int32_t *choice[2], *fbits[2], *mbits[2];  // [slice batch] / [slice batch][15]
  const uint8_t *status[2];
  const uint8_t *packets[2];     // [slice batch][15][stride]
  int64_t stride[2];
  int64_t i0[2];                 // the slice's first block of class W in the plan's batches
  int64_t k0;                    // ... and its first block in the plan's order[]
  long s0;                       // the group stream of the slice's first stream
  int bs[2];
  int ch;
  int64_t stream_stride, eof;
  const long long *frames_of;
  int head;
  FeedLive live;
};

// a wave per slice stream: rel[k] = bytes (each handed-out packet rounded up to 4) of the slice stream's packets before k
__global__ __launch_bounds__(64) void k_feed_sizes_managed(FeedSlice P, int64_t *__restrict__ rel, int64_t *__restrict__ stream_bytes) {
  const long s = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t k0 = P.stream_start[s], k1 = P.stream_start[s + 1];
  int64_t run = 0;
  for (int64_t base = k0; base < k1; base += 64) {
    const int64_t k = base + lane;
    int bytes = 0;
    if (k < k1) {
      const int o = P.order[k], W = (o >> 30) & 1, i = o & 0x3fffffff;
      unsigned st = 0;
      for (int c = 0; c < P.ch; c++) st |= P.status[W][(int64_t)i * P.ch + c];
      const long gs = P.s0 + s;
      st |= live_status(P.live, gs, P.src[W][P.i0[W] + i] - gs * P.stream_stride, P.bs[W]);
      bytes = st ? 0 : (((P.fbits[W][i] + 7) >> 3) + 3) & ~3;
    }
    int incl = bytes;
    for (int d = 1; d < 64; d <<= 1) {
      const int up = __shfl_up(incl, d, 64);
      if (lane >= d) incl += up;
    }
    if (k < k1) rel[k] = run + incl - bytes;
    run += __shfl(incl, 63, 64);
  }
  if (lane == 0) stream_bytes[s] = run;
}

// a wave per packet of the slice: the chosen candidate's first bytes, zero bytes behind them up to the handed-out size
// (the manager's padding) and to the next multiple of 4, into the output arena at base + stream_off + rel; the record of
// the packet at its place in the group (k0 + k)
__global__ __launch_bounds__(256) void k_feed_copy_managed(FeedSlice P, long nblocks, int64_t base, const int64_t *__restrict__ rel,
                                                           const int64_t *__restrict__ stream_off, const int32_t *__restrict__ sid,
                                                           FeedOut O) {
  const long k = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= nblocks) return;
  const int ls = sid[k];
  const long s = P.s0 + ls;
  const int o = P.order[k], W = (o >> 30) & 1, i = o & 0x3fffffff;
  unsigned st = 0;
  for (int c = 0; c < P.ch; c++) st |= P.status[W][(int64_t)i * P.ch + c];
  st |= live_status(P.live, s, P.src[W][P.i0[W] + i] - s * P.stream_stride, P.bs[W]);
  const int choice = P.choice[W][i], fbits = P.fbits[W][i];
  const int64_t fb = st ? 0 : ((int64_t)fbits + 7) >> 3;
  int64_t own = st ? 0 : ((int64_t)P.mbits[W][(int64_t)i * VAMD_PACKETBLOBS + choice] + 7) >> 3;
  if (own > P.stride[W]) own = P.stride[W];
  const int64_t keep = own < fb ? own : fb, words = (fb + 3) >> 2;
  const int64_t off = base + stream_off[ls] + rel[k];
  if (off + 4 * words <= O.cap) {
    const uint8_t *row = P.packets[W] + ((int64_t)i * VAMD_PACKETBLOBS + choice) * P.stride[W];
    uint32_t *dst = (uint32_t *)(O.bytes + off);
    uint32_t *mir = O.m_bytes ? (uint32_t *)(O.m_bytes + off) : nullptr;
    for (int64_t w = lane; w < words; w += 64) {
      uint32_t v = 0;
      if (4 * w < keep) {
        v = ((const uint32_t *)row)[w];
        const int64_t live = keep - 4 * w;  // bytes of this word that are the candidate's
        if (live < 4) v &= (1u << (8 * live)) - 1u;
      }
      dst[w] = v;
      if (mir) mir[w] = v;
    }
  }
  if (lane == 0) {
    const int64_t g = P.k0 + k, gi = P.i0[W] + i;
    const int64_t begin = P.src[W][gi] - (int64_t)s * P.stream_stride, center = begin + P.bs[W] / 2;
    const bool last = g + 1 == P.g_start[s + 1] && (!P.live.in || P.live.in[s].close);
    O.offset[g] = off;
    O.bits[g] = st ? -1 : fbits;
    const int64_t eof = P.live.in ? P.live.in[s].eof : (P.frames_of ? (int64_t)P.head + P.frames_of[s] : P.eof);
    const int64_t gp = (center < eof ? center : eof) - P.bs[1] / 2 + (P.live.in ? P.live.in[s].origin : 0);
    const uint8_t info = (uint8_t)(W | (last ? 2 : 0) | ((st & 3) << 2) | ((st ? 0 : choice) << 4));
    O.granulepos[g] = gp;
    O.info[g] = info;
    if (O.m_bytes) O.m_off[g] = off, O.m_bits[g] = st ? -1 : fbits, O.m_gp[g] = gp, O.m_info[g] = info;
  }
}

struct Buf {
  void *p = nullptr;
  size_t bytes = 0;
  bool host = false;
  hipError_t need(size_t n) {
    if (bytes >= n) return hipSuccess;
    if (p) (void)(host ? hipHostFree(p) : hipFree(p));
    p = nullptr, bytes = 0;
    const hipError_t e = host ? hipHostMalloc(&p, n, hipHostMallocDefault) : hipMalloc(&p, n);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  void drop() {
    if (p) (void)(host ? hipHostFree(p) : hipFree(p));
    p = nullptr, bytes = 0;
  }
  // pinned host memory only: at least n bytes, the first `keep` kept
  hipError_t grow_keeping(size_t n, size_t keep) {
    if (bytes >= n) return hipSuccess;
    void *q = nullptr;
    const hipError_t e = hipHostMalloc(&q, n, hipHostMallocDefault);
    if (e != hipSuccess) return e;
    if (p && keep) memcpy(q, p, keep < bytes ? keep : bytes);
    drop();
    p = q, bytes = n;
    return hipSuccess;
  }
};

}  // namespace

enum { LANE_FREE = 0, LANE_FILLING, LANE_QUEUED, LANE_DONE };

struct FeedLane {
  int device = 0;
  vamd_ctx *ctx = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev_up = nullptr, ev_end = nullptr;
  Buf h_in, h_out, h_rec;                      // pinned: the group's samples; its packets; their records
  Buf d_in, d_pcm, d_states, d_amp;            // HBM: the samples as they came; as floats, planar; detector states; ampmax chains
  Buf d_pk[2], d_bits[2], d_status[2];         // the analysis' packet rows per size class
  Buf d_rel, d_sid, d_sbytes, d_soff, d_len, h_len;  // (d_len / h_len: [frames_of | first_of] of a group of unequal streams)
  // bitrate-managed setups (run_group_managed): a slice's fifteen candidates per block and what the analysis needs beside
  // them, the walk's answers, the managers' states, the slices' rebased lists (h_slice pinned, d_slice its copy)
  Buf d_mpk[2], d_mbits[2], d_mposts[2], d_mvalid[2], d_miwork[2], d_mnz[2], d_choice[2], d_fbits[2];
  Buf d_bstate, d_slice, h_slice;
  // a live feed (run_group_live): the two stream buffers, the walks' states, the carried detector flags, the first
  // non-finite sample per stream, the manager's fresh state; the group's LiveIn (pinned, its copy) and the host mirror
  Buf d_buf[2], d_walk, d_rows, d_nan, d_btmpl, d_live, h_live, h_lstatus;
  int cur = 0;                    // the buffer that holds the streams now
  bool btmpl_ready = false;
  struct LiveStream {             // the host's mirror of one stream of the lane
    bool open = false, headed = false;
    int64_t origin = 0;           // the stream's position (head room included) of buffer sample 0
    int64_t have = 0, total = 0;  // samples in the buffer; frames received
    int64_t steps = 0;            // detector steps taken (buffer coordinates)
    int64_t shift = 0;            // where the next buffer begins (the last walk's rebase)
  };
  std::vector<LiveStream> live;
  // an Ogg feed (vamd_feed_ogg_headers): the device mirror of the packet arena and of the records, the header packets, the
  // group's serial numbers, the page table and the streams' file sizes; the files (pinned) and their record (pinned)
  Buf d_mirror, d_moff, d_mgp, d_mrbits, d_minfo, d_hdr, d_serial, h_serial, d_pages, d_fbytes, d_foff, d_npages, d_ostatus;
  Buf h_ogg, h_orec;
  int32_t hdr_off[3] = {0, 0, 0};
  std::vector<uint32_t> serials, user_serials;  // the job's; what vamd_feed_ogg_serials set for it
  vamd_feed_ogg_result ogg_result;
  std::vector<uint8_t> close_of;  // the job's closes (live)
  std::thread worker;
  std::mutex *upload_turn = nullptr;  // its device's (vamd_feed::upload_turns)
  // the job (guarded by vamd_feed::m)
  int state = LANE_FREE;
  long nstreams = 0, frames = 0;  // frames: the group's longest stream
  std::vector<int64_t> frames_of;  // empty: every stream is `frames` long
  int format = 0;
  int status = 0;
  std::string err;
  vamd_feed_result result;
  double t_wrote = 0.;
  long served = 0;  // groups this lane has carried (the free lane that has waited longest goes out first)
};

struct vamd_feed {
  std::vector<FeedLane> lanes;
  int ch = 0, bs[2] = {0, 0};
  bool managed = false;  // the blob carries a bitrate manager (vamd_setup_header.off_bitrate): run_group_managed
  long slice = 2048;     // blocks per slice of a managed group (VAMD_FEED_SLICE, a test knob)
  long pkcap[2] = {0, 0};
  long max_streams = 0, max_frames = 0;
  int format = VAMD_FEED_S16;
  int write_frames = 0;             // > 0: a live feed (vamd_feed_create_live), the reference's frames per write
  long live_cs = 0, row_stride = 0, retain = 0;  // its buffers' samples per channel, flag rows, the retention bound
  bool ogg = false;                 // an Ogg feed (vamd_feed_ogg_headers): files beside the packets
  std::vector<uint8_t> ogg_hdr[3];  // its identification, comment and setup packets
  uint32_t next_serial = 0;         // the running serial number (a group's streams take the next nstreams)
  long rate = 0;
  std::mutex m;
  std::vector<std::unique_ptr<std::mutex>> upload_turns;  // one per device
  std::condition_variable cv_work, cv_done;
  bool stop = false;
  long turn = 0;
  std::string err;
};

#define FEED_TRY(expr)                                                              \
  do {                                                                              \
    const hipError_t e__ = (expr);                                                  \
    if (e__ != hipSuccess) {                                                        \
      L.err = std::string(#expr) + ": " + hipGetErrorString(e__);                   \
      return VAMD_EFAULT;                                                           \
    }                                                                               \
  } while (0)
#define FEED_CALL(expr)                                                             \
  do {                                                                              \
    const int r__ = (expr);                                                         \
    if (r__) {                                                                      \
      L.err = std::string(#expr) + ": " + vamd_last_error(L.ctx);                   \
      return r__;                                                                   \
    }                                                                               \
  } while (0)

#define FEED_OWN(expr)           \
  do {                           \
    const int r__ = (expr);      \
    if (r__) return r__;         \
  } while (0)

// ---- an Ogg feed: the mirror the copy kernels fill, the pager behind the last packet (k_ogg.h) ----
// The mirror's buffers for a group of nb packets, as large as the packet arena (+ 16: the pager reads whole words), the
// first `keep` bytes kept when it has to grow in mid-group (a managed group's earlier slices); O's mirror pointers set, or
// null on a feed without Ogg headers.
static int feed_mirror(vamd_feed *f, FeedLane &L, FeedOut &O, long nb, size_t keep) {
  O.m_bytes = O.m_info = nullptr, O.m_off = O.m_gp = nullptr, O.m_bits = nullptr;
  if (!f->ogg) return VAMD_OK;
  const size_t want = L.h_out.bytes + 16, n = (size_t)(nb ? nb : 1);
  if (L.d_mirror.bytes < want) {
    if (keep && L.d_mirror.p) {
      void *q = nullptr;
      FEED_TRY(hipMalloc(&q, want));
      FEED_TRY(hipMemcpyAsync(q, L.d_mirror.p, keep < L.d_mirror.bytes ? keep : L.d_mirror.bytes, hipMemcpyDeviceToDevice, L.stream));
      FEED_TRY(hipStreamSynchronize(L.stream));
      L.d_mirror.drop();
      L.d_mirror.p = q, L.d_mirror.bytes = want;
    } else {
      FEED_TRY(hipStreamSynchronize(L.stream));  // (nothing in flight reads the old one when it goes)
      FEED_TRY(L.d_mirror.need(want));
    }
  }
  FEED_TRY(L.d_moff.need(n * 8));
  FEED_TRY(L.d_mgp.need(n * 8));
  FEED_TRY(L.d_mrbits.need(n * 4));
  FEED_TRY(L.d_minfo.need(n));
  O.m_bytes = (uint8_t *)L.d_mirror.p, O.m_info = (uint8_t *)L.d_minfo.p;
  O.m_off = (int64_t *)L.d_moff.p, O.m_gp = (int64_t *)L.d_mgp.p, O.m_bits = (int32_t *)L.d_mrbits.p;
  return VAMD_OK;
}

// the group's record of its files, in pinned memory: [total | stream_offset (ns + 1) | npages (ns) | status (ns)]
static size_t orec_npages(long ns) { return 8 + (size_t)(ns + 1) * 8; }
static size_t orec_status(long ns) { return orec_npages(ns) + (size_t)ns * 4; }

// The pager, queued behind the group's last copy kernel: k_ogg_plan (a wave per stream) -> k_feed_scan (the files end to
// end) -> k_ogg_pages (a wave per page slot; the pages cross the link inside it).  Nothing here waits: the page table is
// sized by ogg_slots_per_packet, the arena by ogg_file_bound of the PACKET arena's size -- packets that fit theirs make
// files that fit this one.  d_packet_total (VBR): the packets' bytes on the device; beyond the arena nothing was mirrored
// and nothing is paged (finish_group lays the group out again).
static int run_pager(vamd_feed *f, FeedLane &L, const int64_t *d_stream_start, long ns, long nb, const int64_t *d_packet_total) {
  hipStream_t st = L.stream;
  int32_t hb[3];
  for (int i = 0; i < 3; i++) hb[i] = (int32_t)f->ogg_hdr[i].size();
  if (!L.d_hdr.p) {  // the header packets, each at a multiple of 4: once per lane
    size_t at = 0;
    for (int i = 0; i < 3; i++) L.hdr_off[i] = (int32_t)at, at += al((size_t)hb[i], 4);
    std::vector<uint8_t> img(at + 16, 0);
    for (int i = 0; i < 3; i++) memcpy(img.data() + L.hdr_off[i], f->ogg_hdr[i].data(), (size_t)hb[i]);
    FEED_TRY(L.d_hdr.need(img.size()));
    FEED_TRY(hipMemcpy(L.d_hdr.p, img.data(), img.size(), hipMemcpyHostToDevice));
  }
  if ((long)L.serials.size() != ns || !L.d_mirror.p) {
    L.err = "Ogg feed: the group has no serial numbers or no mirror";
    return VAMD_EFAULT;
  }
  FEED_TRY(L.h_serial.need((size_t)ns * 4));
  FEED_TRY(L.d_serial.need((size_t)ns * 4));
  memcpy(L.h_serial.p, L.serials.data(), (size_t)ns * 4);
  FEED_TRY(hipMemcpyAsync(L.d_serial.p, L.h_serial.p, (size_t)ns * 4, hipMemcpyHostToDevice, st));
  const int64_t hs = vamd::ogg_header_slots(hb), sp = vamd::ogg_slots_per_packet(f->pkcap[0] > f->pkcap[1] ? f->pkcap[0] : f->pkcap[1]);
  const int64_t nslots = ns * hs + sp * nb;
  FEED_TRY(L.d_pages.need((size_t)nslots * sizeof(vamd::OggPage)));
  FEED_TRY(L.d_fbytes.need((size_t)ns * 8));
  FEED_TRY(L.d_foff.need((size_t)(ns + 1) * 8));
  FEED_TRY(L.d_npages.need((size_t)ns * 4));
  FEED_TRY(L.d_ostatus.need((size_t)ns));
  FEED_TRY(L.h_orec.need(al(orec_status(ns) + (size_t)ns, 16)));
  FEED_TRY(L.h_ogg.need(al((size_t)vamd::ogg_file_bound((int64_t)L.h_out.bytes, nb, ns, hb) + 16, 4096)));
  void *drec = nullptr, *dbytes = nullptr;
  FEED_TRY(hipHostGetDevicePointer(&drec, L.h_orec.p, 0));
  FEED_TRY(hipHostGetDevicePointer(&dbytes, L.h_ogg.p, 0));
  vamd::OggIn I;
  I.stream_start = d_stream_start;
  I.off = (const int64_t *)L.d_moff.p, I.gp = (const int64_t *)L.d_mgp.p, I.bits = (const int32_t *)L.d_mrbits.p;
  I.info = (const uint8_t *)L.d_minfo.p, I.bytes = (const uint8_t *)L.d_mirror.p, I.cap = (int64_t)L.h_out.bytes;
  I.packet_total = d_packet_total;
  I.hdr = (const uint8_t *)L.d_hdr.p;
  for (int i = 0; i < 3; i++) I.hdr_off[i] = L.hdr_off[i], I.hdr_bytes[i] = hb[i];
  I.serial = (const uint32_t *)L.d_serial.p;
  I.header_slots = hs, I.slots_per_packet = sp;
  vamd::OggOut O;
  uint8_t *dr = (uint8_t *)drec;
  O.total = (int64_t *)dr, O.stream_offset = (int64_t *)(dr + 8), O.npages = (int32_t *)(dr + orec_npages(ns)), O.status = dr + orec_status(ns);
  O.bytes = (uint8_t *)dbytes, O.cap = (int64_t)L.h_ogg.bytes;
  hipLaunchKernelGGL(vamd::k_ogg_plan, dim3((unsigned)ns), dim3(64), 0, st, I, ns, (vamd::OggPage *)L.d_pages.p, (int64_t *)L.d_fbytes.p,
                     (int32_t *)L.d_npages.p, (uint8_t *)L.d_ostatus.p);
  hipLaunchKernelGGL(k_feed_scan, dim3(1), dim3(1024), 0, st, ns, (const int64_t *)L.d_fbytes.p, (int64_t *)L.d_foff.p);
  hipLaunchKernelGGL(vamd::k_ogg_pages, dim3((unsigned)nslots), dim3(64), 0, st, I, ns, (const vamd::OggPage *)L.d_pages.p,
                     (const int64_t *)L.d_foff.p, (const int32_t *)L.d_npages.p, (const uint8_t *)L.d_ostatus.p, O);
  FEED_TRY(hipGetLastError());
  return VAMD_OK;
}

// ... and after the group's wait: what vamd_feed_ogg hands out
static int pager_result(vamd_feed *f, FeedLane &L, long ns) {
  (void)f;
  const uint8_t *hr = (const uint8_t *)L.h_orec.p;
  vamd_feed_ogg_result &R = L.ogg_result;
  R.nstreams = ns;
  R.stream_offset = (const int64_t *)(hr + 8), R.npages = (const int32_t *)(hr + orec_npages(ns)), R.status = hr + orec_status(ns);
  R.bytes = (const uint8_t *)L.h_ogg.p, R.total_bytes = *(const int64_t *)hr;
  for (long s = 0; s < ns; s++)
    if (R.status[s] & 0x80) {
      L.err = "Ogg feed: a stream needed more pages than its slots of the page table";
      return VAMD_EFAULT;
    }
  if (R.total_bytes + 4 > (int64_t)L.h_ogg.bytes) {
    L.err = "Ogg feed: the files exceed the bound their arena was sized by";
    return VAMD_EFAULT;
  }
  return VAMD_OK;
}

// A bitrate-managed group, from its plan on: the blocks in slices of at most f->slice (in order[] order, so a slice holds
// the end of one stream, whole streams, the start of another), each slice through
//   vamd_analyze_streams_mixed_managed (fifteen candidate packets per block; the ampmax chains resume per stream) ->
//   vamd_bitrate_walk (the managers resume per stream) -> the handed-out packets laid end to end behind the previous
//   slice's, straight into the pinned arena
// The workspace is bounded by the slice, not the group: a long stereo block's candidates alone take 15 x its integer
// residue (120 KB) and 15 packet rows.  The host waits once per slice for the slice's byte count (to grow the arena
// before anything is written into it: the candidates do not outlive their slice).
// (live: `live` set, ns streams planned of which the caller's first ns_out are reported; the managers carried across groups)
static int run_group_managed(vamd_feed *f, FeedLane &L, const vamd_stream_plan &plan, const float *pcm, long ns, long ss, long cs,
                             const long long *d_frames_of, FeedLive live, long ns_out) {
  const long frames = L.frames;
  const int ch = f->ch, head = f->bs[1] / 2;
  const long nb = (long)(plan.nblocks[0] + plan.nblocks[1]);
  hipStream_t st = L.stream;
  std::vector<int32_t> order((size_t)(nb ? nb : 1));
  std::vector<int64_t> start((size_t)ns + 1);
  FEED_CALL(vamd_plan_fetch(L.ctx, &plan, nullptr, nullptr, nullptr, nullptr, order.data(), start.data()));
  // the slices: [k0, k1) of order[], their first stream, their classes' first blocks and counts, order[] rebased to the
  // slice's batches and stream_start over the slice's pieces of streams -- all slices' lists in one upload
  struct Slice {
    long k0, k1, s0, s1;  // s1: one past the slice's last stream
    int64_t i0[2], n[2];
    size_t starts;        // where its stream_start lies in the uploaded lists (int64 units, behind the rebased order[])
  };
  std::vector<Slice> sl;
  const long S = f->slice;
  int64_t seen[2] = {0, 0}, most[2] = {0, 0};
  size_t nstarts = 0;
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
        L.err = "stream plan: a size class's blocks are not numbered in stream order";
        return VAMD_EFAULT;
      }
      seen[W]++;
      order[(size_t)k] = (W << 30) | (int)(i - x.i0[W]);
    }
    for (int W = 0; W < 2; W++) {
      x.n[W] = seen[W] - x.i0[W];
      if (x.n[W] > most[W]) most[W] = x.n[W];
    }
    x.starts = nstarts;
    nstarts += (size_t)(x.s1 - x.s0) + 1;
    sl.push_back(x);
  }
  const size_t lists = al((size_t)(nb ? nb : 1) * 4, 8) + nstarts * 8;
  FEED_TRY(L.h_slice.need(lists + 16));
  FEED_TRY(L.d_slice.need(lists + 16));
  int64_t *h_total = (int64_t *)L.h_slice.p;  // [0]: the slice's byte count on its way back
  uint8_t *hl = (uint8_t *)L.h_slice.p + 16, *dl = (uint8_t *)L.d_slice.p + 16;
  memcpy(hl, order.data(), (size_t)nb * 4);
  int64_t *hs = (int64_t *)(hl + al((size_t)(nb ? nb : 1) * 4, 8));
  for (const Slice &x : sl)
    for (long j = x.s0; j <= x.s1; j++) {
      const int64_t a = j == x.s0 ? x.k0 : (j == x.s1 ? x.k1 : start[(size_t)j]);
      hs[x.starts + (size_t)(j - x.s0)] = (a < x.k0 ? x.k0 : (a > x.k1 ? x.k1 : a)) - x.k0;
    }
  FEED_TRY(hipMemcpyAsync(dl, hl, lists, hipMemcpyHostToDevice, st));
  const int32_t *d_order = (const int32_t *)dl;
  const int64_t *d_starts = (const int64_t *)(dl + al((size_t)(nb ? nb : 1) * 4, 8));
  // the slice's buffers, sized for the largest slice of each class
  const int K = VAMD_PACKETBLOBS;
  for (int W = 0; W < 2; W++) {
    const size_t m = (size_t)(most[W] ? most[W] : 1), n2 = (size_t)f->bs[W] / 2;
    FEED_TRY(L.d_mpk[W].need(m * K * (size_t)f->pkcap[W]));
    FEED_TRY(L.d_mbits[W].need(m * K * 4));
    FEED_TRY(L.d_mposts[W].need(m * K * ch * VAMD_POSTS_STRIDE * 4));
    FEED_TRY(L.d_mvalid[W].need(m * K * ch * 4));
    FEED_TRY(L.d_miwork[W].need(m * K * ch * n2 * 4));
    FEED_TRY(L.d_mnz[W].need(m * K * ch * 4));
    FEED_TRY(L.d_status[W].need(m * (size_t)ch));
    FEED_TRY(L.d_choice[W].need(m * 4));
    FEED_TRY(L.d_fbits[W].need(m * 4));
  }
  const size_t most_slice = (size_t)(S < nb ? S : (nb ? nb : 1));
  FEED_TRY(L.d_rel.need(most_slice * 8));
  FEED_TRY(L.d_sid.need(most_slice * 4));
  FEED_TRY(L.d_sbytes.need((size_t)ns * 8));
  FEED_TRY(L.d_soff.need((size_t)(ns + 1) * 8));
  if (!live.in) {  // (a live lane's managers live across groups: k_live_begin starts the fresh ones)
    FEED_TRY(L.d_bstate.need((size_t)ns * sizeof(vamd_bitrate_state)));
    FEED_CALL(vamd_bitrate_init_states(L.ctx, (vamd_bitrate_state *)L.d_bstate.p, ns));
  }
  // records: [total | stream_start (ns + 1) | offset (nb) | granulepos (nb) | bits (nb) | info (nb)], as run_group's
  const size_t o_start = 8, o_off = o_start + (size_t)(ns + 1) * 8, o_gp = o_off + (size_t)nb * 8, o_bits = o_gp + (size_t)nb * 8,
               o_info = o_bits + (size_t)nb * 4, rec_bytes = al(o_info + (size_t)nb, 16);
  FEED_TRY(L.h_rec.need(rec_bytes + rec_bytes / 4));
  uint8_t *hrec = (uint8_t *)L.h_rec.p;
  void *drec = nullptr;
  FEED_TRY(hipHostGetDevicePointer(&drec, hrec, 0));
  int64_t base = 0;  // bytes of the packets laid out so far
  for (const Slice &x : sl) {
    const long nss = x.s1 - x.s0, nbs = x.k1 - x.k0;
    vamd_batch_desc desc[2];
    vamd_batch_io io[2];
    vamd_managed_io m[2];
    for (int W = 0; W < 2; W++) {
      memset(&desc[W], 0, sizeof(desc[W]));
      memset(&io[W], 0, sizeof(io[W]));
      memset(&m[W], 0, sizeof(m[W]));
      desc[W].W = W;
      desc[W].nblocks = (long)x.n[W];
      if (!x.n[W]) continue;
      desc[W].lW = plan.lW[W] + x.i0[W], desc[W].nW = plan.nW[W] + x.i0[W], desc[W].blocktype = plan.blocktype[W] + x.i0[W];
      io[W].pcm = pcm;
      io[W].pcm_src = plan.src[W] + x.i0[W];
      io[W].pcm_channel_stride = cs;
      io[W].status = (uint8_t *)L.d_status[W].p;
      m[W].posts = (int32_t *)L.d_mposts[W].p;
      m[W].post_valid = (int32_t *)L.d_mvalid[W].p;
      m[W].iwork = (int32_t *)L.d_miwork[W].p;
      m[W].nonzero = (int32_t *)L.d_mnz[W].p;
      m[W].packets = (uint8_t *)L.d_mpk[W].p;
      m[W].packet_bits = (int32_t *)L.d_mbits[W].p;
      m[W].packet_stride = f->pkcap[W];
    }
    const int32_t *o = d_order + x.k0;
    const int64_t *ls = d_starts + x.starts;
    FEED_CALL(vamd_analyze_streams_mixed_managed(L.ctx, &desc[0], &io[0], &m[0], &desc[1], &io[1], &m[1], o, ls, nss, nbs,
                                                 (float *)L.d_amp.p + x.s0));
    const int32_t *bits[2] = {(const int32_t *)L.d_mbits[0].p, (const int32_t *)L.d_mbits[1].p};
    const uint8_t *stat[2] = {(const uint8_t *)L.d_status[0].p, (const uint8_t *)L.d_status[1].p};
    int32_t *choice[2] = {(int32_t *)L.d_choice[0].p, (int32_t *)L.d_choice[1].p};
    int32_t *fbits[2] = {(int32_t *)L.d_fbits[0].p, (int32_t *)L.d_fbits[1].p};
    FEED_CALL(vamd_bitrate_walk(L.ctx, o, ls, nss, bits, stat, (vamd_bitrate_state *)L.d_bstate.p + x.s0, choice, fbits));
    FeedSlice P;
    P.order = o, P.stream_start = ls, P.g_start = plan.stream_start;
    for (int W = 0; W < 2; W++) {
      P.src[W] = plan.src[W], P.choice[W] = choice[W], P.fbits[W] = fbits[W], P.mbits[W] = bits[W], P.status[W] = stat[W];
      P.packets[W] = (const uint8_t *)L.d_mpk[W].p, P.stride[W] = f->pkcap[W], P.i0[W] = x.i0[W], P.bs[W] = f->bs[W];
    }
    P.k0 = x.k0, P.s0 = x.s0, P.ch = ch, P.stream_stride = ss, P.eof = head + frames, P.frames_of = d_frames_of, P.head = head;
    P.live = live;
    hipLaunchKernelGGL(k_feed_sid, dim3((unsigned)nss), dim3(64), 0, st, ls, (int32_t *)L.d_sid.p);
    hipLaunchKernelGGL(k_feed_sizes_managed, dim3((unsigned)nss), dim3(64), 0, st, P, (int64_t *)L.d_rel.p, (int64_t *)L.d_sbytes.p);
    hipLaunchKernelGGL(k_feed_scan, dim3(1), dim3(1024), 0, st, nss, (const int64_t *)L.d_sbytes.p, (int64_t *)L.d_soff.p);
    FEED_TRY(hipGetLastError());
    FEED_TRY(hipMemcpyAsync(h_total, (const int64_t *)L.d_soff.p + nss, 8, hipMemcpyDeviceToHost, st));
    FEED_TRY(hipStreamSynchronize(st));
    const int64_t need = base + *h_total;
    if (need > (int64_t)L.h_out.bytes) FEED_TRY(L.h_out.grow_keeping((size_t)need + (size_t)need / 8, (size_t)base));
    void *dbytes = nullptr;
    FEED_TRY(hipHostGetDevicePointer(&dbytes, L.h_out.p, 0));
    FeedOut O;
    uint8_t *dr = (uint8_t *)drec;
    O.total = (int64_t *)dr, O.stream_start = (int64_t *)(dr + o_start), O.offset = (int64_t *)(dr + o_off);
    O.granulepos = (int64_t *)(dr + o_gp), O.bits = (int32_t *)(dr + o_bits), O.info = dr + o_info;
    O.bytes = (uint8_t *)dbytes, O.cap = (int64_t)L.h_out.bytes;
    FEED_OWN(feed_mirror(f, L, O, nb, (size_t)base));
    hipLaunchKernelGGL(k_feed_copy_managed, dim3((unsigned)((nbs + 3) / 4)), dim3(256), 0, st, P, nbs, base, (const int64_t *)L.d_rel.p,
                       (const int64_t *)L.d_soff.p, (const int32_t *)L.d_sid.p, O);
    FEED_TRY(hipGetLastError());
    base = need;
  }
  if (f->ogg) FEED_OWN(run_pager(f, L, plan.stream_start, ns, nb, nullptr));
  FEED_TRY(hipEventRecord(L.ev_end, st));
  FEED_TRY(hipEventSynchronize(L.ev_end));
  if (f->ogg) FEED_OWN(pager_result(f, L, ns));
  *(int64_t *)hrec = base;
  memcpy(hrec + o_start, start.data(), (size_t)(ns + 1) * 8);
  vamd_feed_result &R = L.result;
  R.nstreams = ns_out, R.nblocks = nb;
  R.stream_start = (const int64_t *)(hrec + o_start), R.offset = (const int64_t *)(hrec + o_off);
  R.granulepos = (const int64_t *)(hrec + o_gp), R.bits = (const int32_t *)(hrec + o_bits), R.info = hrec + o_info;
  R.bytes = (const uint8_t *)L.h_out.p, R.total_bytes = base;
  float up = 0.f, dev = 0.f;
  (void)hipEventElapsedTime(&up, L.ev0, L.ev_up);
  (void)hipEventElapsedTime(&dev, L.ev0, L.ev_end);
  L.result.upload_ms = up, L.result.device_ms = dev;
  return VAMD_OK;
}

static int finish_group(vamd_feed *f, FeedLane &L, const vamd_stream_plan &plan, const float *pcm, long ns, long ss, long cs,
                        const long long *d_frames_of, FeedLive live, long ns_out);

// one group through its lane (the lane's own thread; its device is current)
static int run_group(vamd_feed *f, FeedLane &L) {
  const long ns = L.nstreams, frames = L.frames;
  const int ch = f->ch, head = f->bs[1] / 2, pad = 3 * f->bs[1];
  const size_t sample = L.format == VAMD_FEED_S16 ? 2 : 4;
  const bool uneven = !L.frames_of.empty();
  size_t in_frames = (size_t)ns * frames;
  if (uneven) {
    in_frames = 0;
    for (long i = 0; i < ns; i++) in_frames += (size_t)L.frames_of[(size_t)i];
  }
  const size_t in_bytes = in_frames * ch * sample;
  const long cs = (long)al((size_t)head + ((frames + 3) & ~3L) + pad, 64), ss = cs * ch;
  hipStream_t st = L.stream;
  FEED_TRY(L.d_in.need(in_bytes ? in_bytes : 16));
  FEED_TRY(L.d_pcm.need((size_t)ns * ss * 4));
  FEED_TRY(L.d_states.need((size_t)ns * sizeof(vamd_envelope_state)));
  FEED_TRY(L.d_amp.need((size_t)ns * 4));
  const long long *d_frames_of = nullptr, *d_first_of = nullptr;
  if (uneven) {
    FEED_TRY(L.h_len.need((size_t)ns * 16));
    FEED_TRY(L.d_len.need((size_t)ns * 16));
    long long *h = (long long *)L.h_len.p, at = 0;
    for (long i = 0; i < ns; i++) {
      h[i] = L.frames_of[(size_t)i];
      h[ns + i] = at;
      at += h[i];
    }
    FEED_TRY(hipMemcpyAsync(L.d_len.p, h, (size_t)ns * 16, hipMemcpyHostToDevice, st));
    d_frames_of = (const long long *)L.d_len.p;
    d_first_of = d_frames_of + ns;
  }
  {
    // ONE upload at a time per device.  The link is a single resource: lanes that upload side by side each get a share
    // of it and all finish late together -- and then all compute together while the link idles (measured: three lanes
    // in lockstep, 2.3 ms of every 13 without a single kernel on the chip).  Taking turns, a lane has the whole link,
    // starts its kernels the moment its samples are up, and the next lane's upload runs beside them: the lanes stagger
    // themselves.
    std::lock_guard<std::mutex> turn(*L.upload_turn);
    FEED_TRY(hipEventRecord(L.ev0, st));
    if (in_bytes) FEED_TRY(hipMemcpyAsync(L.d_in.p, L.h_in.p, in_bytes, hipMemcpyHostToDevice, st));
    FEED_TRY(hipEventRecord(L.ev_up, st));
    FEED_TRY(hipEventSynchronize(L.ev_up));
  }
  {
    const long total = ns * ((long)(head >> 2) + ((frames + 3) >> 2) + (pad >> 2));
    long blocks = (total + 255) / 256;
    if (blocks > 256L * 32) blocks = 256L * 32;
    if (blocks < 1) blocks = 1;
    if (L.format == VAMD_FEED_S16)
      hipLaunchKernelGGL(k_feed_ingest<int16_t>, dim3((unsigned)blocks), dim3(256), 0, st, (const int16_t *)L.d_in.p, ch, ns, frames, head, pad,
                         (float *)L.d_pcm.p, ss, cs, (float *)L.d_amp.p, (vamd_envelope_state *)L.d_states.p, d_frames_of, d_first_of);
    else
      hipLaunchKernelGGL(k_feed_ingest<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float *)L.d_in.p, ch, ns, frames, head, pad,
                         (float *)L.d_pcm.p, ss, cs, (float *)L.d_amp.p, (vamd_envelope_state *)L.d_states.p, d_frames_of, d_first_of);
    FEED_TRY(hipGetLastError());
  }
  vamd_stream_plan plan;
  if (uneven)
    FEED_CALL(vamd_plan_streams_whole_v(L.ctx, (float *)L.d_pcm.p, ss, cs, ns, frames, L.frames_of.data(), (vamd_envelope_state *)L.d_states.p, &plan));
  else
    FEED_CALL(vamd_plan_streams_whole(L.ctx, (float *)L.d_pcm.p, ss, cs, ns, frames, (vamd_envelope_state *)L.d_states.p, &plan));
  FeedLive none;
  none.in = nullptr, none.nan = nullptr;
  return finish_group(f, L, plan, (const float *)L.d_pcm.p, ns, ss, cs, d_frames_of, none, ns);
}

// a group from its plan on (whole or live): the analysis, the packets end to end into the pinned arena
static int finish_group(vamd_feed *f, FeedLane &L, const vamd_stream_plan &plan, const float *pcm, long ns, long ss, long cs,
                        const long long *d_frames_of, FeedLive live, long ns_out) {
  const long frames = L.frames;
  const int ch = f->ch, head = f->bs[1] / 2;
  hipStream_t st = L.stream;
  if (f->managed) return run_group_managed(f, L, plan, pcm, ns, ss, cs, d_frames_of, live, ns_out);
  const long nb = (long)(plan.nblocks[0] + plan.nblocks[1]);
  vamd_batch_desc desc[2];
  vamd_batch_io io[2];
  for (int W = 0; W < 2; W++) {
    const size_t n = (size_t)plan.nblocks[W];
    FEED_TRY(L.d_pk[W].need((n ? n : 1) * (size_t)f->pkcap[W]));
    FEED_TRY(L.d_bits[W].need((n ? n : 1) * 4));
    FEED_TRY(L.d_status[W].need((n ? n : 1) * (size_t)ch));
    memset(&desc[W], 0, sizeof(desc[W]));
    memset(&io[W], 0, sizeof(io[W]));
    desc[W].W = W;
    desc[W].nblocks = (long)n;
    desc[W].lW = plan.lW[W], desc[W].nW = plan.nW[W], desc[W].blocktype = plan.blocktype[W];
    if (!n) continue;
    io[W].pcm = pcm;
    io[W].pcm_src = plan.src[W];
    io[W].pcm_channel_stride = cs;
    io[W].packets = (uint8_t *)L.d_pk[W].p;
    io[W].packet_bits = (int32_t *)L.d_bits[W].p;
    io[W].packet_stride = f->pkcap[W];
    io[W].status = (uint8_t *)L.d_status[W].p;
  }
  if (nb)
    FEED_CALL(vamd_analyze_streams_mixed(L.ctx, &desc[0], &io[0], &desc[1], &io[1], plan.order, plan.stream_start, ns, nb,
                                         (float *)L.d_amp.p));
  // the packets end to end, into the pinned arena
  FEED_TRY(L.d_rel.need((size_t)(nb ? nb : 1) * 8));
  FEED_TRY(L.d_sid.need((size_t)(nb ? nb : 1) * 4));
  FEED_TRY(L.d_sbytes.need((size_t)ns * 8));
  FEED_TRY(L.d_soff.need((size_t)(ns + 1) * 8));
  // records: [total | stream_start (ns + 1) | offset (nb) | granulepos (nb) | bits (nb) | info (nb)]
  const size_t o_start = 8, o_off = o_start + (size_t)(ns + 1) * 8, o_gp = o_off + (size_t)nb * 8, o_bits = o_gp + (size_t)nb * 8,
               o_info = o_bits + (size_t)nb * 4, rec_bytes = al(o_info + (size_t)nb, 16);
  FEED_TRY(L.h_rec.need(rec_bytes + rec_bytes / 4));
  FeedPlan P;
  P.order = plan.order, P.stream_start = plan.stream_start;
  for (int W = 0; W < 2; W++) {
    P.src[W] = plan.src[W], P.bits[W] = (const int32_t *)L.d_bits[W].p, P.status[W] = (const uint8_t *)L.d_status[W].p;
    P.packets[W] = (const uint8_t *)L.d_pk[W].p, P.stride[W] = f->pkcap[W], P.bs[W] = f->bs[W];
  }
  P.ch = ch, P.stream_stride = ss, P.eof = head + frames, P.frames_of = d_frames_of, P.head = head;
  P.live = live;
  for (int attempt = 0;; attempt++) {
    uint8_t *hrec = (uint8_t *)L.h_rec.p;
    void *drec = nullptr, *dbytes = nullptr;
    FEED_TRY(hipHostGetDevicePointer(&drec, hrec, 0));
    FEED_TRY(hipHostGetDevicePointer(&dbytes, L.h_out.p, 0));
    FeedOut O;
    uint8_t *dr = (uint8_t *)drec;
    O.total = (int64_t *)dr, O.stream_start = (int64_t *)(dr + o_start), O.offset = (int64_t *)(dr + o_off);
    O.granulepos = (int64_t *)(dr + o_gp), O.bits = (int32_t *)(dr + o_bits), O.info = dr + o_info;
    O.bytes = (uint8_t *)dbytes, O.cap = (int64_t)L.h_out.bytes;
    FEED_OWN(feed_mirror(f, L, O, nb, 0));
    hipLaunchKernelGGL(k_feed_sid, dim3((unsigned)ns), dim3(64), 0, st, plan.stream_start, (int32_t *)L.d_sid.p);
    hipLaunchKernelGGL(k_feed_sizes, dim3((unsigned)ns), dim3(64), 0, st, P, ns, (int64_t *)L.d_rel.p, (int64_t *)L.d_sbytes.p);
    hipLaunchKernelGGL(k_feed_scan, dim3(1), dim3(1024), 0, st, ns, (const int64_t *)L.d_sbytes.p, (int64_t *)L.d_soff.p);
    const long waves = (nb > ns + 1 ? nb : ns + 1);
    hipLaunchKernelGGL(k_feed_copy, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, P, ns, nb, (const int64_t *)L.d_rel.p,
                       (const int64_t *)L.d_soff.p, (const int32_t *)L.d_sid.p, O);
    FEED_TRY(hipGetLastError());
    if (f->ogg) FEED_OWN(run_pager(f, L, plan.stream_start, ns, nb, (const int64_t *)L.d_soff.p + ns));
    FEED_TRY(hipEventRecord(L.ev_end, st));
    FEED_TRY(hipEventSynchronize(L.ev_end));
    const int64_t total = *(const int64_t *)hrec;
    if (total <= (int64_t)L.h_out.bytes) {
      if (f->ogg) FEED_OWN(pager_result(f, L, ns));
      vamd_feed_result &R = L.result;
      R.nstreams = ns_out, R.nblocks = nb;
      R.stream_start = (const int64_t *)(hrec + o_start), R.offset = (const int64_t *)(hrec + o_off);
      R.granulepos = (const int64_t *)(hrec + o_gp), R.bits = (const int32_t *)(hrec + o_bits), R.info = hrec + o_info;
      R.bytes = (const uint8_t *)L.h_out.p, R.total_bytes = total;
      break;
    }
    if (attempt) {
      L.err = "packet arena still too small after growing it";
      return VAMD_EFAULT;
    }
    FEED_TRY(L.h_out.need((size_t)total + (size_t)total / 8));  // the packets are still in HBM: lay them out again
  }
  float up = 0.f, dev = 0.f;
  (void)hipEventElapsedTime(&up, L.ev0, L.ev_up);
  (void)hipEventElapsedTime(&dev, L.ev0, L.ev_end);
  L.result.upload_ms = up, L.result.device_ms = dev;
  return VAMD_OK;
}

// one group of a live lane: the pieces of its streams 0 .. L.nstreams-1 (and 0-frame pieces of its other open streams, which
// then emit nothing: their walks stop where they stood).  Upload -> k_live_begin (fresh streams' states) -> k_live_ingest
// (kept samples + piece into the other buffer) -> vamd_live_plan (stream ends where due, detector over the new steps,
// resumed walk, rebase; its wait brings the block counts and every stream's next rebase home) -> analysis and packets as
// a whole group's.  The host mirror of each stream says what the device holds of it.
static int run_group_live(vamd_feed *f, FeedLane &L) {
  const long nsc = L.nstreams;
  const int ch = f->ch, bs1 = f->bs[1], head = bs1 / 2, pad = 3 * bs1, step = 64;
  long ns = nsc;
  for (long i = nsc; i < f->max_streams; i++)
    if (L.live[(size_t)i].open) ns = i + 1;
  const long cs = f->live_cs, ss = cs * ch;
  const size_t sample = L.format == VAMD_FEED_S16 ? 2 : 4;
  const long n_head = ((long)bs1 / f->write_frames + 1) * f->write_frames;  // lib/block.c:525-526
  hipStream_t st = L.stream;
  FEED_TRY(L.d_live.need((size_t)ns * sizeof(LiveIn)));
  FEED_TRY(L.h_live.need((size_t)ns * (sizeof(LiveIn) + sizeof(vamd_live_geo) + 8)));
  LiveIn *hin = (LiveIn *)L.h_live.p;
  vamd_live_geo *geo = (vamd_live_geo *)(hin + ns);
  long long *shift = (long long *)(geo + ns);
  int64_t first = 0, quads = 0;
  for (long i = 0; i < ns; i++) {
    const int64_t n = i < nsc ? L.frames_of[(size_t)i] : 0;
    const bool cl = i < nsc && L.close_of[(size_t)i];
    FeedLane::LiveStream &m = L.live[(size_t)i];
    LiveIn &in = hin[i];
    vamd_live_geo &g = geo[i];
    memset(&in, 0, sizeof(in));
    memset(&g, 0, sizeof(g));
    in.first = first, in.frames = n;
    first += n;
    in.fresh = !m.open;
    if (!m.open && !n) {  // (a stream starts with its first frame: until then it is not there, and nothing of it is planned)
      in.eof = LIVE_OPEN;
      g.fresh = 1;
      continue;
    }
    if (!m.open) {
      m = FeedLane::LiveStream();
      m.open = true, m.have = head;
      in.keep = head;
    } else {  // the rebase the last walk asked for
      in.shift = m.shift, in.keep = m.have - m.shift;
      m.origin += m.shift, m.steps -= m.shift / step, m.have = in.keep, m.shift = 0;
    }
    in.origin = m.origin;
    m.have += n, m.total += n;
    if (!m.headed && (m.total >= n_head || cl)) {  // the backward extrapolation: lib/block.c:524-528, or the close (:480-481)
      m.headed = true;
      g.n_head = (int)(m.total < n_head ? m.total : n_head);
    }
    g.have = m.have, g.kept = m.steps;
    if (m.headed) {
      const int64_t last = m.have / step - 4;  // lib/envelope.c:223-224
      g.c1 = last > m.steps ? last - m.steps : 0;
    }
    if (cl) {
      const int64_t s1 = m.steps + g.c1, sa = (m.have + pad) / step - 4;
      g.c2 = sa > s1 ? sa - s1 : 0;
    }
    g.fresh = in.fresh, g.close = cl;
    in.close = cl, in.eof = cl ? m.have : LIVE_OPEN;
    m.steps += g.c1;
    if (in.keep + n + pad + 256 > cs) {
      L.err = "live feed: a stream's kept samples and piece exceed its buffer (the retention bound does not hold)";
      return VAMD_EFAULT;
    }
    const int64_t q = (in.keep + n + pad + 256 + 3) / 4;
    if (q > quads) quads = q;
  }
  const size_t in_bytes = (size_t)first * ch * sample;
  FEED_TRY(L.d_in.need(in_bytes ? in_bytes : 16));
  {
    std::lock_guard<std::mutex> turn(*L.upload_turn);  // (run_group: one upload at a time per device)
    FEED_TRY(hipEventRecord(L.ev0, st));
    if (in_bytes) FEED_TRY(hipMemcpyAsync(L.d_in.p, L.h_in.p, in_bytes, hipMemcpyHostToDevice, st));
    FEED_TRY(hipMemcpyAsync(L.d_live.p, hin, (size_t)ns * sizeof(LiveIn), hipMemcpyHostToDevice, st));
    FEED_TRY(hipEventRecord(L.ev_up, st));
    FEED_TRY(hipEventSynchronize(L.ev_up));
  }
  const LiveIn *d_live = (const LiveIn *)L.d_live.p;
  vamd_bitrate_state *bst = f->managed ? (vamd_bitrate_state *)L.d_bstate.p : nullptr;
  if (f->managed && !L.btmpl_ready) {
    FEED_CALL(vamd_bitrate_init_states(L.ctx, (vamd_bitrate_state *)L.d_btmpl.p, 1));
    L.btmpl_ready = true;
  }
  {
    const long words = ns * (long)(sizeof(vamd_envelope_state) / 4);
    hipLaunchKernelGGL(k_live_begin, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, ns, d_live, (vamd_envelope_state *)L.d_states.p,
                       (float *)L.d_amp.p, bst, (const vamd_bitrate_state *)L.d_btmpl.p, (unsigned long long *)L.d_nan.p);
    *(volatile int *)L.h_lstatus.p = 0;
    void *d_lstatus = nullptr;
    FEED_TRY(hipHostGetDevicePointer(&d_lstatus, L.h_lstatus.p, 0));
    long blocks = (ns * quads + 255) / 256;
    if (blocks > 256L * 32) blocks = 256L * 32;
    if (blocks < 1) blocks = 1;
    const float *old = (const float *)L.d_buf[L.cur].p;
    float *pcm = (float *)L.d_buf[1 - L.cur].p;
    if (L.format == VAMD_FEED_S16)
      hipLaunchKernelGGL(k_live_ingest<int16_t>, dim3((unsigned)blocks), dim3(256), 0, st, (const int16_t *)L.d_in.p, ch, ns, (long)quads, pad + 256,
                         d_live, old, pcm, ss, cs, (unsigned long long *)L.d_nan.p, (int *)d_lstatus);
    else
      hipLaunchKernelGGL(k_live_ingest<float>, dim3((unsigned)blocks), dim3(256), 0, st, (const float *)L.d_in.p, ch, ns, (long)quads, pad + 256,
                         d_live, old, pcm, ss, cs, (unsigned long long *)L.d_nan.p, (int *)d_lstatus);
    FEED_TRY(hipGetLastError());
  }
  L.cur = 1 - L.cur;
  float *pcm = (float *)L.d_buf[L.cur].p;
  vamd_stream_plan plan;
  FEED_CALL(vamd_live_plan(L.ctx, pcm, ss, cs, ns, geo, (int)n_head, L.d_walk.p, (unsigned char *)L.d_rows.p, f->row_stride,
                           (vamd_envelope_state *)L.d_states.p, shift, &plan));
  if (*(volatile int *)L.h_lstatus.p) {  // (written by the ingest, mapped; the plan's wait is behind it)
    L.err = "live feed: the ingest found a stream whose samples exceed its buffer";
    return VAMD_EFAULT;
  }
  for (long i = 0; i < ns; i++) {
    FeedLane::LiveStream &m = L.live[(size_t)i];
    if (hin[i].close) {
      m = FeedLane::LiveStream();  // (its next piece starts a fresh stream)
      continue;
    }
    m.shift = shift[i];
    if (m.shift < 0 || m.shift > m.have || m.have - m.shift > f->retain) {
      L.err = "live feed: a stream would keep more samples than the retention bound allows";
      return VAMD_EFAULT;
    }
  }
  FeedLive live;
  live.in = d_live, live.nan = (const unsigned long long *)L.d_nan.p;
  const int r = finish_group(f, L, plan, pcm, ns, ss, cs, nullptr, live, nsc);
  if (!r && L.result.stream_start && L.result.stream_start[nsc] != L.result.nblocks) {
    L.err = "live feed: a stream outside the group emitted blocks";
    return VAMD_EFAULT;
  }
  return r;
}

static void feed_lane_main(vamd_feed *f, FeedLane *lane) {
  FeedLane &L = *lane;
  (void)hipSetDevice(L.device);
  std::unique_lock<std::mutex> g(f->m);
  for (;;) {
    f->cv_work.wait(g, [&] { return f->stop || L.state == LANE_QUEUED; });
    if (f->stop) return;
    g.unlock();
    const int r = f->write_frames ? run_group_live(f, L) : run_group(f, L);
    if (r && f->write_frames)  // (what the device holds of the lane's streams is unknown: they start afresh)
      for (FeedLane::LiveStream &m : L.live) m = FeedLane::LiveStream();
    const double t = now_s();
    g.lock();
    L.status = r;
    L.result.total_ms = (t - L.t_wrote) * 1e3;
    L.state = LANE_DONE;
    if (r) f->err = L.err;
    f->cv_done.notify_all();
  }
}

static void feed_free(vamd_feed *f) {
  {
    std::lock_guard<std::mutex> g(f->m);
    f->stop = true;
  }
  f->cv_work.notify_all();
  f->cv_done.notify_all();
  for (FeedLane &L : f->lanes)
    if (L.worker.joinable()) L.worker.join();
  int cur = 0;
  (void)hipGetDevice(&cur);
  for (FeedLane &L : f->lanes) {
    (void)hipSetDevice(L.device);
    if (L.stream) (void)hipStreamSynchronize(L.stream);
    if (L.ctx) vamd_destroy(L.ctx);
    Buf *all[] = {&L.d_len, &L.h_len, &L.h_in, &L.h_out, &L.h_rec, &L.d_in, &L.d_pcm, &L.d_states, &L.d_amp, &L.d_pk[0], &L.d_pk[1], &L.d_bits[0],
                  &L.d_bits[1], &L.d_status[0], &L.d_status[1], &L.d_rel, &L.d_sid, &L.d_sbytes, &L.d_soff, &L.d_bstate, &L.d_slice, &L.h_slice,
                  &L.d_buf[0], &L.d_buf[1], &L.d_walk, &L.d_rows, &L.d_nan, &L.d_btmpl, &L.d_live, &L.h_live, &L.h_lstatus,
                  &L.d_mirror, &L.d_moff, &L.d_mgp, &L.d_mrbits, &L.d_minfo, &L.d_hdr, &L.d_serial, &L.h_serial, &L.d_pages, &L.d_fbytes,
                  &L.d_foff, &L.d_npages, &L.d_ostatus, &L.h_ogg, &L.h_orec};
    for (int W = 0; W < 2; W++) {
      Buf *m[] = {&L.d_mpk[W], &L.d_mbits[W], &L.d_mposts[W], &L.d_mvalid[W], &L.d_miwork[W], &L.d_mnz[W], &L.d_choice[W], &L.d_fbits[W]};
      for (Buf *b : m) b->drop();
    }
    for (Buf *b : all) b->drop();
    if (L.ev0) (void)hipEventDestroy(L.ev0);
    if (L.ev_up) (void)hipEventDestroy(L.ev_up);
    if (L.ev_end) (void)hipEventDestroy(L.ev_end);
    if (L.stream) (void)hipStreamDestroy(L.stream);
  }
  (void)hipSetDevice(cur);
  f->lanes.clear();
}

// why this thread's last vamd_feed_create failed (vamd_feed_last_error(NULL))
thread_local std::string feed_create_err;

static int feed_create(vamd_feed **out, const void *setup_blob, size_t blob_bytes, const int *devices, int ndevices,
                       int lanes_per_device, long max_streams, long max_frames, int format, int write_frames) {
  if (!out) return VAMD_EINVAL;
  *out = nullptr;
  if (!setup_blob || lanes_per_device < 1 || lanes_per_device > 8 || max_streams < 1 || max_frames < 1 || ndevices < 0 ||
      ndevices > 64 || (ndevices > 0 && !devices) || (format != VAMD_FEED_S16 && format != VAMD_FEED_F32) || write_frames < 0)
    return VAMD_EINVAL;
  feed_create_err.clear();
  // a bitrate-managed setup is fed through its manager (run_group_managed), which needs the blob's manager section; a
  // managed blob packed before the section existed would otherwise get the VBR candidate of every block
  vamd_setup_header h;
  memset(&h, 0, sizeof(h));
  if (blob_bytes >= sizeof(h)) memcpy(&h, setup_blob, sizeof(h));
  if (h.managed && !h.off_bitrate) {
    feed_create_err = "bitrate-managed setup blob without the bitrate manager's section (packed before it existed): repack it with vamd_pack_setup";
    return VAMD_EIMPL;
  }
  int cur = 0;
  if (hipGetDevice(&cur) != hipSuccess) return VAMD_EFAULT;
  std::vector<int> devs;
  if (ndevices == 0) devs.push_back(cur);
  for (int i = 0; i < ndevices; i++) devs.push_back(devices[i] >= 0 ? devices[i] : cur);
  vamd_feed *f = new vamd_feed;
  f->max_streams = max_streams, f->max_frames = max_frames, f->format = format, f->write_frames = write_frames;
  f->managed = h.managed && h.off_bitrate;
  f->rate = h.rate;
  {
    const vamd::Knobs K = vamd::read_knobs();
    f->slice = K.feed_slice > 0 ? K.feed_slice : 2048;
  }
  f->lanes.resize(devs.size() * (size_t)lanes_per_device);
  for (size_t d = 0; d < devs.size(); d++) f->upload_turns.emplace_back(new std::mutex);
  int r = VAMD_OK;
  // lane l runs on device l % ndevices: consecutive groups go to different devices first, to a device's next lane after
  for (size_t l = 0; l < f->lanes.size() && !r; l++) {
    FeedLane &L = f->lanes[l];
    L.device = devs[l % devs.size()];
    L.upload_turn = f->upload_turns[l % devs.size()].get();
    L.h_in.host = L.h_out.host = L.h_rec.host = L.h_len.host = L.h_slice.host = L.h_live.host = L.h_lstatus.host = true;
    L.h_ogg.host = L.h_orec.host = L.h_serial.host = true;
    r = vamd_create(&L.ctx, setup_blob, blob_bytes, L.device);
    if (r) break;
    hipError_t e = hipSetDevice(L.device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L.ev0, hipEventDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L.ev_up, hipEventBlockingSync);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L.ev_end, hipEventBlockingSync);
    if (e == hipSuccess && vamd_set_stream(L.ctx, L.stream) != VAMD_OK) e = hipErrorUnknown;
    if (e == hipSuccess && l == 0) {
      f->ch = vamd_channels(L.ctx);
      for (int W = 0; W < 2; W++) f->bs[W] = vamd_blocksize(L.ctx, W), f->pkcap[W] = vamd_packet_capacity(L.ctx, W);
      if (f->pkcap[0] <= 0 || f->pkcap[1] <= 0) r = VAMD_EIMPL;  // packets of this mode are not assembled on the GPU
      if (!r && write_frames) {
        const char *why = vamd_live_check(L.ctx, write_frames, max_frames);
        if (why) {
          feed_create_err = why;
          r = VAMD_EIMPL;
        }
        f->retain = vamd_live_retain(L.ctx, write_frames);
        f->live_cs = (long)al((size_t)(2 * f->retain + max_frames + 3 * f->bs[1] + 512), 64);
        f->row_stride = f->live_cs / 64 + 16;
      }
    }
    if (e == hipSuccess && !r && write_frames) {  // a live lane's device state, for every stream it may carry
      const size_t ns = (size_t)max_streams;
      for (int b = 0; b < 2 && e == hipSuccess; b++) e = L.d_buf[b].need(ns * f->ch * (size_t)f->live_cs * 4);
      if (e == hipSuccess) e = L.d_walk.need(ns * VAMD_LIVE_WALK_BYTES);
      if (e == hipSuccess) e = L.d_rows.need(ns * (size_t)f->row_stride);
      if (e == hipSuccess) e = L.d_nan.need(ns * 8);
      if (e == hipSuccess) e = L.d_states.need(ns * sizeof(vamd_envelope_state));
      if (e == hipSuccess) e = L.d_amp.need(ns * 4);
      if (e == hipSuccess) e = L.d_bstate.need(ns * sizeof(vamd_bitrate_state));
      if (e == hipSuccess) e = L.d_btmpl.need(sizeof(vamd_bitrate_state));
      if (e == hipSuccess) e = L.h_lstatus.need(64);
      L.live.resize(ns);
    }
    // the arenas: the group's samples; packets: half the samples' size AS 16-BIT to start with (a q 0.4 stream is a
    // tenth of that, q 1.0 on noise a third; run_group grows the arena when a group needs more)
    const size_t in_cap = (size_t)max_streams * max_frames * f->ch * (format == VAMD_FEED_S16 ? 2 : 4);
    if (e == hipSuccess && !r) e = L.h_in.need(in_cap);
    if (e == hipSuccess && !r) e = L.h_out.need(al((size_t)max_streams * max_frames * f->ch + (size_t)max_streams * 65536, 4096));
    if (e != hipSuccess) r = VAMD_EFAULT;
  }
  (void)hipSetDevice(cur);
  if (!r) {
    try {
      for (FeedLane &L : f->lanes) L.worker = std::thread(feed_lane_main, f, &L);
    } catch (...) {
      r = VAMD_EFAULT;
    }
  }
  if (r) {
    if (feed_create_err.empty())
      feed_create_err = f->lanes.empty() || !f->lanes[0].ctx ? "vamd_create failed (setup blob refused, or a HIP failure)"
                                                                : "the setup's packets are not assembled on the GPU, or a HIP failure";
    feed_free(f);
    delete f;
    return r;
  }
  *out = f;
  return VAMD_OK;
}

// an Ogg feed's group (f->m held): its serial numbers -- the next nstreams of the feed's running counter, then what
// vamd_feed_ogg_serials set for the slot in their place
static void ogg_job(vamd_feed *f, FeedLane &L, long nstreams) {
  memset(&L.ogg_result, 0, sizeof(L.ogg_result));
  if (!f->ogg) return;
  L.serials.resize((size_t)nstreams);
  for (long s = 0; s < nstreams; s++) L.serials[(size_t)s] = f->next_serial++;
  for (size_t s = 0; s < L.user_serials.size() && s < (size_t)nstreams; s++) L.serials[s] = L.user_serials[s];
  L.user_serials.clear();
}

static uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

extern "C" {

int vamd_feed_ogg_headers(vamd_feed *f, const void *id, long id_bytes, const void *comment, long comment_bytes, const void *setup,
                          long setup_bytes) {
  if (!f) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  if (f->write_frames) {
    f->err = "Ogg files of a live feed are not implemented (a page may span two groups)";
    return VAMD_EIMPL;
  }
  if (f->turn) {
    f->err = "vamd_feed_ogg_headers comes before the first vamd_feed_buffer";
    return VAMD_EINVAL;
  }
  const uint8_t *pk[3] = {(const uint8_t *)id, (const uint8_t *)comment, (const uint8_t *)setup};
  const long n[3] = {id_bytes, comment_bytes, setup_bytes};
  for (int i = 0; i < 3; i++)
    if (!pk[i] || n[i] < 7 || n[i] > (1L << 24) || pk[i][0] != 1 + 2 * i || memcmp(pk[i] + 1, "vorbis", 6)) {
      f->err = std::string("Ogg headers: packet ") + std::to_string(i) + " is not a Vorbis header of type " + std::to_string(1 + 2 * i);
      return VAMD_EINVAL;
    }
  if (id_bytes != 30) {
    f->err = "Ogg headers: the identification header is not 30 bytes";
    return VAMD_EINVAL;
  }
  const uint8_t *h = pk[0];
  const long hch = h[11], hrate = (long)le32(h + 12);
  const int b0 = 1 << (h[28] & 15), b1 = 1 << (h[28] >> 4);
  if (le32(h + 7) != 0 || !(h[29] & 1)) {
    f->err = "Ogg headers: the identification header's version or framing bit is wrong";
    return VAMD_EINVAL;
  }
  if (hch != f->ch || hrate != f->rate || b0 != f->bs[0] || b1 != f->bs[1]) {
    f->err = "Ogg headers: identification header (" + std::to_string(hch) + " ch, " + std::to_string(hrate) + " Hz, blocks " + std::to_string(b0) +
             "/" + std::to_string(b1) + ") is not the setup's (" + std::to_string(f->ch) + " ch, " + std::to_string(f->rate) + " Hz, blocks " +
             std::to_string(f->bs[0]) + "/" + std::to_string(f->bs[1]) + ")";
    return VAMD_EINVAL;
  }
  for (int i = 0; i < 3; i++) f->ogg_hdr[i].assign(pk[i], pk[i] + n[i]);
  f->ogg = true;
  return VAMD_OK;
}

int vamd_feed_ogg_serials(vamd_feed *f, int slot, const uint32_t *serials, long n) {
  if (!f || !serials || n < 0 || slot < 0 || slot >= (int)f->lanes.size()) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  FeedLane &L = f->lanes[(size_t)slot];
  if (!f->ogg || L.state != LANE_FILLING || n > f->max_streams) {
    f->err = "vamd_feed_ogg_serials: an Ogg feed's slot between vamd_feed_buffer and vamd_feed_wrote, at most max_streams numbers";
    return VAMD_EINVAL;
  }
  L.user_serials.assign(serials, serials + n);
  return VAMD_OK;
}

int vamd_feed_ogg(vamd_feed *f, int slot, vamd_feed_ogg_result *out) {
  if (!f || !out || slot < 0 || slot >= (int)f->lanes.size()) return VAMD_EINVAL;
  std::unique_lock<std::mutex> g(f->m);
  if (!f->ogg) {
    f->err = "vamd_feed_ogg: the feed has no Ogg headers (vamd_feed_ogg_headers)";
    return VAMD_EINVAL;
  }
  FeedLane &L = f->lanes[(size_t)slot];
  if (L.state != LANE_QUEUED && L.state != LANE_DONE) return VAMD_EINVAL;
  f->cv_done.wait(g, [&] { return f->stop || L.state == LANE_DONE; });
  if (L.state != LANE_DONE) return VAMD_EFAULT;
  *out = L.ogg_result;
  return L.status;
}

int vamd_feed_create(vamd_feed **out, const void *setup_blob, size_t blob_bytes, const int *devices, int ndevices,
                     int lanes_per_device, long max_streams, long max_frames, int format) {
  return feed_create(out, setup_blob, blob_bytes, devices, ndevices, lanes_per_device, max_streams, max_frames, format, 0);
}

int vamd_feed_create_live(vamd_feed **out, const void *setup_blob, size_t blob_bytes, const int *devices, int ndevices,
                          int lanes_per_device, long max_streams, long max_frames, int format, int write_frames) {
  if (write_frames < 1) {
    if (out) *out = nullptr;
    return VAMD_EINVAL;
  }
  return feed_create(out, setup_blob, blob_bytes, devices, ndevices, lanes_per_device, max_streams, max_frames, format, write_frames);
}

void vamd_feed_destroy(vamd_feed *f) {
  if (!f) return;
  feed_free(f);
  delete f;
}

int vamd_feed_lanes(const vamd_feed *f) { return f ? (int)f->lanes.size() : VAMD_EINVAL; }

int vamd_feed_device(const vamd_feed *f, int slot) {
  return (f && slot >= 0 && slot < (int)f->lanes.size()) ? f->lanes[(size_t)slot].device : VAMD_EINVAL;
}

int vamd_feed_buffer(vamd_feed *f, void **pcm) {
  if (!f || !pcm) return VAMD_EINVAL;
  std::unique_lock<std::mutex> g(f->m);
  for (;;) {
    if (f->stop) return VAMD_EFAULT;
    int best = -1;
    for (size_t l = 0; l < f->lanes.size(); l++)
      if (f->lanes[l].state == LANE_FREE && (best < 0 || f->lanes[l].served < f->lanes[(size_t)best].served)) best = (int)l;
    if (best >= 0) {
      FeedLane &L = f->lanes[(size_t)best];
      L.state = LANE_FILLING;
      L.served = ++f->turn;
      *pcm = L.h_in.p;
      return best;
    }
    // every lane is out: wait for a release -- unless nothing can release one (all handed out and none queued or done
    // would be the caller waiting for itself)
    bool hope = false;
    for (const FeedLane &L : f->lanes) hope |= L.state == LANE_QUEUED || L.state == LANE_DONE;
    if (!hope) return VAMD_EINVAL;
    f->cv_done.wait(g);
  }
}

int vamd_feed_wrote(vamd_feed *f, int slot, long nstreams, long frames) {
  if (!f || slot < 0 || slot >= (int)f->lanes.size() || f->write_frames) return VAMD_EINVAL;
  if (nstreams < 1 || nstreams > f->max_streams || frames < 1 || frames > f->max_frames) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  FeedLane &L = f->lanes[(size_t)slot];
  if (L.state != LANE_FILLING) return VAMD_EINVAL;
  L.nstreams = nstreams, L.frames = frames, L.format = f->format;
  L.frames_of.clear();
  L.status = 0;
  memset(&L.result, 0, sizeof(L.result));
  ogg_job(f, L, nstreams);
  L.t_wrote = now_s();
  L.state = LANE_QUEUED;
  f->cv_work.notify_all();
  return VAMD_OK;
}

int vamd_feed_wrote_v(vamd_feed *f, int slot, long nstreams, const int64_t *frames) {
  if (!f || !frames || slot < 0 || slot >= (int)f->lanes.size() || f->write_frames) return VAMD_EINVAL;
  if (nstreams < 1 || nstreams > f->max_streams) return VAMD_EINVAL;
  long longest = 0;
  long long total = 0;
  for (long i = 0; i < nstreams; i++) {
    if (frames[i] < 1 || frames[i] > f->max_frames) return VAMD_EINVAL;
    if (frames[i] > longest) longest = (long)frames[i];
    total += frames[i];
  }
  if (total > (long long)f->max_streams * f->max_frames) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  FeedLane &L = f->lanes[(size_t)slot];
  if (L.state != LANE_FILLING) return VAMD_EINVAL;
  L.nstreams = nstreams, L.frames = longest, L.format = f->format;
  L.frames_of.assign(frames, frames + nstreams);
  L.status = 0;
  memset(&L.result, 0, sizeof(L.result));
  ogg_job(f, L, nstreams);
  L.t_wrote = now_s();
  L.state = LANE_QUEUED;
  f->cv_work.notify_all();
  return VAMD_OK;
}

int vamd_feed_wrote_live(vamd_feed *f, int slot, long nstreams, const int64_t *frames, const uint8_t *close) {
  if (!f || !frames || slot < 0 || slot >= (int)f->lanes.size() || !f->write_frames) return VAMD_EINVAL;
  if (nstreams < 1 || nstreams > f->max_streams) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  FeedLane &L = f->lanes[(size_t)slot];
  if (L.state != LANE_FILLING) return VAMD_EINVAL;
  for (long i = 0; i < nstreams; i++) {
    if (frames[i] < 0 || frames[i] > f->max_frames) return VAMD_EINVAL;
    if (close && close[i] && !frames[i] && !L.live[(size_t)i].open) return VAMD_EINVAL;  // (closing a stream that never had a frame)
  }
  L.nstreams = nstreams, L.frames = f->max_frames, L.format = f->format;
  L.frames_of.assign(frames, frames + nstreams);
  L.close_of.assign((size_t)nstreams, 0);
  if (close)
    for (long i = 0; i < nstreams; i++) L.close_of[(size_t)i] = close[i] != 0;
  L.status = 0;
  memset(&L.result, 0, sizeof(L.result));
  L.t_wrote = now_s();
  L.state = LANE_QUEUED;
  f->cv_work.notify_all();
  return VAMD_OK;
}

int vamd_feed_packets(vamd_feed *f, int slot, vamd_feed_result *out) {
  if (!f || !out || slot < 0 || slot >= (int)f->lanes.size()) return VAMD_EINVAL;
  std::unique_lock<std::mutex> g(f->m);
  FeedLane &L = f->lanes[(size_t)slot];
  if (L.state != LANE_QUEUED && L.state != LANE_DONE) return VAMD_EINVAL;
  f->cv_done.wait(g, [&] { return f->stop || L.state == LANE_DONE; });
  if (L.state != LANE_DONE) return VAMD_EFAULT;
  *out = L.result;
  return L.status;
}

int vamd_feed_release(vamd_feed *f, int slot) {
  if (!f || slot < 0 || slot >= (int)f->lanes.size()) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  FeedLane &L = f->lanes[(size_t)slot];
  if (L.state != LANE_DONE && L.state != LANE_FILLING) return VAMD_EINVAL;
  L.user_serials.clear();
  L.state = LANE_FREE;
  f->cv_done.notify_all();
  return VAMD_OK;
}

const char *vamd_feed_last_error(const vamd_feed *f) { return f ? f->err.c_str() : feed_create_err.c_str(); }

}  // extern "C"
