// k_feed.h -- the kernels of the host-fed farm (vamd_feed.hip is their host side): the ingest of a group's samples (whole
// streams: k_feed_ingest; a live lane's continuing streams: k_live_begin, k_live_ingest; either from tensors that already lie
// in HBM: k_feed_ingest_dev, k_live_ingest_dev over k_feed_src.h) and the packet hand-over -- the
// analysis' packets laid end to end into the pinned output arena, their records beside them: per-stream sizes (a wave per
// stream), a scan over the streams, and a wave per packet that copies its words across the link.  The hand-over takes a run
// of packets in stream order (FeedSlice): a whole VBR group, or one slice of a bitrate-managed group.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "vorbis_amd.h"
#include "k_feed_src.h"
#include "vamd_feed_host.h"

namespace vamd {

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
// (LiveIn, LIVE_OPEN, LIVE_NO_NAN: vamd_feed_host.h, beside the host mirror that builds them)

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

// ---- a DEVICE-fed group (vamd_feed_wrote_device / _wrote_live_device): the same buffers from a caller's tensors ----
// T: int16_t, float, src_f16 or src_bf16 (k_feed_src.h); stream s reads element (c, k) at base + c * cstride + k * fstride.
// k_feed_ingest's layout and work split: a thread owns four frames of every channel and stores 16 bytes per channel;
// consecutive threads own consecutive quads, so with fstride == 1 a wave reads 64 quads of one channel row back to back
// (1 KB of floats, 512 B of a 16-bit type), each quad in one load where its address is aligned to it (src_quad).  The
// streams' lengths and base pointers come in one list, [frames_of (nstreams) | base_of (nstreams)] (the lane's d_len).
template <typename T>
__global__ void k_feed_ingest_dev(int ch, long nstreams, long frames, int head, int pad, float *__restrict__ pcm, long ss, long cs,
                                  float *__restrict__ amp, vamd_envelope_state *__restrict__ states, const long long *__restrict__ frames_of,
                                  const long long *__restrict__ base_of, int64_t cstride, int64_t fstride) {
  const long per = (head >> 2) + ((frames + 3) >> 2) + (pad >> 2), total = nstreams * per;
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x)
    feed_ingest_dev_item<T>(t, ch, frames, head, pad, pcm, ss, cs, amp, VAMD_AMPMAX_FLOOR, frames_of, base_of, cstride, fstride, true);
  // a fresh detector state per stream (all-zero == a stream's start, include/vorbis_amd.h)
  const long words = nstreams * (long)(sizeof(vamd_envelope_state) / 4);
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < words; t += (long)gridDim.x * blockDim.x) ((uint32_t *)states)[t] = 0u;
}

// k_live_ingest with the piece of stream s at the base pointer that LiveIn::first carries (frame 0 of the piece, channel 0).
// The float types: the first non-finite sample of each stream is recorded, as for VAMD_FEED_F32.  A quad that lies whole in
// the piece goes through src_quad (one load where consecutive and aligned); a quad across an edge is put together by element.
template <typename T>
__global__ void k_live_ingest_dev(int ch, long nstreams, long quads, int room, const LiveIn *__restrict__ li, const float *__restrict__ old,
                                  float *__restrict__ pcm, long ss, long cs, unsigned long long *__restrict__ nan, int *__restrict__ status,
                                  int64_t cstride, int64_t fstride) {
  for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < nstreams * quads; t += (long)gridDim.x * blockDim.x) {
    const long s = t / quads, p0 = (t - s * quads) << 2;
    const LiveIn L = li[s];
    const long data = L.keep + L.frames, end = data + room < cs ? data + room : cs;
    if (data + room > cs || L.keep < 0 || L.shift < 0 || L.shift + L.keep > cs) {
      if (p0 == 0) *(volatile int *)status = 1;  // (host memory, mapped: a plain store)
      continue;
    }
    if (p0 >= end) continue;
    const T *base = (const T *)(uintptr_t)L.first;
    for (int c = 0; c < ch; c++) {
      float v[4];
      const T *row = base + (int64_t)c * cstride;
      if (p0 >= L.keep && p0 + 4 <= data) src_quad(row, (int64_t)(p0 - L.keep), fstride, 4, true, v);
      else {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const long p = p0 + k;
          float x = 0.f;
          if (p < L.keep) {
            if (!L.fresh) x = old[s * ss + (long)c * cs + L.shift + p];
          } else if (p < data) x = src_float(row[(int64_t)(p - L.keep) * fstride]);
          v[k] = x;
        }
      }
      src_store4(pcm + s * ss + (long)c * cs + p0, v[0], v[1], v[2], v[3]);
      if (src_has_non_finite<T>()) {
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const long p = p0 + k;
          if (p >= L.keep && p < data && src_non_finite(v[k])) {
            atomicMin(nan + s, (unsigned long long)(L.origin + p));
            break;
          }
        }
      }
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

// A run of packets in stream order, and what the hand-over kernels need of it: its blocks (order[] into the run's own
// batches, stream_start over the run's pieces of streams), their rows, bit counts and status -- and of the group: the
// plan's stream_start, src and the streams' lengths, for the records.  A slice of a bitrate-managed group
// (run_group_managed) is such a run: fifteen candidate rows per block, the walk's choice among them and the size it hands
// out.  A VBR group is the run that is the whole group: i0 = {0, 0}, k0 = 0, s0 = 0, g_start = stream_start, one row per
// block whose bit count is what is handed out (fbits = the analysis' packet_bits; choice and mbits unused).
struct FeedSlice {
  const int32_t *order;          // [run blocks] W << 30 | index in the run's batch of class W
  const int64_t *stream_start;   // [run streams + 1] into order[]
  const int64_t *g_start;        // the plan's stream_start (whole group)
  const int64_t *src[2];         // the plan's src[W] (whole group)
  const int32_t *choice[2], *fbits[2], *mbits[2];  // [run batch] / [run batch] / [run batch][15]
  const uint8_t *status[2];
  const uint8_t *packets[2];     // [run batch][stride], managed: [run batch][15][stride]
  int64_t stride[2];
  int64_t i0[2];                 // the run's first block of class W in the plan's batches
  int64_t k0;                    // ... and its first block in the plan's order[]
  long s0;                       // the group stream of the run's first stream
  int bs[2];
  int ch;
  int64_t stream_stride, eof;    // eof: first sample past the stream's real ones, in its buffer's coordinates
  const long long *frames_of;    // streams of unequal length: eof = head + frames_of[s]
  int head;
  FeedLive live;                 // a live group's streams (in == null: whole streams)
};

// packet k of the run, in its stream ls: its size class, its index in the run's batch, and its status -- the channels'
// OR'ed, and a live stream's non-finite mark.  A packet with a status is not handed out (0 bytes, bits -1).
struct FeedPacket {
  int W, i;
  unsigned st;
};
__device__ __forceinline__ FeedPacket feed_packet(const FeedSlice &P, int64_t k, long ls) {
  const int o = P.order[k];
  FeedPacket p;
  p.W = (o >> 30) & 1, p.i = o & 0x3fffffff, p.st = 0;
  for (int c = 0; c < P.ch; c++) p.st |= P.status[p.W][(int64_t)p.i * P.ch + c];
  const long s = P.s0 + ls;
  p.st |= live_status(P.live, s, P.src[p.W][P.i0[p.W] + p.i] - s * P.stream_stride, P.bs[p.W]);
  return p;
}

// a wave per stream of the run: rel[k] = bytes (each handed-out packet rounded up to 4) of the stream's packets before k
__global__ __launch_bounds__(64) void k_feed_sizes(FeedSlice P, int64_t *__restrict__ rel, int64_t *__restrict__ stream_bytes) {
  const long s = blockIdx.x;
  const int lane = threadIdx.x;
  const int64_t k0 = P.stream_start[s], k1 = P.stream_start[s + 1];
  int64_t run = 0;
  for (int64_t base = k0; base < k1; base += 64) {
    const int64_t k = base + lane;
    int bytes = 0;
    if (k < k1) {
      const FeedPacket p = feed_packet(P, k, s);
      bytes = p.st ? 0 : (((P.fbits[p.W][p.i] + 7) >> 3) + 3) & ~3;
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

// where the packets and their records go: the output arena and the group's record (host memory, mapped)
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

// the record of packet k of the run, at its place in the group (k0 + k), by one lane of the packet's wave: where it lies,
// the bits handed out, its granule position, and info = W | last << 1 | status << 2 | choice << 4 (choice: the bitrate
// manager's candidate, 0 on a VBR setup) -- and the same into the Ogg mirror's records
__device__ __forceinline__ void feed_record(const FeedSlice &P, const FeedOut &O, int64_t k, long ls, const FeedPacket &p, int64_t off,
                                            int bits, int choice) {
  const long s = P.s0 + ls;
  const int64_t g = P.k0 + k;
  const int64_t begin = P.src[p.W][P.i0[p.W] + p.i] - (int64_t)s * P.stream_stride, center = begin + P.bs[p.W] / 2;
  const bool last = g + 1 == P.g_start[s + 1] && (!P.live.in || P.live.in[s].close);
  const int64_t eof = P.live.in ? P.live.in[s].eof : (P.frames_of ? (int64_t)P.head + P.frames_of[s] : P.eof);
  const int64_t gp = (center < eof ? center : eof) - P.bs[1] / 2 + (P.live.in ? P.live.in[s].origin : 0);
  const uint8_t info = (uint8_t)(p.W | (last ? 2 : 0) | ((p.st & 3) << 2) | ((p.st ? 0 : choice) << 4));
  O.offset[g] = off;
  O.bits[g] = p.st ? -1 : bits;
  O.granulepos[g] = gp;
  O.info[g] = info;
  if (O.m_bytes) O.m_off[g] = off, O.m_bits[g] = p.st ? -1 : bits, O.m_gp[g] = gp, O.m_info[g] = info;
}

// a VBR group, a wave per packet: its words into the output arena, its record beside them -- and the group's total and
// stream_start, so that the host waits once
__global__ __launch_bounds__(256) void k_feed_copy(FeedSlice P, long nstreams, long nblocks, const int64_t *__restrict__ rel,
                                                   const int64_t *__restrict__ stream_off, const int32_t *__restrict__ sid,
                                                   FeedOut O) {
  const long k = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k == 0 && lane == 0) *O.total = stream_off[nstreams];
  if (k <= nstreams && lane == 1) O.stream_start[k] = P.stream_start[k];  // (nstreams + 1 <= nblocks + 1 entries; see the launch)
  if (k >= nblocks) return;
  const int s = sid[k];
  const FeedPacket p = feed_packet(P, k, s);
  const int bits = P.fbits[p.W][p.i], words = p.st ? 0 : (((bits + 7) >> 3) + 3) >> 2;
  const int64_t off = stream_off[s] + rel[k];
  const bool fits = off + 4 * (int64_t)words <= O.cap;
  if (fits) {
    const uint32_t *src = (const uint32_t *)(P.packets[p.W] + (int64_t)p.i * P.stride[p.W]);
    uint32_t *dst = (uint32_t *)(O.bytes + off);
    uint32_t *mir = O.m_bytes ? (uint32_t *)(O.m_bytes + off) : nullptr;
    for (int w = lane; w < words; w += 64) {
      const uint32_t v = src[w];
      dst[w] = v;
      if (mir) mir[w] = v;
    }
  }
  if (lane == 0) feed_record(P, O, k, s, p, off, bits, 0);
}

// sid[k] = the stream packet k belongs to (a wave per stream)
__global__ __launch_bounds__(64) void k_feed_sid(const int64_t *__restrict__ stream_start, int32_t *__restrict__ sid) {
  const long s = blockIdx.x;
  for (int64_t k = stream_start[s] + threadIdx.x; k < stream_start[s + 1]; k += 64) sid[k] = (int32_t)s;
}

// a slice of a bitrate-managed group, a wave per packet: the chosen candidate's first bytes, zero bytes behind them up to
// the handed-out size (the manager's padding) and to the next multiple of 4, into the output arena at base + stream_off +
// rel; the record of the packet at its place in the group
__global__ __launch_bounds__(256) void k_feed_copy_managed(FeedSlice P, long nblocks, int64_t base, const int64_t *__restrict__ rel,
                                                           const int64_t *__restrict__ stream_off, const int32_t *__restrict__ sid,
                                                           FeedOut O) {
  const long k = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (k >= nblocks) return;
  const int ls = sid[k];
  const FeedPacket p = feed_packet(P, k, ls);
  const int W = p.W, i = p.i;
  const unsigned st = p.st;
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
  if (lane == 0) feed_record(P, O, k, ls, p, off, fbits, choice);
}

}  // namespace vamd
