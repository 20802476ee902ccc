// vamd_decode_live_plan.h -- the host half of the live decoder (vamd_decode_live.h; include/vorbis_amd.h:
// vamd_decode_live_plan, vamd_decode_live_wrote): what a slot holds between calls, and the plan of a call -- the
// DecodePlan of its pieces with each continuing stream's carried block in front of its blocks.  Plain C++, no HIP: the
// library and the one-lane test program (tests/c/decode_live_host.cpp) share it.
#pragma once
#include "vamd_decode_plan.h"
#include "k_synth.h"

namespace vamd {

// A slot between calls.  The carried block's second half lies on the device (CarryP::carry, the slot's row).
struct LiveSlot {
  bool open = false;  // a stream is under way: its first piece has been seen, no piece has closed it
  uint8_t dead = 0;   // the VAMD_STATUS_* of its flagged packets: no frames until a piece closes it
  int carry = -1;     // the size class of its last block, -1: no block yet
  int64_t total = 0;  // the frames handed out since it opened
};

// The plan of a call.  P.order, P.lap_start and P.src[W] hold the carried blocks too -- P.extra[W] rows of size class W
// behind the P.nblocks[W] unpacked ones, each with its centre at 0 (src = -bs[W]/2) -- so that k_lap and lap_sample run
// on it as on a whole-stream plan.  The blocks that have a packet are named once more, without the carried ones, for
// k_unpack and the statuses: unpack / unpack_start, and P.packet beside unpack.
struct DecodeLivePlan {
  DecodePlan P;
  std::vector<int32_t> unpack;        // W << 30 | index inside W's batch, stream after stream
  std::vector<int64_t> unpack_start;  // [nstreams + 1] into unpack[]
  std::vector<CarryRow> in, out;      // k_decode_carry_in's and k_decode_carry_out's tables
  std::vector<LiveSlot> next;         // [nstreams] the slot behind this call, unless a packet is flagged on the device
};

// -> false with a reason for a bad descriptor.  Reads `slots` ([max_streams]) and changes nothing.  Every index the two
// carry kernels use -- the slots, the extra rows, the last blocks' rows -- is set here and checked before it returns.
// first: NULL, or per packet its first byte, as decode_plan_build takes them (the live Ogg decoder's packets lie together
// on the device alone: vamd_demux_live.h); `bytes` is not read then.
inline bool decode_live_plan_build(const int bs[2], int modes, int modebits, const std::vector<LiveSlot> &slots, int64_t nstreams, int64_t npackets,
                                   const int64_t *slot, const uint8_t *bytes, const int64_t *offset, const int64_t *stream_start,
                                   const uint8_t *close, const int64_t *end_granule, DecodeLivePlan *L, std::string *err,
                                   const uint8_t *first = nullptr) {
  *L = DecodeLivePlan();
  DecodePlan &P = L->P;
  const int64_t max_streams = (int64_t)slots.size();
  if (!decode_desc_check(nstreams, npackets, bytes, offset, stream_start, end_granule, first, err)) return false;
  if (nstreams > max_streams) return *err = "decode_live: more streams than the decoder has slots", false;
  if (nstreams && !slot) return *err = "decode_live: null slot", false;
  std::vector<uint8_t> named((size_t)max_streams, 0);
  for (int64_t s = 0; s < nstreams; s++) {
    if (slot[s] < 0 || slot[s] >= max_streams) return *err = "decode_live: a slot outside 0 .. max_streams-1", false;
    if (named[(size_t)slot[s]]++) return *err = "decode_live: a slot named twice", false;
  }
  P.frames.assign((size_t)nstreams, 0);
  P.status.assign((size_t)nstreams, 0);
  P.lap_start.assign((size_t)nstreams + 1, 0);
  L->unpack_start.assign((size_t)nstreams + 1, 0);
  L->next.assign((size_t)nstreams, LiveSlot());
  std::vector<int64_t> extra_src[2];
  std::vector<size_t> extra_at;  // the carried blocks' places in order[]: their rows are known once nblocks[] is
  std::vector<int> cls;
  for (int64_t s = 0; s < nstreams; s++) {
    const LiveSlot &was = slots[(size_t)slot[s]];
    LiveSlot now = was;
    now.open = true;
    const int64_t p0 = stream_start[s], p1 = stream_start[s + 1];
    cls.clear();
    uint8_t st = now.dead;
    for (int64_t p = p0; p < p1; p++) {
      const int W = decode_packet_class(first ? first + p : bytes + offset[p], offset[p + 1] - offset[p], modes, modebits);
      if (W < 0) st |= (uint8_t)-W;
      cls.push_back(W);
    }
    P.status[(size_t)s] = now.dead = st;
    if (!st && p1 > p0) {
      int lW = now.carry;
      int64_t at = 0, step = 0;
      if (lW >= 0) {  // the carried block, its centre at 0
        extra_at.push_back(P.order.size());
        P.order.push_back((int32_t)(lW << 30) | (int32_t)P.extra[lW]++);
        extra_src[lW].push_back(-(int64_t)(bs[lW] / 2));
        L->in.push_back(CarryRow{(int)slot[s], lW, -1});
      }
      for (int64_t p = p0; p < p1; p++) {
        const int W = cls[(size_t)(p - p0)];
        step = lW >= 0 ? decode_step(bs, lW, W) : 0;
        at += step;
        if (P.nblocks[W] >= (1 << 30) - max_streams) return *err = "decode: more than 2^30 blocks of a size class", false;
        const int32_t o = (int32_t)(W << 30) | (int32_t)P.nblocks[W]++;
        P.order.push_back(o);
        L->unpack.push_back(o);
        P.src[W].push_back(at - bs[W] / 2);
        P.packet.push_back(p);
        lW = W;
      }
      int64_t frames = at;
      now.total += frames;
      if (close && close[s] && end_granule && end_granule[s] >= 0 && end_granule[s] < now.total) frames -= std::min(now.total - end_granule[s], step);
      now.carry = lW;
      L->out.push_back(CarryRow{(int)slot[s], lW, (int)(P.nblocks[lW] - 1)});
      P.frames[(size_t)s] = frames;
      P.max_frames = std::max(P.max_frames, frames);
    }
    if (close && close[s]) {
      now = LiveSlot();
      if (!st && p1 > p0) L->out.pop_back();  // (a stream that closes leaves no carry)
    }
    L->next[(size_t)s] = now;
    P.lap_start[(size_t)s + 1] = (int64_t)P.order.size();
    L->unpack_start[(size_t)s + 1] = (int64_t)L->unpack.size();
  }
  // the carried blocks' rows: behind the unpacked ones of their size class
  for (size_t e = 0; e < extra_at.size(); e++) {
    int32_t &o = P.order[extra_at[e]];
    const int W = (o >> 30) & 1;
    o = (int32_t)(W << 30) | (int32_t)(P.nblocks[W] + (o & 0x3fffffff));
    L->in[e].row = o & 0x3fffffff;
  }
  for (int W = 0; W < 2; W++) P.src[W].insert(P.src[W].end(), extra_src[W].begin(), extra_src[W].end());
  // what the kernels index with, once more, against the buffers' sizes
  for (const CarryRow &r : L->in)
    if (r.slot < 0 || r.slot >= max_streams || r.W < 0 || r.W >= modes || r.row < P.nblocks[r.W] || r.row >= P.nblocks[r.W] + P.extra[r.W])
      return *err = "decode_live: a carried row outside its buffer", false;
  for (const CarryRow &r : L->out)
    if (r.slot < 0 || r.slot >= max_streams || r.W < 0 || r.W >= modes || r.row < 0 || r.row >= P.nblocks[r.W])
      return *err = "decode_live: a last block outside its buffer", false;
  return true;
}

// The slots behind a call that has succeeded: status[s] as the call gave it (the heads' flags, the device's, the slot's own).
inline void decode_live_commit(std::vector<LiveSlot> *slots, const DecodeLivePlan &L, int64_t nstreams, const int64_t *slot, const uint8_t *close,
                               const uint8_t *status) {
  for (int64_t s = 0; s < nstreams; s++) {
    LiveSlot now = L.next[(size_t)s];
    const uint8_t flagged = status[s] & (uint8_t)~VAMD_STATUS_PARTIAL;  // (a packet kept under vamd_decode_partial costs its stream nothing)
    if (flagged && !(close && close[s])) now.dead = flagged, now.carry = -1;
    (*slots)[(size_t)slot[s]] = now;
  }
}

}  // namespace vamd
