// vamd_feed_ingest.h -- a part of vamd_feed.hip's translation unit: a group from its samples to its plan.  The upload turn of
// a host-fed group and the producer's event of a device-fed one, the one launch of an ingest kernel, a whole-stream group
// (run_group) and a live lane's group (run_group_live), each ending in finish_group, and the check of a device-fed group's
// source.
#pragma once
#include "vamd_feed_group.h"

// The group's samples up: in_bytes of the pinned input arena into d_in, and a small list beside them (side_bytes from
// side_src, pinned, to side_dst; 0: none), between the events the upload time is read from; returns when they are up.
// ONE upload at a time per device.  The link is a single resource: lanes that upload side by side each get a share
// of it and all finish late together -- and then all compute together while the link idles (measured: three lanes
// in lockstep, 2.3 ms of every 13 without a single kernel on the chip).  Taking turns, a lane has the whole link,
// starts its kernels the moment its samples are up, and the next lane's upload runs beside them: the lanes stagger
// themselves.
static int upload(FeedLane &L, size_t in_bytes, void *side_dst = nullptr, const void *side_src = nullptr, size_t side_bytes = 0) {
  std::lock_guard<std::mutex> turn(*L.upload_turn);
  FEED_TRY(L, hipEventRecord(L.ev0, L.stream));
  if (in_bytes) FEED_TRY(L, hipMemcpyAsync(L.d_in.p, L.h_in.p, in_bytes, hipMemcpyHostToDevice, L.stream));
  if (side_bytes) FEED_TRY(L, hipMemcpyAsync(side_dst, side_src, side_bytes, hipMemcpyHostToDevice, L.stream));
  FEED_TRY(L, hipEventRecord(L.ev_up, L.stream));
  FEED_TRY(L, hipEventSynchronize(L.ev_up));
  return VAMD_OK;
}

// A device-fed group's start, in upload()'s place: the lane's stream waits for the producer's event (recorded by
// vamd_feed_wrote_device on the caller's thread), the side list goes up, and the timing events stand where the ingest begins.
// No upload turn: the link carries a few bytes per stream.
static int source_begin(FeedLane &L, void *side_dst, const void *side_src, size_t side_bytes) {
  FEED_TRY(L, hipStreamWaitEvent(L.stream, L.src.ev_src, 0));
  if (side_bytes) FEED_TRY(L, hipMemcpyAsync(side_dst, side_src, side_bytes, hipMemcpyHostToDevice, L.stream));
  FEED_TRY(L, hipEventRecord(L.ev0, L.stream));
  FEED_TRY(L, hipEventRecord(L.ev_up, L.stream));
  return VAMD_OK;
}

// ... and behind its ingest's launch: the event vamd_feed_source_done hands out, and the word that it stands
static int source_ingested(vamd_feed *f, FeedLane &L) {
  const hipError_t e = hipEventRecord(L.src.ev_ingest, L.stream);
  {
    std::lock_guard<std::mutex> g(f->m);
    L.src.ingest_queued = true, L.src.ingest_recorded = e == hipSuccess;
  }
  f->cv_done.notify_all();
  FEED_TRY(L, e);
  return VAMD_OK;
}

// the two ingests, each in its two forms: from the lane's d_in (T: the arena's sample type), from a caller's tensors
// (T: their element type)
struct WholeIngest {
  template <typename T> static auto dev() { return k_feed_ingest_dev<T>; }
  template <typename T> static auto host() { return k_feed_ingest<T>; }
};
struct LiveIngest {
  template <typename T> static auto dev() { return k_live_ingest_dev<T>; }
  template <typename T> static auto host() { return k_live_ingest<T>; }
};

// The group's ingest kernel, K's: `items` threads' worth of work in workgroups of 256, at most 8192 of them (the kernels
// stride).  A device-fed group: the form for its tensors' element type, the strides behind args; a host-fed one: the form
// for the arena's sample type (16-bit or float), d_in in front of args.  Followed by the group's word to
// vamd_feed_source_done where it is device-fed; returns what the launch said.
template <typename K, typename... A>
static int launch_ingest(vamd_feed *f, FeedLane &L, long items, A... args) {
  long blocks = (items + 255) / 256;
  if (blocks > 256L * 32) blocks = 256L * 32;
  if (blocks < 1) blocks = 1;
  const dim3 grid((unsigned)blocks), wg(256);
  hipStream_t st = L.stream;
  if (L.src.dev) {
    const int64_t cstride = L.src.cstride, fstride = L.src.fstride;
    switch (L.src.dtype) {
      case VAMD_SRC_S16: hipLaunchKernelGGL(K::template dev<int16_t>(), grid, wg, 0, st, args..., cstride, fstride); break;
      case VAMD_SRC_F32: hipLaunchKernelGGL(K::template dev<float>(), grid, wg, 0, st, args..., cstride, fstride); break;
      case VAMD_SRC_F16: hipLaunchKernelGGL(K::template dev<vamd::src_f16>(), grid, wg, 0, st, args..., cstride, fstride); break;
      default: hipLaunchKernelGGL(K::template dev<vamd::src_bf16>(), grid, wg, 0, st, args..., cstride, fstride); break;
    }
    const hipError_t launched = hipGetLastError();
    FEED_OWN(source_ingested(f, L));
    FEED_TRY(L, launched);
    return VAMD_OK;
  }
  if (L.format == VAMD_FEED_S16) hipLaunchKernelGGL(K::template host<int16_t>(), grid, wg, 0, st, (const int16_t *)L.d_in.p, args...);
  else hipLaunchKernelGGL(K::template host<float>(), grid, wg, 0, st, (const float *)L.d_in.p, args...);
  FEED_TRY(L, hipGetLastError());
  return VAMD_OK;
}

// One whole-stream group through its lane (the lane's own thread; its device is current), from the pinned arena or from
// device memory.  Streams of unequal length (always, where device-fed) take one list, [frames_of | where each stream
// begins]: its first frame in the arena (first_of), or its base pointer (base_of).  A device-fed group has no d_in and no
// upload turn: the list rides with source_begin.
static int run_group(vamd_feed *f, FeedLane &L) {
  const long ns = L.nstreams, frames = L.frames;
  const int ch = f->ch, head = f->bs[1] / 2, pad = 3 * f->bs[1];
  const bool dev = L.src.dev, uneven = !L.frames_of.empty();
  const long cs = (long)al((size_t)head + ((frames + 3) & ~3L) + pad, 64), ss = cs * ch;
  hipStream_t st = L.stream;
  size_t in_bytes = 0;
  if (!dev) {
    size_t in_frames = (size_t)ns * frames;
    if (uneven) {
      in_frames = 0;
      for (long i = 0; i < ns; i++) in_frames += (size_t)L.frames_of[(size_t)i];
    }
    in_bytes = in_frames * ch * (L.format == VAMD_FEED_S16 ? 2 : 4);
    FEED_TRY(L, L.d_in.need(in_bytes ? in_bytes : 16));
  }
  FEED_TRY(L, L.d_pcm.need((size_t)ns * ss * 4));
  FEED_TRY(L, L.d_states.need((size_t)ns * sizeof(vamd_envelope_state)));
  FEED_TRY(L, L.d_amp.need((size_t)ns * 4));
  long long *h = nullptr;
  const long long *d_frames_of = nullptr, *d_begin_of = nullptr;
  if (uneven) {
    FEED_TRY(L, L.h_len.need((size_t)ns * 16));
    FEED_TRY(L, L.d_len.need((size_t)ns * 16));
    h = (long long *)L.h_len.p;
    long long at = 0;
    for (long i = 0; i < ns; i++) {
      h[i] = L.frames_of[(size_t)i];
      h[ns + i] = dev ? (long long)(uintptr_t)L.src.base[(size_t)i] : at;
      at += h[i];
    }
    d_frames_of = (const long long *)L.d_len.p;
    d_begin_of = d_frames_of + ns;
  }
  if (dev) FEED_OWN(source_begin(L, L.d_len.p, h, (size_t)ns * 16));
  else {
    if (uneven) FEED_TRY(L, hipMemcpyAsync(L.d_len.p, h, (size_t)ns * 16, hipMemcpyHostToDevice, st));
    FEED_OWN(upload(L, in_bytes));
  }
  FEED_OWN(launch_ingest<WholeIngest>(f, L, ns * ((long)(head >> 2) + ((frames + 3) >> 2) + (pad >> 2)), ch, ns, frames, head, pad,
                                      (float *)L.d_pcm.p, ss, cs, (float *)L.d_amp.p, (vamd_envelope_state *)L.d_states.p, d_frames_of,
                                      d_begin_of));
  vamd_stream_plan plan;
  if (uneven)
    FEED_CALL(L, vamd_plan_streams_whole_v(L.ctx, (float *)L.d_pcm.p, ss, cs, ns, frames, L.frames_of.data(), (vamd_envelope_state *)L.d_states.p, &plan));
  else
    FEED_CALL(L, vamd_plan_streams_whole(L.ctx, (float *)L.d_pcm.p, ss, cs, ns, frames, (vamd_envelope_state *)L.d_states.p, &plan));
  const FeedLive none = {nullptr, nullptr};
  return finish_group(f, L, plan, (const float *)L.d_pcm.p, ns, ss, cs, d_frames_of, none, ns);
}

// one group of a live lane: the pieces of its streams 0 .. L.nstreams-1 (and 0-frame pieces of its other open streams, which
// then emit nothing: their walks stop where they stood).  Upload -> k_live_begin (fresh streams' states) -> k_live_ingest
// (kept samples + piece into the other buffer) -> vamd_live_plan (stream ends where due, detector over the new steps,
// resumed walk, rebase; its wait brings the block counts and every stream's next rebase home) -> analysis and packets as
// a whole group's.  The host mirror of each stream says what the device holds of it (live_piece / live_planned,
// vamd_feed_host.h).
static int run_group_live(vamd_feed *f, FeedLane &L) {
  FeedLane::Live &V = L.live;
  const long nsc = L.nstreams;
  const int ch = f->ch;
  long ns = nsc;
  for (long i = nsc; i < f->max_streams; i++)
    if (V.streams[(size_t)i].open) ns = i + 1;
  const LiveShape G(f->bs[1], f->write_frames, f->live_cs);
  const long cs = G.cs, ss = cs * ch;
  hipStream_t st = L.stream;
  FEED_TRY(L, V.d_live.need((size_t)ns * sizeof(LiveIn)));
  FEED_TRY(L, V.h_live.need((size_t)ns * (sizeof(LiveIn) + sizeof(vamd_live_geo) + 8)));
  LiveIn *hin = (LiveIn *)V.h_live.p;
  vamd_live_geo *geo = (vamd_live_geo *)(hin + ns);
  long long *shift = (long long *)(geo + ns);
  int64_t first = 0, quads = 0;
  for (long i = 0; i < ns; i++) {
    const int64_t n = i < nsc ? L.frames_of[(size_t)i] : 0;
    // (a device-fed piece: where it lies; else its first frame in the arena)
    const int64_t at = !L.src.dev ? first : i < nsc ? (int64_t)(uintptr_t)L.src.base[(size_t)i] : 0;
    const char *why = live_piece(G, V.streams[(size_t)i], at, n, i < nsc && V.close_of[(size_t)i], hin[i], geo[i], &quads);
    if (why) {
      L.err = why;
      return VAMD_EFAULT;
    }
    first += n;
  }
  const size_t in_bytes = (size_t)first * ch * (L.format == VAMD_FEED_S16 ? 2 : 4);
  if (L.src.dev) FEED_OWN(source_begin(L, V.d_live.p, hin, (size_t)ns * sizeof(LiveIn)));
  else {
    FEED_TRY(L, L.d_in.need(in_bytes ? in_bytes : 16));
    FEED_OWN(upload(L, in_bytes, V.d_live.p, hin, (size_t)ns * sizeof(LiveIn)));
  }
  const LiveIn *d_live = (const LiveIn *)V.d_live.p;
  vamd_bitrate_state *bst = f->managed ? (vamd_bitrate_state *)L.managed.d_bstate.p : nullptr;
  if (f->managed && !V.btmpl_ready) {
    FEED_CALL(L, vamd_bitrate_init_states(L.ctx, (vamd_bitrate_state *)V.d_btmpl.p, 1));
    V.btmpl_ready = true;
  }
  {
    const long words = ns * (long)(sizeof(vamd_envelope_state) / 4);
    hipLaunchKernelGGL(k_live_begin, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, st, ns, d_live, (vamd_envelope_state *)L.d_states.p,
                       (float *)L.d_amp.p, bst, (const vamd_bitrate_state *)V.d_btmpl.p, (unsigned long long *)V.d_nan.p);
    *(volatile int *)V.h_lstatus.p = 0;
    int *d_lstatus = nullptr;
    FEED_TRY(L, V.h_lstatus.mapped(&d_lstatus));
    FEED_OWN(launch_ingest<LiveIngest>(f, L, ns * (long)quads, ch, ns, (long)quads, G.pad + 256, d_live, (const float *)V.d_buf[V.cur].p,
                                       (float *)V.d_buf[1 - V.cur].p, ss, cs, (unsigned long long *)V.d_nan.p, d_lstatus));
  }
  V.cur = 1 - V.cur;
  float *pcm = (float *)V.d_buf[V.cur].p;
  vamd_stream_plan plan;
  FEED_CALL(L, vamd_live_plan(L.ctx, pcm, ss, cs, ns, geo, (int)G.n_head, V.d_walk.p, (unsigned char *)V.d_rows.p, f->row_stride,
                              (vamd_envelope_state *)L.d_states.p, shift, &plan));
  if (*(volatile int *)V.h_lstatus.p) {  // (written by the ingest, mapped; the plan's wait is behind it)
    L.err = "live feed: the ingest found a stream whose samples exceed its buffer";
    return VAMD_EFAULT;
  }
  for (long i = 0; i < ns; i++) {
    const char *why = live_planned(V.streams[(size_t)i], hin[i].close != 0, shift[i], f->retain);
    if (why) {
      L.err = why;
      return VAMD_EFAULT;
    }
  }
  if (f->ogg) {  // what the pager needs to know of each stream: it begins with this group, ends with it, or is not there
    std::vector<uint32_t> &flags = L.ogg_live.flags;
    const std::vector<uint8_t> &flush = L.ogg_live.flush;
    flags.assign((size_t)ns, 0);
    for (long i = 0; i < ns; i++) {
      const bool absent = hin[i].fresh && !hin[i].frames;
      flags[(size_t)i] = absent ? vamd::OGG_LIVE_ABSENT : (hin[i].fresh ? vamd::OGG_LIVE_BEGIN : 0) | (hin[i].close ? vamd::OGG_LIVE_CLOSE : 0);
      if ((size_t)i < flush.size() && flush[(size_t)i]) flags[(size_t)i] |= vamd::OGG_LIVE_FLUSH;  // (the pager decides whom it concerns)
    }
  }
  FeedLive live;
  live.in = d_live, live.nan = (const unsigned long long *)V.d_nan.p;
  const int r = finish_group(f, L, plan, pcm, ns, ss, cs, nullptr, live, nsc);
  if (!r && L.result.stream_start && L.result.stream_start[nsc] != L.result.nblocks) {
    L.err = "live feed: a stream outside the group emitted blocks";
    return VAMD_EFAULT;
  }
  return r;
}

// what vamd_feed_wrote_device / _wrote_live_device check of their source before anything is enqueued (f->m held; the lane's
// device current): the reason in f->err
static int source_check(vamd_feed *f, const FeedLane &L, long nstreams, const int64_t *frames, const vamd_feed_source *src) {
  if (!src || !src->base) {
    f->err = "device-fed group: no source, or no base pointers";
    return VAMD_EINVAL;
  }
  if (src->dtype < 0 || src->dtype >= vamd::SRC_TYPES) {
    f->err = "device-fed group: unknown dtype " + std::to_string(src->dtype) + " (VAMD_SRC_S16 / _F32 / _F16 / _BF16)";
    return VAMD_EINVAL;
  }
  const int eb = vamd::src_elem_bytes(src->dtype);
  for (long s = 0; s < nstreams; s++) {
    const void *p = src->base[s];
    const std::string who = "device-fed group: stream " + std::to_string(s);
    if (!p) {
      if (frames[s]) {
        f->err = who + " has frames and no base pointer";
        return VAMD_EINVAL;
      }
      continue;
    }
    if ((uintptr_t)p % (uintptr_t)eb) {
      f->err = who + ": the base pointer is not a multiple of the element size";
      return VAMD_EINVAL;
    }
    hipPointerAttribute_t at;
    memset(&at, 0, sizeof(at));
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
      (void)hipGetLastError();
      f->err = who + ": the base pointer is not memory the HIP runtime knows (host memory?)";
      return VAMD_EINVAL;
    }
    if (at.type != hipMemoryTypeDevice || at.isManaged) {
      f->err = who + ": the base pointer is " + (at.isManaged || at.type == hipMemoryTypeManaged ? "managed" : at.type == hipMemoryTypeHost ? "pinned host" : "not device") +
               " memory; a device-fed group reads device memory";
      return VAMD_EINVAL;
    }
    if (at.device != L.device) {
      f->err = who + ": the base pointer is on device " + std::to_string(at.device) + ", the slot's lane on device " + std::to_string(L.device) +
               " (vamd_feed_buffer_on)";
      return VAMD_EINVAL;
    }
    hipDeviceptr_t abase = nullptr;
    size_t abytes = 0;
    if (hipMemGetAddressRange(&abase, &abytes, (hipDeviceptr_t)p) != hipSuccess || !abase || (uintptr_t)p < (uintptr_t)abase) {
      (void)hipGetLastError();
      f->err = who + ": the allocation of the base pointer cannot be had (hipMemGetAddressRange)";
      return VAMD_EINVAL;
    }
    int64_t lo = 0, hi = 0;
    const int64_t off = (int64_t)((uintptr_t)p - (uintptr_t)abase);
    const int why = vamd::source_extent(f->ch, frames[s], src->channel_stride, src->frame_stride, eb, off, (int64_t)abytes, &lo, &hi);
    if (why) {
      f->err = who + (why == 1 ? ": the extent of its strides does not fit 64-bit arithmetic"
                               : ": it reads elements [" + std::to_string(lo) + ", " + std::to_string(hi) + ") of " + std::to_string(eb) +
                                     " bytes from its base pointer, which lies " + std::to_string(off) + " bytes into an allocation of " +
                                     std::to_string(abytes) + " bytes: out of range");
      return VAMD_EINVAL;
    }
  }
  return VAMD_OK;
}
