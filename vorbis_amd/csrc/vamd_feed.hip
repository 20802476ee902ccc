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
//   * DEVICE-FED GROUPS (vamd_feed_wrote_device / _wrote_live_device): the samples already lie in HBM as a caller's tensors.
//     Such a group skips the arena, d_in and the upload turn: the call checks every base pointer and extent on the caller's
//     thread (source_check: an error code, never a fault), records an event on the producer's stream, and the lane's stream
//     waits for it in front of k_feed_ingest_dev / k_live_ingest_dev (k_feed_src.h); from the plan on it is any group.
// Built on the public C ABI only (a context is used by one thread: its lane's), like vamd_batcher.hip.
//
// One translation unit in parts by topic, like vamd_hip.hip's: vamd_feed_host.h (host arithmetic without HIP: slices, record
// layouts, the comment table, the live mirror), vamd_feed_lane.h (buffers, the lane, the feed, the error macros),
// vamd_feed_ogg.h (an Ogg feed: mirror, pager, a job's serials and comments, the header check), vamd_feed_group.h (a group
// from its plan on: record, managed slices, decoded signal, finish_group), vamd_feed_ingest.h (a group up to its plan: upload,
// device source, the ingest launch, run_group, run_group_live).  Here: the lane's thread, the feed's making and end, and
// the entry points.
#include <stdio.h>
#include <chrono>
#include "vamd_knobs.h"
#include "vamd_live.h"
#include "vamd_feed_ingest.h"

static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

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
      for (LiveStream &m : L.live.streams) m = LiveStream();
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
  f->lanes.clear();  // (~FeedLane, each on its own device)
  (void)hipSetDevice(cur);
}

// why this thread's last vamd_feed_create failed (vamd_feed_last_error(NULL))
thread_local std::string feed_create_err;

// One lane of a feed in the making, on L.device: its context, stream and events, the feed's geometry from the first lane's
// context, a live lane's device state, the arenas.  Returns at the first failure; feed_free cleans up whatever was made.
static int lane_init(vamd_feed *f, FeedLane &L, bool first, const void *setup_blob, size_t blob_bytes) {
  const long max_streams = f->max_streams, max_frames = f->max_frames;
  const int write_frames = f->write_frames;
  FEED_OWN(vamd_create(&L.ctx, setup_blob, blob_bytes, L.device));
  FEED_TRY(L, hipSetDevice(L.device));
  FEED_TRY(L, hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking));
  FEED_TRY(L, L.ev0.make(hipEventDefault));
  FEED_TRY(L, L.ev_up.make(hipEventBlockingSync));
  FEED_TRY(L, L.ev_end.make(hipEventBlockingSync));
  FEED_TRY(L, L.src.ev_src.make(hipEventDisableTiming));
  FEED_TRY(L, L.src.ev_ingest.make(hipEventDisableTiming | hipEventBlockingSync));
  if (f->decoded) FEED_TRY(L, L.dec.ev.make(hipEventDisableTiming | hipEventBlockingSync));
  if (vamd_set_stream(L.ctx, L.stream) != VAMD_OK) return VAMD_EFAULT;
  if (first) {
    f->ch = vamd_channels(L.ctx);
    for (int W = 0; W < 2; W++) f->bs[W] = vamd_blocksize(L.ctx, W), f->pkcap[W] = vamd_packet_capacity(L.ctx, W);
    if (f->pkcap[0] <= 0 || f->pkcap[1] <= 0) return VAMD_EIMPL;  // packets of this mode are not assembled on the GPU
    for (int W = 0; W < 2 && f->decoded; W++) {  // ... or its blocks not synthesised
      if (vamd_synth_check(L.ctx, W) != VAMD_OK) {
        feed_create_err = std::string("VAMD_FEED_DECODED: ") + vamd_last_error(L.ctx);
        return VAMD_EIMPL;
      }
    }
    if (write_frames) {
      const char *why = vamd_live_check(L.ctx, write_frames, max_frames);
      if (why) {
        feed_create_err = why;
        return VAMD_EIMPL;
      }
      f->retain = vamd_live_retain(L.ctx, write_frames);
      f->live_cs = (long)al((size_t)(2 * f->retain + max_frames + 3 * f->bs[1] + 512), 64);
      f->row_stride = f->live_cs / 64 + 16;
    }
  }
  if (write_frames) {  // a live lane's device state, for every stream it may carry
    FeedLane::Live &V = L.live;
    const size_t ns = (size_t)max_streams;
    for (int b = 0; b < 2; b++) FEED_TRY(L, V.d_buf[b].need(ns * f->ch * (size_t)f->live_cs * 4));
    FEED_TRY(L, V.d_walk.need(ns * VAMD_LIVE_WALK_BYTES));
    FEED_TRY(L, V.d_rows.need(ns * (size_t)f->row_stride));
    FEED_TRY(L, V.d_nan.need(ns * 8));
    FEED_TRY(L, L.d_states.need(ns * sizeof(vamd_envelope_state)));
    FEED_TRY(L, L.d_amp.need(ns * 4));
    FEED_TRY(L, L.managed.d_bstate.need(ns * sizeof(vamd_bitrate_state)));
    FEED_TRY(L, V.d_btmpl.need(sizeof(vamd_bitrate_state)));
    FEED_TRY(L, V.h_lstatus.need(64));
    V.streams.resize(ns);
  }
  // the arenas: the group's samples; packets: half the samples' size AS 16-BIT to start with (a q 0.4 stream is a
  // tenth of that, q 1.0 on noise a third; run_group grows the arena when a group needs more)
  const size_t in_cap = (size_t)max_streams * max_frames * f->ch * (f->format == VAMD_FEED_S16 ? 2 : 4);
  if (!f->no_arena) FEED_TRY(L, L.h_in.need(in_cap));
  const size_t out_cap = f->out_bytes ? (size_t)f->out_bytes : (size_t)max_streams * max_frames * f->ch + (size_t)max_streams * 65536;
  FEED_TRY(L, L.h_out.need(al(out_cap, 4096)));
  if (f->decoded) {  // the decoded arena, and k_synth's scratch for a group of long blocks (half overlapped: twice its samples)
    const size_t group = (size_t)max_streams * max_frames * f->ch;
    FEED_TRY(L, L.dec.d_dec.need((group + 4) * 4));
    FEED_TRY(L, L.dec.d_synth[1].need((2 * group + (size_t)max_streams * 4 * f->bs[1] * f->ch) * 4));
  }
  return VAMD_OK;
}

static int feed_create(vamd_feed **out, const void *setup_blob, size_t blob_bytes, const int *devices, int ndevices,
                       int lanes_per_device, long max_streams, long max_frames, int format, int write_frames) {
  if (!out) return VAMD_EINVAL;
  *out = nullptr;
  const bool no_arena = (format & VAMD_FEED_NO_ARENA) != 0, decoded = (format & VAMD_FEED_DECODED) != 0;
  format &= ~(VAMD_FEED_NO_ARENA | VAMD_FEED_DECODED);
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
  // the decoded signal: not of a live feed (the overlap would have to be carried between groups), not of a managed one (the
  // manager may cut the chosen packet, and a decoder that runs out of bits stops in mid-residue)
  if (decoded && write_frames) {
    feed_create_err = "VAMD_FEED_DECODED: a live feed has no decoded signal (whole-stream feeds only)";
    return VAMD_EIMPL;
  }
  if (decoded && h.managed) {
    feed_create_err = "VAMD_FEED_DECODED: a bitrate-managed setup has no decoded signal (the manager may cut a packet short of its residue)";
    return VAMD_EIMPL;
  }
  int cur = 0;
  if (hipGetDevice(&cur) != hipSuccess) return VAMD_EFAULT;
  std::vector<int> devs;
  if (ndevices == 0) devs.push_back(cur);
  for (int i = 0; i < ndevices; i++) devs.push_back(devices[i] >= 0 ? devices[i] : cur);
  vamd_feed *f = new vamd_feed;
  f->max_streams = max_streams, f->max_frames = max_frames, f->format = format, f->write_frames = write_frames;
  f->no_arena = no_arena, f->decoded = decoded;
  f->managed = h.managed && h.off_bitrate;
  f->rate = h.rate;
  {
    const vamd::Knobs K = vamd::read_knobs();
    f->slice = K.feed_slice > 0 ? K.feed_slice : 2048;
    f->out_bytes = K.feed_out_bytes > 0 ? K.feed_out_bytes : 0;
  }
  for (size_t l = 0; l < devs.size() * (size_t)lanes_per_device; l++) f->lanes.emplace_back();
  for (size_t d = 0; d < devs.size(); d++) f->upload_turns.emplace_back(new std::mutex);
  int r = VAMD_OK;
  // lane l runs on device l % ndevices: consecutive groups go to different devices first, to a device's next lane after
  for (size_t l = 0; l < f->lanes.size() && !r; l++) {
    FeedLane &L = f->lanes[l];
    L.device = devs[l % devs.size()];
    L.upload_turn = f->upload_turns[l % devs.size()].get();
    r = lane_init(f, L, l == 0, setup_blob, blob_bytes);
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

// the one checked way from (f, slot) to a lane; null: the feed has no such slot
static FeedLane *lane_of(const vamd_feed *f, int slot) {
  return f && slot >= 0 && slot < (int)f->lanes.size() ? const_cast<FeedLane *>(&f->lanes[(size_t)slot]) : nullptr;
}

// What the five vamd_feed_wrote* calls (`call` names the one) check of their group and set of it (f->m held): the slot
// between vamd_feed_buffer and its group, 1 to max_streams streams, each stream's frames in range -- frames[i], or `uniform`
// for every stream where frames is null -- and the lane's frames_of, a live group's close_of.  live: a piece of 0 frames is
// allowed, and `close` (may be null), but not of a stream that never had a frame.  *longest: the group's longest stream.
// (A call that fails behind this check leaves the lists set and the slot as it was: its next vamd_feed_wrote* sets them again.)
static int group_check(vamd_feed *f, FeedLane &L, const char *call, long nstreams, const int64_t *frames, long uniform, bool live,
                       const uint8_t *close, long *longest) {
  const std::string who = call;
  if (nstreams < 1 || nstreams > f->max_streams || L.state != LANE_FILLING) {
    f->err = who + ": a slot between vamd_feed_buffer and its group, 1 to max_streams streams";
    return VAMD_EINVAL;
  }
  *longest = 0;
  for (long i = 0; i < nstreams; i++) {
    const int64_t n = frames ? frames[i] : uniform;
    if (n < (live ? 0 : 1) || n > f->max_frames) {
      f->err = who + ": stream " + std::to_string(i) + " has " + std::to_string(n) + " frames, not " + (live ? "0" : "1") + " to max_frames";
      return VAMD_EINVAL;
    }
    if (live && close && close[i] && !n && !L.live.streams[(size_t)i].open) {  // (closing a stream that never had a frame)
      f->err = who + ": stream " + std::to_string(i) + " is closed and never had a frame";
      return VAMD_EINVAL;
    }
    if (n > *longest) *longest = (long)n;
  }
  if (frames) L.frames_of.assign(frames, frames + nstreams);
  else L.frames_of.clear();
  if (live) {
    L.live.close_of.assign((size_t)nstreams, 0);
    if (close)
      for (long i = 0; i < nstreams; i++) L.live.close_of[(size_t)i] = close[i] != 0;
  }
  return VAMD_OK;
}

// the tail of vamd_feed_wrote / _wrote_v / _wrote_live (f->m held; the lane's frames_of / close_of are set): the group
// goes to its lane's thread
static int queue_group(vamd_feed *f, FeedLane &L, long nstreams, long frames, bool src_dev = false) {
  L.nstreams = nstreams, L.frames = frames, L.format = f->format;
  L.src.dev = src_dev, L.src.ingest_queued = L.src.ingest_recorded = false;
  L.status = 0;
  memset(&L.result, 0, sizeof(L.result));
  memset(&L.dec.result, 0, sizeof(L.dec.result));
  ogg_job(f, L, nstreams);
  L.t_wrote = now_s();
  L.state = LANE_QUEUED;
  f->cv_work.notify_all();
  return VAMD_OK;
}

// vamd_feed_packets / vamd_feed_ogg / vamd_feed_decoded: waits for the slot's group, then hands out what its lane holds for
// the caller (result: which of the lane's)
template <typename R, typename Get>
static int await_group(vamd_feed *f, int slot, R *out, bool ogg, Get result) {
  FeedLane *lane = lane_of(f, slot);
  if (!lane || !out) return VAMD_EINVAL;
  std::unique_lock<std::mutex> g(f->m);
  if (ogg && !f->ogg) {
    f->err = "vamd_feed_ogg: the feed has no Ogg headers (vamd_feed_ogg_headers / vamd_feed_ogg_headers_live)";
    return VAMD_EINVAL;
  }
  FeedLane &L = *lane;
  if (L.state != LANE_QUEUED && L.state != LANE_DONE) return VAMD_EINVAL;
  f->cv_done.wait(g, [&] { return f->stop || L.state == LANE_DONE; });
  if (L.state != LANE_DONE) return VAMD_EFAULT;
  *out = result(L);
  return L.status;
}

extern "C" {

int vamd_feed_ogg_headers(vamd_feed *f, const void *id, long id_bytes, const void *comment, long comment_bytes, const void *setup,
                          long setup_bytes) {
  if (!f) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  if (f->write_frames) {
    f->err = "a live feed returns its Ogg files in pieces, a contract of its own: vamd_feed_ogg_headers_live";
    return VAMD_EIMPL;
  }
  return ogg_headers_set(f, "vamd_feed_ogg_headers", id, id_bytes, comment, comment_bytes, setup, setup_bytes);
}

int vamd_feed_ogg_headers_live(vamd_feed *f, const void *id, long id_bytes, const void *comment, long comment_bytes, const void *setup,
                               long setup_bytes) {
  if (!f) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  if (!f->write_frames) {
    f->err = "vamd_feed_ogg_headers_live is for a live feed (vamd_feed_create_live); a whole-stream feed takes vamd_feed_ogg_headers";
    return VAMD_EINVAL;
  }
  return ogg_headers_set(f, "vamd_feed_ogg_headers_live", id, id_bytes, comment, comment_bytes, setup, setup_bytes);
}

int vamd_feed_ogg_serials(vamd_feed *f, int slot, const uint32_t *serials, long n) {
  FeedLane *lane = lane_of(f, slot);
  if (!lane || !serials || n < 0) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  FeedLane &L = *lane;
  if (!f->ogg || L.state != LANE_FILLING || n > f->max_streams) {
    f->err = "vamd_feed_ogg_serials: an Ogg feed's slot between vamd_feed_buffer and vamd_feed_wrote, at most max_streams numbers";
    return VAMD_EINVAL;
  }
  L.ogg.user_serials.assign(serials, serials + n);
  return VAMD_OK;
}

int vamd_feed_ogg_comments(vamd_feed *f, int slot, const void *const *comment, const long *bytes, long n) {
  FeedLane *lane = lane_of(f, slot);
  if (!lane) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  FeedLane &L = *lane;
  if (!f->ogg || L.state != LANE_FILLING || n < 0 || n > f->max_streams || (n && (!comment || !bytes))) {
    f->err = !f->ogg ? "vamd_feed_ogg_comments: the feed has no Ogg headers (vamd_feed_ogg_headers / vamd_feed_ogg_headers_live)"
                     : "vamd_feed_ogg_comments: a slot between vamd_feed_buffer and vamd_feed_wrote, 0 to max_streams comments and their lengths";
    return VAMD_EINVAL;
  }
  std::vector<std::vector<uint8_t>> all((size_t)n);
  for (long s = 0; s < n; s++) {
    if (!comment[s]) continue;
    const uint8_t *p = (const uint8_t *)comment[s];
    const int why = vamd::ogg_comment_check(p, (int64_t)bytes[s]);
    if (why) {
      f->err = "vamd_feed_ogg_comments: the comment header of stream " + std::to_string(s) + " (" + std::to_string(bytes[s]) +
               " bytes) is refused: " + vamd::ogg_comment_why(why);
      return VAMD_EINVAL;
    }
    all[(size_t)s].assign(p, p + bytes[s]);
  }
  L.ogg.user_comments.swap(all);
  return VAMD_OK;
}

int vamd_feed_ogg_flush(vamd_feed *f, int slot, const uint8_t *flush, long n) {
  FeedLane *lane = lane_of(f, slot);
  if (!lane) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  FeedLane &L = *lane;
  if (!f->write_frames || !f->ogg || L.state != LANE_FILLING || n < 0 || n > f->max_streams) {
    f->err = !f->write_frames ? "vamd_feed_ogg_flush is for a live Ogg feed (vamd_feed_create_live, vamd_feed_ogg_headers_live): a whole stream's file has no open page to flush"
             : !f->ogg        ? "vamd_feed_ogg_flush: the feed has no Ogg headers (vamd_feed_ogg_headers_live)"
                              : "vamd_feed_ogg_flush: a slot between vamd_feed_buffer and vamd_feed_wrote_live, 0 to max_streams flags";
    return VAMD_EINVAL;
  }
  L.ogg_live.user_flush.assign((size_t)n, 1);  // (flush == NULL: every one of the first n)
  if (flush)
    for (long s = 0; s < n; s++) L.ogg_live.user_flush[(size_t)s] = flush[s] != 0;
  return VAMD_OK;
}

int vamd_feed_ogg(vamd_feed *f, int slot, vamd_feed_ogg_result *out) { return await_group(f, slot, out, true, [](const FeedLane &L) { return L.ogg.result; }); }

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
  const FeedLane *lane = lane_of(f, slot);
  return lane ? lane->device : VAMD_EINVAL;
}

// vamd_feed_buffer (device < 0: a lane anywhere) and vamd_feed_buffer_on (a lane on `device`)
static int feed_buffer(vamd_feed *f, int device, void **pcm) {
  if (!f || !pcm) return VAMD_EINVAL;
  std::unique_lock<std::mutex> g(f->m);
  auto mine = [&](const FeedLane &L) { return device < 0 || L.device == device; };
  if (device >= 0) {
    bool any = false;
    for (const FeedLane &L : f->lanes) any |= mine(L);
    if (!any) {
      f->err = "vamd_feed_buffer_on: the feed has no lane on device " + std::to_string(device);
      return VAMD_EINVAL;
    }
  }
  for (;;) {
    if (f->stop) return VAMD_EFAULT;
    int best = -1;
    for (size_t l = 0; l < f->lanes.size(); l++)
      if (mine(f->lanes[l]) && f->lanes[l].state == LANE_FREE && (best < 0 || f->lanes[l].served < f->lanes[(size_t)best].served)) best = (int)l;
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
    for (const FeedLane &L : f->lanes) hope |= mine(L) && (L.state == LANE_QUEUED || L.state == LANE_DONE);
    if (!hope) return VAMD_EINVAL;
    f->cv_done.wait(g);
  }
}

// the tail of the two: the source is the lane's, the producer's event recorded (the lane's device current), the group queued
static int queue_group_device(vamd_feed *f, FeedLane &L, long nstreams, long frames, const vamd_feed_source *src) {
  const hipError_t e = hipEventRecord(L.src.ev_src, (hipStream_t)src->producer);
  if (e != hipSuccess) {
    f->err = std::string("device-fed group: hipEventRecord on the producer's stream: ") + hipGetErrorString(e);
    return VAMD_EINVAL;
  }
  L.src.base.assign(src->base, src->base + nstreams);
  L.src.dtype = src->dtype, L.src.cstride = src->channel_stride, L.src.fstride = src->frame_stride;
  return queue_group(f, L, nstreams, frames, true);
}

// the lane's device current for a call's checks and its event, the caller's restored behind them
struct DeviceScope {
  int before = -1;
  explicit DeviceScope(int device) {
    if (hipGetDevice(&before) != hipSuccess) before = -1;
    if (before != device) (void)hipSetDevice(device);
    else before = -1;
  }
  ~DeviceScope() {
    if (before >= 0) (void)hipSetDevice(before);
  }
};

int vamd_feed_buffer(vamd_feed *f, void **pcm) { return feed_buffer(f, -1, pcm); }

int vamd_feed_buffer_on(vamd_feed *f, int device, void **pcm) { return device < 0 ? VAMD_EINVAL : feed_buffer(f, device, pcm); }

int vamd_feed_wrote_device(vamd_feed *f, int slot, long nstreams, const int64_t *frames, const vamd_feed_source *src) {
  FeedLane *lane = lane_of(f, slot);
  if (!lane || !frames) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  if (f->write_frames) {
    f->err = "vamd_feed_wrote_device is for a whole-stream feed; a live feed takes vamd_feed_wrote_live_device";
    return VAMD_EINVAL;
  }
  FeedLane &L = *lane;
  long longest = 0;
  FEED_OWN(group_check(f, L, "vamd_feed_wrote_device", nstreams, frames, 0, false, nullptr, &longest));
  DeviceScope on(L.device);
  FEED_OWN(source_check(f, L, nstreams, frames, src));
  return queue_group_device(f, L, nstreams, longest, src);
}

int vamd_feed_wrote_live_device(vamd_feed *f, int slot, long nstreams, const int64_t *frames, const uint8_t *close, const vamd_feed_source *src) {
  FeedLane *lane = lane_of(f, slot);
  if (!lane || !frames) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  if (!f->write_frames) {
    f->err = "vamd_feed_wrote_live_device is for a live feed (vamd_feed_create_live); a whole-stream feed takes vamd_feed_wrote_device";
    return VAMD_EINVAL;
  }
  FeedLane &L = *lane;
  long longest = 0;
  FEED_OWN(group_check(f, L, "vamd_feed_wrote_live_device", nstreams, frames, 0, true, close, &longest));
  DeviceScope on(L.device);
  FEED_OWN(source_check(f, L, nstreams, frames, src));
  return queue_group_device(f, L, nstreams, f->max_frames, src);
}

int vamd_feed_source_done(vamd_feed *f, int slot, void *consumer, int wait_on_host) {
  FeedLane *lane = lane_of(f, slot);
  if (!lane) return VAMD_EINVAL;
  std::unique_lock<std::mutex> g(f->m);
  FeedLane &L = *lane;
  if ((L.state != LANE_QUEUED && L.state != LANE_DONE) || !L.src.dev) {
    f->err = "vamd_feed_source_done: the slot holds no device-fed group";
    return VAMD_EINVAL;
  }
  f->cv_done.wait(g, [&] { return f->stop || L.src.ingest_queued || L.state == LANE_DONE; });
  if (f->stop) return VAMD_EFAULT;
  if (!L.src.ingest_recorded) return VAMD_OK;  // (the group failed before its ingest: nothing of the lane's reads the source)
  const hipEvent_t ev = L.src.ev_ingest;
  g.unlock();  // (the event is this group's until the slot is released, which is the caller's to do)
  if (consumer && hipStreamWaitEvent((hipStream_t)consumer, ev, 0) != hipSuccess) return VAMD_EFAULT;
  if (wait_on_host && hipEventSynchronize(ev) != hipSuccess) return VAMD_EFAULT;
  return VAMD_OK;
}

int vamd_feed_wrote(vamd_feed *f, int slot, long nstreams, long frames) {
  FeedLane *lane = lane_of(f, slot);
  if (!lane || f->write_frames || f->no_arena) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  long longest = 0;
  FEED_OWN(group_check(f, *lane, "vamd_feed_wrote", nstreams, nullptr, frames, false, nullptr, &longest));
  return queue_group(f, *lane, nstreams, frames);
}

int vamd_feed_wrote_v(vamd_feed *f, int slot, long nstreams, const int64_t *frames) {
  FeedLane *lane = lane_of(f, slot);
  if (!lane || !frames || f->write_frames || f->no_arena) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  long longest = 0;
  FEED_OWN(group_check(f, *lane, "vamd_feed_wrote_v", nstreams, frames, 0, false, nullptr, &longest));
  long long total = 0;  // (the streams lie back to back in the arena, which holds max_streams * max_frames frames)
  for (long i = 0; i < nstreams; i++) total += frames[i];
  if (total > (long long)f->max_streams * f->max_frames) return VAMD_EINVAL;
  return queue_group(f, *lane, nstreams, longest);
}

int vamd_feed_wrote_live(vamd_feed *f, int slot, long nstreams, const int64_t *frames, const uint8_t *close) {
  FeedLane *lane = lane_of(f, slot);
  if (!lane || !frames || !f->write_frames || f->no_arena) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  long longest = 0;
  FEED_OWN(group_check(f, *lane, "vamd_feed_wrote_live", nstreams, frames, 0, true, close, &longest));
  return queue_group(f, *lane, nstreams, f->max_frames);
}

int vamd_feed_packets(vamd_feed *f, int slot, vamd_feed_result *out) { return await_group(f, slot, out, false, [](const FeedLane &L) { return L.result; }); }

int vamd_feed_decoded(vamd_feed *f, int slot, vamd_feed_decoded_result *out) {
  FeedLane *lane = lane_of(f, slot);
  if (!lane || !out) return VAMD_EINVAL;
  memset(out, 0, sizeof(*out));
  if (!f->decoded) {
    std::lock_guard<std::mutex> g(f->m);
    f->err = "vamd_feed_decoded: the feed was not created with VAMD_FEED_DECODED";
    return VAMD_EINVAL;
  }
  const int r = await_group(f, slot, out, false, [](const FeedLane &L) { return L.dec.result; });
  if (r) {
    memset(out, 0, sizeof(*out));
    return r;
  }
  if (hipEventSynchronize(lane->dec.ev) != hipSuccess) {
    std::lock_guard<std::mutex> g(f->m);
    f->err = "vamd_feed_decoded: the decoded signal's kernels failed";
    memset(out, 0, sizeof(*out));
    return VAMD_EFAULT;
  }
  return VAMD_OK;
}

int vamd_feed_release(vamd_feed *f, int slot) {
  FeedLane *lane = lane_of(f, slot);
  if (!lane) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  FeedLane &L = *lane;
  if (L.state != LANE_DONE && L.state != LANE_FILLING) return VAMD_EINVAL;
  L.ogg.user_serials.clear();
  L.ogg.user_comments.clear();
  L.ogg.comments.clear();
  L.ogg_live.user_flush.clear();
  L.ogg_live.flush.clear();
  L.state = LANE_FREE;
  f->cv_done.notify_all();
  return VAMD_OK;
}

const char *vamd_feed_last_error(const vamd_feed *f) { return f ? f->err.c_str() : feed_create_err.c_str(); }

}  // extern "C"
