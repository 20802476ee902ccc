// vamd_feed_lane.h -- a part of vamd_feed.hip's translation unit: what a lane is made of.  Buffers and events that free
// themselves, the lane with each feature's members in a sub-object of its own, the feed, and the macros that put a failing
// call's text into a lane's error.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <condition_variable>
#include <deque>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "vorbis_amd.h"
#include "vamd_feed_host.h"

using namespace vamd;  // (the feed's kernels and their structs: k_feed.h, k_ogg.h; its host arithmetic: vamd_feed_host.h)

namespace {

// A buffer that says where it lives -- HBM, or pinned host memory (what the copy engine reads and what the kernels write
// across the link) -- and frees itself: a lane's buffers go with the lane (~FeedLane), each exactly once.
template <bool pinned>
struct BufIn {
  void *p = nullptr;
  size_t bytes = 0;
  BufIn() = default;
  BufIn(const BufIn &) = delete;
  BufIn &operator=(const BufIn &) = delete;
  ~BufIn() { drop(); }
  static hipError_t take(void **q, size_t n) { return pinned ? hipHostMalloc(q, n, hipHostMallocDefault) : hipMalloc(q, n); }
  void drop() {
    if (p) (void)(pinned ? hipHostFree(p) : hipFree(p));
    p = nullptr, bytes = 0;
  }
  void adopt(void *q, size_t n) { drop(), p = q, bytes = n; }
  // at least n bytes; what it held is gone when it has to grow
  hipError_t need(size_t n) {
    if (bytes >= n) return hipSuccess;
    drop();
    const hipError_t e = take(&p, n);
    if (e == hipSuccess) bytes = n;
    return e;
  }
  // pinned host memory only: at least n bytes, the first `keep` kept
  hipError_t grow_keeping(size_t n, size_t keep) {
    static_assert(pinned, "the host copies what is kept");
    if (bytes >= n) return hipSuccess;
    void *q = nullptr;
    const hipError_t e = take(&q, n);
    if (e != hipSuccess) return e;
    if (p && keep) memcpy(q, p, keep < bytes ? keep : bytes);
    adopt(q, n);
    return hipSuccess;
  }
  // pinned host memory only: the block as the device sees it (it is mapped into the device's address space)
  template <typename T>
  hipError_t mapped(T **q) const {
    static_assert(pinned, "HBM is not mapped");
    void *d = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&d, p, 0);
    *q = (T *)d;
    return e;
  }
};
using Buf = BufIn<false>;     // HBM
using Pinned = BufIn<true>;   // pinned host memory

// an event that goes with its lane, like a buffer (~FeedLane: the lane's device is current when the members go)
struct Event {
  hipEvent_t ev = nullptr;
  Event() = default;
  Event(const Event &) = delete;
  Event &operator=(const Event &) = delete;
  ~Event() {
    if (ev) (void)hipEventDestroy(ev);
  }
  hipError_t make(unsigned flags) { return hipEventCreateWithFlags(&ev, flags); }
  operator hipEvent_t() const { return ev; }
};

}  // namespace

enum { LANE_FREE = 0, LANE_FILLING, LANE_QUEUED, LANE_DONE };

struct FeedLane {
  int device = 0;
  vamd_ctx *ctx = nullptr;
  hipStream_t stream = nullptr;
  Event ev0, ev_up, ev_end;                    // around the upload and behind the hand-over: the two timings, the group's wait
  Pinned h_in, h_out, h_rec;                   // the group's samples; its packets; their records
  Buf d_in, d_pcm, d_states, d_amp;            // HBM: the samples as they came; as floats, planar; detector states; ampmax chains
  Buf d_pk[2], d_bits[2], d_status[2];         // the analysis' packet rows per size class
  Buf d_rel, d_sid, d_sbytes, d_soff, d_len;   // (d_len: [frames_of | first_of] of a group of unequal streams: h_len's copy)
  Pinned h_len;
  // bitrate-managed setups (run_group_managed): a slice's fifteen candidates per block and what the analysis needs beside
  // them, the walk's answers, the managers' states, the slices' rebased lists (d_slice: h_slice's copy)
  struct Managed {
    Buf d_mpk[2], d_mbits[2], d_mposts[2], d_mvalid[2], d_miwork[2], d_mnz[2], d_choice[2], d_fbits[2];
    Buf d_bstate, d_slice;
    Pinned h_slice;
  } managed;
  // a live feed (run_group_live): the two stream buffers, the walks' states, the carried detector flags, the first
  // non-finite sample per stream, the manager's fresh state; the group's LiveIn (d_live: h_live's copy), the ingest's
  // complaint (h_lstatus) and the host mirror
  struct Live {
    Buf d_buf[2], d_walk, d_rows, d_nan, d_btmpl, d_live;
    Pinned h_live, h_lstatus;
    int cur = 0;                      // the buffer that holds the streams now
    bool btmpl_ready = false;
    std::vector<LiveStream> streams;  // the host's mirror of each stream of the lane (vamd_feed_host.h)
    std::vector<uint8_t> close_of;    // the job's closes
  } live;
  // an Ogg feed (vamd_feed_ogg_headers): the device mirror of the packet arena and of the records, the header packets, the
  // group's serial numbers, the page table and the streams' file sizes; the files and their record
  struct Ogg {
    Buf d_mirror, d_moff, d_mgp, d_mrbits, d_minfo, d_hdr, d_serial, d_pages, d_fbytes, d_foff, d_npages, d_ostatus;
    Pinned h_serial, h_ogg, h_orec;
    int32_t hdr_off[3] = {0, 0, 0};
    std::vector<uint32_t> serials, user_serials;  // the job's; what vamd_feed_ogg_serials set for it
    // comment headers per stream (vamd_feed_ogg_comments; an empty entry: the feed's own): what the call set for the slot,
    // and the job's, kept until the group is done -- a group laid out twice is paged twice.  h_cmt / d_cmt: the job's table
    // and bytes as the pager reads them (comment_table, vamd_feed_host.h)
    std::vector<std::vector<uint8_t>> comments, user_comments;
    Pinned h_cmt;
    Buf d_cmt;
    vamd_feed_ogg_result result;
  } ogg;
  // a live Ogg feed (vamd_feed_ogg_headers_live): per stream the pager's state and its carry -- the packets on the page
  // still open -- in two buffers each; cur names the one the last group left, the next group writes the other
  // (k_ogg.h, OggLiveIO).  flags: the group's OGG_LIVE_* per stream (run_group_live).  flush: the streams the job
  // flushes behind its packets (vamd_feed_ogg_flush; user_flush: what the call set for the slot), kept like the comments
  // until the group is done; it rides in flags as OGG_LIVE_FLUSH.
  struct OggLiveState {
    Buf d_olive[2], d_crec[2], d_cbytes[2], d_gstart;
    int cur = 0;
    std::vector<uint32_t> flags;
    std::vector<uint8_t> flush, user_flush;
  } ogg_live;
  // a device-fed job (vamd_feed_wrote_device / _wrote_live_device): the streams' base pointers and what else the call named;
  // ev_src: recorded on the producer's stream by the call, waited for by the lane's stream before the ingest; ev_ingest:
  // recorded behind the ingest, what vamd_feed_source_done hands out.  ingest_queued / ingest_recorded (guarded by
  // vamd_feed::m): the lane's thread is past the ingest's launch; ev_ingest stands for this group's ingest.
  struct Source {
    bool dev = false, ingest_queued = false, ingest_recorded = false;
    std::vector<const void *> base;
    int dtype = 0;
    int64_t cstride = 0, fstride = 0;
    Event ev_src, ev_ingest;
  } src;
  // a decoded feed (VAMD_FEED_DECODED): k_synth's scratch per size class, the decoded arena, the streams' [frames | offset]
  // (d_dgeo: h_dgeo's copy); ev: recorded behind the lap, what vamd_feed_decoded waits for; what it hands out
  struct Decoded {
    Buf d_synth[2], d_dec, d_dgeo;
    Pinned h_dgeo;
    Event ev;
    std::vector<int64_t> frames, offset;
    std::vector<uint8_t> status;
    vamd_feed_decoded_result result;
  } dec;
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
  // The lane's end (feed_free has joined its worker): its device current, nothing of its stream in flight, the context
  // before the buffers it was given -- which, members like the events, free themselves behind this body, the device still
  // current.
  ~FeedLane() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (ctx) vamd_destroy(ctx);
    if (stream) (void)hipStreamDestroy(stream);
  }
};

struct vamd_feed {
  std::deque<FeedLane> lanes;  // (a deque: a lane is made in place and never moved -- its worker holds its address)
  int ch = 0, bs[2] = {0, 0};
  bool managed = false;  // the blob carries a bitrate manager (vamd_setup_header.off_bitrate): run_group_managed
  long slice = 2048;     // blocks per slice of a managed group (VAMD_FEED_SLICE, a test knob)
  long out_bytes = 0;    // > 0: a lane's packet arena to start with (VAMD_FEED_OUT_BYTES, a test knob: the arena then has to grow)
  long pkcap[2] = {0, 0};
  long max_streams = 0, max_frames = 0;
  int format = VAMD_FEED_S16;
  bool no_arena = false;            // VAMD_FEED_NO_ARENA: the lanes have no pinned input arena (device-fed groups only)
  bool decoded = false;             // VAMD_FEED_DECODED: the decoded signal beside the packets (vamd_feed_decoded)
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

// a HIP call / a call of the library's on lane L's behalf: its failure is the lane's error and the caller's return
#define FEED_TRY(L, expr)                                                           \
  do {                                                                              \
    const hipError_t e__ = (expr);                                                  \
    if (e__ != hipSuccess) {                                                        \
      (L).err = std::string(#expr) + ": " + hipGetErrorString(e__);                 \
      return VAMD_EFAULT;                                                           \
    }                                                                               \
  } while (0)
#define FEED_CALL(L, expr)                                                          \
  do {                                                                              \
    const int r__ = (expr);                                                         \
    if (r__) {                                                                      \
      (L).err = std::string(#expr) + ": " + vamd_last_error((L).ctx);               \
      return r__;                                                                   \
    }                                                                               \
  } while (0)

#define FEED_OWN(expr)           \
  do {                           \
    const int r__ = (expr);      \
    if (r__) return r__;         \
  } while (0)
