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
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <chrono>
#include <memory>
#include <condition_variable>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "vorbis_amd.h"
#include "vamd_knobs.h"
#include "vamd_live.h"
#include "k_feed.h"
#include "k_ogg.h"

using namespace vamd;  // (the feed's kernels and their structs: k_feed.h, k_ogg.h)

namespace {

double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
size_t al(size_t x, size_t a) { return (x + a - 1) / a * a; }

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
};
using Buf = BufIn<false>;     // HBM
using Pinned = BufIn<true>;   // pinned host memory

}  // namespace

enum { LANE_FREE = 0, LANE_FILLING, LANE_QUEUED, LANE_DONE };

struct FeedLane {
  int device = 0;
  vamd_ctx *ctx = nullptr;
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev_up = nullptr, ev_end = nullptr;
  Pinned h_in, h_out, h_rec;                   // the group's samples; its packets; their records
  Buf d_in, d_pcm, d_states, d_amp;            // HBM: the samples as they came; as floats, planar; detector states; ampmax chains
  Buf d_pk[2], d_bits[2], d_status[2];         // the analysis' packet rows per size class
  Buf d_rel, d_sid, d_sbytes, d_soff, d_len;   // (d_len: [frames_of | first_of] of a group of unequal streams: h_len's copy)
  Pinned h_len;
  // bitrate-managed setups (run_group_managed): a slice's fifteen candidates per block and what the analysis needs beside
  // them, the walk's answers, the managers' states, the slices' rebased lists (d_slice: h_slice's copy)
  Buf d_mpk[2], d_mbits[2], d_mposts[2], d_mvalid[2], d_miwork[2], d_mnz[2], d_choice[2], d_fbits[2];
  Buf d_bstate, d_slice;
  Pinned h_slice;
  // a live feed (run_group_live): the two stream buffers, the walks' states, the carried detector flags, the first
  // non-finite sample per stream, the manager's fresh state; the group's LiveIn (d_live: h_live's copy), the ingest's
  // complaint (h_lstatus) and the host mirror
  Buf d_buf[2], d_walk, d_rows, d_nan, d_btmpl, d_live;
  Pinned h_live, h_lstatus;
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
  // group's serial numbers, the page table and the streams' file sizes; the files and their record
  Buf d_mirror, d_moff, d_mgp, d_mrbits, d_minfo, d_hdr, d_serial, d_pages, d_fbytes, d_foff, d_npages, d_ostatus;
  Pinned h_serial, h_ogg, h_orec;
  int32_t hdr_off[3] = {0, 0, 0};
  std::vector<uint32_t> serials, user_serials;  // the job's; what vamd_feed_ogg_serials set for it
  // comment headers per stream (vamd_feed_ogg_comments; an empty entry: the feed's own): what the call set for the slot,
  // and the job's, kept until the group is done -- a group laid out twice is paged twice.  h_cmt / d_cmt: the job's table
  // and bytes as the pager reads them, [off (ns, 8 bytes each) | bytes (ns, 4 each) | the comments, each at a multiple of 4]
  std::vector<std::vector<uint8_t>> comments, user_comments;
  Pinned h_cmt;
  Buf d_cmt;
  // a live Ogg feed (vamd_feed_ogg_headers_live): per stream the pager's state and its carry -- the packets on the page
  // still open -- in two buffers each; ogg_cur names the one the last group left, the next group writes the other
  // (k_ogg.h, OggLiveIO).  ogg_flags: the group's OGG_LIVE_* per stream (run_group_live).  flush: the streams the job
  // flushes behind its packets (vamd_feed_ogg_flush; user_flush: what the call set for the slot), kept like the comments
  // until the group is done; it rides in ogg_flags as OGG_LIVE_FLUSH.
  Buf d_olive[2], d_crec[2], d_cbytes[2], d_gstart;
  int ogg_cur = 0;
  std::vector<uint32_t> ogg_flags;
  std::vector<uint8_t> flush, user_flush;
  vamd_feed_ogg_result ogg_result;
  std::vector<uint8_t> close_of;  // the job's closes (live)
  // a device-fed job (vamd_feed_wrote_device / _wrote_live_device): the streams' base pointers and what else the call named;
  // ev_src: recorded on the producer's stream by the call, waited for by the lane's stream before the ingest; ev_ingest:
  // recorded behind the ingest, what vamd_feed_source_done hands out.  ingest_queued / ingest_recorded (guarded by
  // vamd_feed::m): the lane's thread is past the ingest's launch; ev_ingest stands for this group's ingest.
  bool src_dev = false, ingest_queued = false, ingest_recorded = false;
  std::vector<const void *> src_base;
  int src_dtype = 0;
  int64_t src_cstride = 0, src_fstride = 0;
  hipEvent_t ev_src = nullptr, ev_ingest = nullptr;
  // a decoded feed (VAMD_FEED_DECODED): k_synth's scratch per size class, the decoded arena, the streams' [frames | offset]
  // (d_dgeo: h_dgeo's copy); ev_dec: recorded behind the lap, what vamd_feed_decoded waits for; what it hands out
  Buf d_synth[2], d_dec, d_dgeo;
  Pinned h_dgeo;
  hipEvent_t ev_dec = nullptr;
  std::vector<int64_t> dec_frames, dec_offset;
  std::vector<uint8_t> dec_status;
  vamd_feed_decoded_result dec_result;
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
  // before the buffers it was given -- which, members, free themselves behind this body, the device still current.
  ~FeedLane() {
    (void)hipSetDevice(device);
    if (stream) (void)hipStreamSynchronize(stream);
    if (ctx) vamd_destroy(ctx);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev_up) (void)hipEventDestroy(ev_up);
    if (ev_end) (void)hipEventDestroy(ev_end);
    if (ev_src) (void)hipEventDestroy(ev_src);
    if (ev_ingest) (void)hipEventDestroy(ev_ingest);
    if (ev_dec) (void)hipEventDestroy(ev_dec);
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
      L.d_mirror.adopt(q, want);
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
// A group with comment headers of its own (L.comments, vamd_feed_ogg_comments): they go up beside the serial numbers, the
// header slots are those of the group's longest comment and the file arena is sized from their sum (ogg_file_bound_v).
// A live group (f->write_frames): the streams' states and carries go along (OggLiveIO), k_ogg_carry runs behind the pages;
// what it and k_ogg_plan write is the OTHER state and carry, which pager_result makes the current ones -- so a group that
// is laid out twice (finish_group) advances its streams once.
static int run_pager(vamd_feed *f, FeedLane &L, const int64_t *d_stream_start, long ns, long nb, const int64_t *d_packet_total) {
  hipStream_t st = L.stream;
  const bool live = f->write_frames != 0;
  int32_t hb[3];
  for (int i = 0; i < 3; i++) hb[i] = (int32_t)f->ogg_hdr[i].size();
  if (live && !L.d_gstart.p) {  // the streams' states and carries: once per lane, for every stream it may carry
    const size_t n = (size_t)f->max_streams;
    for (int b = 0; b < 2; b++) {
      FEED_TRY(L.d_olive[b].need(n * sizeof(vamd::OggLive)));
      FEED_TRY(L.d_crec[b].need(n * 2 * vamd::OGG_MAX_SEGS * 4));
      FEED_TRY(L.d_cbytes[b].need(n * vamd::OGG_CARRY_BYTES + 16));
      FEED_TRY(hipMemsetAsync(L.d_olive[b].p, 0, L.d_olive[b].bytes, st));
      FEED_TRY(hipMemsetAsync(L.d_crec[b].p, 0, L.d_crec[b].bytes, st));
      FEED_TRY(hipMemsetAsync(L.d_cbytes[b].p, 0, L.d_cbytes[b].bytes, st));
    }
    FEED_TRY(L.d_gstart.need(n * 8));
  }
  if (!L.d_hdr.p) {  // the header packets, each at a multiple of 4: once per lane
    size_t at = 0;
    for (int i = 0; i < 3; i++) L.hdr_off[i] = (int32_t)at, at += al((size_t)hb[i], 4);
    std::vector<uint8_t> img(at + 16, 0);
    for (int i = 0; i < 3; i++) memcpy(img.data() + L.hdr_off[i], f->ogg_hdr[i].data(), (size_t)hb[i]);
    FEED_TRY(L.d_hdr.need(img.size()));
    FEED_TRY(hipMemcpy(L.d_hdr.p, img.data(), img.size(), hipMemcpyHostToDevice));
  }
  if (live) L.serials.resize((size_t)ns, 0);  // (the lane's open streams beyond the caller's begin nothing)
  if ((long)L.serials.size() != ns || !L.d_mirror.p || (live && (long)L.ogg_flags.size() != ns)) {
    L.err = "Ogg feed: the group has no serial numbers or no mirror";
    return VAMD_EFAULT;
  }
  // [serial (ns) | a live group's flags (ns)]
  FEED_TRY(L.h_serial.need((size_t)ns * 8));
  FEED_TRY(L.d_serial.need((size_t)ns * 8));
  memcpy(L.h_serial.p, L.serials.data(), (size_t)ns * 4);
  if (live) memcpy((uint32_t *)L.h_serial.p + ns, L.ogg_flags.data(), (size_t)ns * 4);
  FEED_TRY(hipMemcpyAsync(L.d_serial.p, L.h_serial.p, (size_t)ns * (live ? 8 : 4), hipMemcpyHostToDevice, st));
  // the group's own comment headers: the table and the bytes in one copy; the slots from the longest, the arena from the sum
  const bool tagged = !L.comments.empty();
  int64_t cmt_sum = 0;
  if (tagged) {
    auto own = [&](long s) { return (size_t)s < L.comments.size() && !L.comments[(size_t)s].empty() ? &L.comments[(size_t)s] : nullptr; };
    const size_t table = al((size_t)ns * 12, 8);
    size_t at = table;
    int32_t longest = 0;
    for (long s = 0; s < ns; s++) {
      const size_t n = own(s) ? own(s)->size() : (size_t)hb[1];
      if (own(s)) at += al(n, 4);
      cmt_sum += (int64_t)n;
      if ((int32_t)n > longest) longest = (int32_t)n;
    }
    FEED_TRY(L.h_cmt.need(at + 8));
    FEED_TRY(L.d_cmt.need(at + 8));
    uint8_t *img = (uint8_t *)L.h_cmt.p;
    int64_t *off = (int64_t *)img;
    int32_t *len = (int32_t *)(img + (size_t)ns * 8);
    memset(img, 0, at + 8);
    at = table;
    for (long s = 0; s < ns; s++) {
      off[s] = (int64_t)at, len[s] = -1;
      if (!own(s)) continue;
      len[s] = (int32_t)own(s)->size();
      memcpy(img + at, own(s)->data(), own(s)->size());
      at += al(own(s)->size(), 4);
    }
    FEED_TRY(hipMemcpyAsync(L.d_cmt.p, L.h_cmt.p, at + 8, hipMemcpyHostToDevice, st));
    hb[1] = longest;  // (from here on hb sizes the slots; the pager's own copy of the shared lengths is f->ogg_hdr's)
  }
  const int64_t hs = live ? vamd::ogg_live_slots(hb) : vamd::ogg_header_slots(hb);
  const int64_t sp = vamd::ogg_slots_per_packet(f->pkcap[0] > f->pkcap[1] ? f->pkcap[0] : f->pkcap[1]);
  const int64_t nslots = ns * hs + sp * nb;
  FEED_TRY(L.d_pages.need((size_t)nslots * sizeof(vamd::OggPage)));
  FEED_TRY(L.d_fbytes.need((size_t)ns * 8));
  FEED_TRY(L.d_foff.need((size_t)(ns + 1) * 8));
  FEED_TRY(L.d_npages.need((size_t)ns * 4));
  FEED_TRY(L.d_ostatus.need((size_t)ns));
  FEED_TRY(L.h_orec.need(al(orec_status(ns) + (size_t)ns, 16)));
  const int64_t bound = tagged ? (live ? vamd::ogg_live_file_bound_v((int64_t)L.h_out.bytes, nb, ns, hb, cmt_sum)
                                       : vamd::ogg_file_bound_v((int64_t)L.h_out.bytes, nb, ns, hb, cmt_sum))
                        : live ? vamd::ogg_live_file_bound((int64_t)L.h_out.bytes, nb, ns, hb) : vamd::ogg_file_bound((int64_t)L.h_out.bytes, nb, ns, hb);
  FEED_TRY(L.h_ogg.need(al((size_t)bound + 16, 4096)));
  void *drec = nullptr, *dbytes = nullptr;
  FEED_TRY(hipHostGetDevicePointer(&drec, L.h_orec.p, 0));
  FEED_TRY(hipHostGetDevicePointer(&dbytes, L.h_ogg.p, 0));
  vamd::OggIn I;
  I.stream_start = d_stream_start;
  I.off = (const int64_t *)L.d_moff.p, I.gp = (const int64_t *)L.d_mgp.p, I.bits = (const int32_t *)L.d_mrbits.p;
  I.info = (const uint8_t *)L.d_minfo.p, I.bytes = (const uint8_t *)L.d_mirror.p, I.cap = (int64_t)L.h_out.bytes;
  I.packet_total = d_packet_total;
  I.hdr = (const uint8_t *)L.d_hdr.p;
  for (int i = 0; i < 3; i++) I.hdr_off[i] = L.hdr_off[i], I.hdr_bytes[i] = (int32_t)f->ogg_hdr[i].size();
  I.serial = (const uint32_t *)L.d_serial.p;
  I.header_slots = hs, I.slots_per_packet = sp;
  I.cmt = tagged ? (const uint8_t *)L.d_cmt.p : nullptr;
  vamd::OggOut O;
  uint8_t *dr = (uint8_t *)drec;
  O.total = (int64_t *)dr, O.stream_offset = (int64_t *)(dr + 8), O.npages = (int32_t *)(dr + orec_npages(ns)), O.status = dr + orec_status(ns);
  O.bytes = (uint8_t *)dbytes, O.cap = (int64_t)L.h_ogg.bytes;
  vamd::OggLiveIO V;
  memset(&V, 0, sizeof(V));
  if (live) {
    const int a = L.ogg_cur, b = 1 - a;
    V.in = (const vamd::OggLive *)L.d_olive[a].p, V.out = (vamd::OggLive *)L.d_olive[b].p;
    V.rec_in = (const int32_t *)L.d_crec[a].p, V.rec_out = (int32_t *)L.d_crec[b].p;
    V.bytes_in = (const uint8_t *)L.d_cbytes[a].p, V.bytes_out = (uint8_t *)L.d_cbytes[b].p;
    V.flags = (const uint32_t *)L.d_serial.p + ns, V.gstart = (int64_t *)L.d_gstart.p;
  }
  hipLaunchKernelGGL(vamd::k_ogg_plan, dim3((unsigned)ns), dim3(64), 0, st, I, ns, (vamd::OggPage *)L.d_pages.p, (int64_t *)L.d_fbytes.p,
                     (int32_t *)L.d_npages.p, (uint8_t *)L.d_ostatus.p, V);
  hipLaunchKernelGGL(k_feed_scan, dim3(1), dim3(1024), 0, st, ns, (const int64_t *)L.d_fbytes.p, (int64_t *)L.d_foff.p);
  hipLaunchKernelGGL(vamd::k_ogg_pages, dim3((unsigned)nslots), dim3(64), 0, st, I, ns, (const vamd::OggPage *)L.d_pages.p,
                     (const int64_t *)L.d_foff.p, (const int32_t *)L.d_npages.p, (const uint8_t *)L.d_ostatus.p, O, V);
  if (live) hipLaunchKernelGGL(vamd::k_ogg_carry, dim3((unsigned)ns), dim3(64), 0, st, I, ns, V);
  FEED_TRY(hipGetLastError());
  return VAMD_OK;
}

// ... and after the group's wait: what vamd_feed_ogg hands out (of a live group's ns streams the caller's first ns_out;
// the others completed no page), and the live streams' states advance
static int pager_result(vamd_feed *f, FeedLane &L, long ns, long ns_out) {
  const uint8_t *hr = (const uint8_t *)L.h_orec.p;
  vamd_feed_ogg_result &R = L.ogg_result;
  R.nstreams = ns_out;
  R.stream_offset = (const int64_t *)(hr + 8), R.npages = (const int32_t *)(hr + orec_npages(ns)), R.status = hr + orec_status(ns);
  R.bytes = (const uint8_t *)L.h_ogg.p, R.total_bytes = *(const int64_t *)hr;
  for (long s = 0; s < ns; s++)
    if (R.status[s] & 0x80) {
      L.err = f->write_frames ? "Ogg feed: a stream needed more pages than its slots of the page table, or its live state does not hold"
                              : "Ogg feed: a stream needed more pages than its slots of the page table";
      return VAMD_EFAULT;
    }
  if (R.total_bytes + 4 > (int64_t)L.h_ogg.bytes) {
    L.err = "Ogg feed: the files exceed the bound their arena was sized by";
    return VAMD_EFAULT;
  }
  if (f->write_frames) {
    if (R.stream_offset[ns_out] != R.total_bytes) {
      L.err = "Ogg feed: a stream outside the group completed a page";
      return VAMD_EFAULT;
    }
    L.ogg_cur = 1 - L.ogg_cur;
  }
  return VAMD_OK;
}

// ---- what the two group paths share: the group's record, a size class's batch, the run the hand-over kernels take ----
// The group's record in pinned memory, which the copy kernels write and vamd_feed_packets hands out:
// [total | stream_start (ns + 1) | offset (nb) | granulepos (nb) | bits (nb) | info (nb)]
struct RecLayout {
  size_t start, offset, granulepos, bits, info, bytes;
  RecLayout(long ns, long nb) {
    start = 8, offset = start + (size_t)(ns + 1) * 8, granulepos = offset + (size_t)nb * 8, bits = granulepos + (size_t)nb * 8;
    info = bits + (size_t)nb * 4, bytes = al(info + (size_t)nb, 16);
  }
};

// where a copy kernel writes: the record and the packet arena as the device sees them, and the Ogg mirror (feed_mirror;
// the first `keep` bytes of the mirror are a managed group's earlier slices)
static int feed_out(vamd_feed *f, FeedLane &L, const RecLayout &R, long nb, size_t keep, FeedOut &O) {
  void *drec = nullptr, *dbytes = nullptr;
  FEED_TRY(hipHostGetDevicePointer(&drec, L.h_rec.p, 0));
  FEED_TRY(hipHostGetDevicePointer(&dbytes, L.h_out.p, 0));
  uint8_t *dr = (uint8_t *)drec;
  O.total = (int64_t *)dr, O.stream_start = (int64_t *)(dr + R.start), O.offset = (int64_t *)(dr + R.offset);
  O.granulepos = (int64_t *)(dr + R.granulepos), O.bits = (int32_t *)(dr + R.bits), O.info = dr + R.info;
  O.bytes = (uint8_t *)dbytes, O.cap = (int64_t)L.h_out.bytes;
  return feed_mirror(f, L, O, nb, keep);
}

// ... and behind the group's wait: what vamd_feed_packets hands out, and the two timings
static void feed_result(FeedLane &L, const RecLayout &R, long ns_out, long nb, int64_t total) {
  const uint8_t *hrec = (const uint8_t *)L.h_rec.p;
  vamd_feed_result &out = L.result;
  out.nstreams = ns_out, out.nblocks = nb;
  out.stream_start = (const int64_t *)(hrec + R.start), out.offset = (const int64_t *)(hrec + R.offset);
  out.granulepos = (const int64_t *)(hrec + R.granulepos), out.bits = (const int32_t *)(hrec + R.bits), out.info = hrec + R.info;
  out.bytes = (const uint8_t *)L.h_out.p, out.total_bytes = total;
  float up = 0.f, dev = 0.f;
  (void)hipEventElapsedTime(&up, L.ev0, L.ev_up);
  (void)hipEventElapsedTime(&dev, L.ev0, L.ev_end);
  out.upload_ms = L.src_dev ? 0. : up, out.device_ms = dev;  // (a device-fed group: nothing went up, ev0 stands before the ingest)
}

// the analysis' batch of size class W: blocks [i0, i0 + n) of the plan's, read where they lie in pcm
static void batch_of(const vamd_stream_plan &plan, int W, int64_t i0, int64_t n, const float *pcm, long cs, Buf &status,
                     vamd_batch_desc &desc, vamd_batch_io &io) {
  memset(&desc, 0, sizeof(desc));
  memset(&io, 0, sizeof(io));
  desc.W = W;
  desc.nblocks = (long)n;
  desc.lW = plan.lW[W] + i0, desc.nW = plan.nW[W] + i0, desc.blocktype = plan.blocktype[W] + i0;
  if (!n) return;
  io.pcm = pcm;
  io.pcm_src = plan.src[W] + i0;
  io.pcm_channel_stride = cs;
  io.status = (uint8_t *)status.p;
}

// the group's part of a FeedSlice (k_feed.h); the run's own lists, rows and place in the group are its caller's
static FeedSlice feed_slice_of(vamd_feed *f, const FeedLane &L, const vamd_stream_plan &plan, long ss, const long long *d_frames_of,
                               FeedLive live) {
  FeedSlice P;
  memset(&P, 0, sizeof(P));
  const int head = f->bs[1] / 2;
  P.g_start = plan.stream_start;
  for (int W = 0; W < 2; W++) P.src[W] = plan.src[W], P.status[W] = (const uint8_t *)L.d_status[W].p, P.stride[W] = f->pkcap[W], P.bs[W] = f->bs[W];
  P.ch = f->ch, P.stream_stride = ss, P.eof = head + L.frames, P.frames_of = d_frames_of, P.head = head;
  P.live = live;
  return P;
}

// ---- a bitrate-managed group ----
struct Slice {
  long k0, k1, s0, s1;  // [k0, k1) of order[]; its first stream, and one past its last
  int64_t i0[2], n[2];  // its classes' first blocks in the plan's batches, and their counts
  size_t starts;        // where its stream_start lies in `starts` (one list behind the other)
};

// The slices of a group of nb = order.size() blocks in ns streams (start[]), at most S blocks each, in order[] order -- so a
// slice holds the end of one stream, whole streams, the start of another.  order[] is rebased in place to each slice's own
// batches; starts receives every slice's stream_start over its pieces of streams, relative to its first block.  Host
// arithmetic only.  *why set: the plan is not what the slices rely on.
static std::vector<Slice> plan_slices(std::vector<int32_t> &order, const std::vector<int64_t> &start, long ns, long nb, long S,
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

// A bitrate-managed group, from its plan on: the blocks in slices of at most f->slice (plan_slices), each slice through
//   vamd_analyze_streams_mixed_managed (fifteen candidate packets per block; the ampmax chains resume per stream) ->
//   vamd_bitrate_walk (the managers resume per stream) -> the handed-out packets laid end to end behind the previous
//   slice's, straight into the pinned arena
// The workspace is bounded by the slice, not the group: a long stereo block's candidates alone take 15 x its integer
// residue (120 KB) and 15 packet rows.  The host waits once per slice for the slice's byte count (to grow the arena
// before anything is written into it: the candidates do not outlive their slice).
// (live: `live` set, ns streams planned of which the caller's first ns_out are reported; the managers carried across groups)
static int run_group_managed(vamd_feed *f, FeedLane &L, const vamd_stream_plan &plan, const float *pcm, long ns, long ss, long cs,
                             const long long *d_frames_of, FeedLive live, long ns_out) {
  const int ch = f->ch;
  const long nb = (long)(plan.nblocks[0] + plan.nblocks[1]);
  hipStream_t st = L.stream;
  std::vector<int32_t> order((size_t)(nb ? nb : 1));
  std::vector<int64_t> start((size_t)ns + 1), starts;
  FEED_CALL(vamd_plan_fetch(L.ctx, &plan, nullptr, nullptr, nullptr, nullptr, order.data(), start.data()));
  const char *why = nullptr;
  const std::vector<Slice> sl = plan_slices(order, start, ns, nb, f->slice, starts, &why);
  if (why) {
    L.err = why;
    return VAMD_EFAULT;
  }
  // all slices' lists in one upload: [the slice's byte count on its way back (16) | order[] rebased | the stream_starts]
  const size_t order_bytes = al((size_t)(nb ? nb : 1) * 4, 8), lists = order_bytes + starts.size() * 8;
  FEED_TRY(L.h_slice.need(lists + 16));
  FEED_TRY(L.d_slice.need(lists + 16));
  int64_t *h_total = (int64_t *)L.h_slice.p;
  uint8_t *hl = (uint8_t *)L.h_slice.p + 16, *dl = (uint8_t *)L.d_slice.p + 16;
  memcpy(hl, order.data(), (size_t)nb * 4);
  memcpy(hl + order_bytes, starts.data(), starts.size() * 8);
  FEED_TRY(hipMemcpyAsync(dl, hl, lists, hipMemcpyHostToDevice, st));
  const int32_t *d_order = (const int32_t *)dl;
  const int64_t *d_starts = (const int64_t *)(dl + order_bytes);
  // the slice's buffers, sized for the largest slice of each class
  const int K = VAMD_PACKETBLOBS;
  for (int W = 0; W < 2; W++) {
    int64_t most = 1;
    for (const Slice &x : sl) most = x.n[W] > most ? x.n[W] : most;
    const size_t m = (size_t)most, n2 = (size_t)f->bs[W] / 2;
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
  const size_t most_slice = (size_t)(f->slice < nb ? f->slice : (nb ? nb : 1));
  FEED_TRY(L.d_rel.need(most_slice * 8));
  FEED_TRY(L.d_sid.need(most_slice * 4));
  FEED_TRY(L.d_sbytes.need((size_t)ns * 8));
  FEED_TRY(L.d_soff.need((size_t)(ns + 1) * 8));
  if (!live.in) {  // (a live lane's managers live across groups: k_live_begin starts the fresh ones)
    FEED_TRY(L.d_bstate.need((size_t)ns * sizeof(vamd_bitrate_state)));
    FEED_CALL(vamd_bitrate_init_states(L.ctx, (vamd_bitrate_state *)L.d_bstate.p, ns));
  }
  const RecLayout R(ns, nb);
  FEED_TRY(L.h_rec.need(R.bytes + R.bytes / 4));
  FeedSlice P = feed_slice_of(f, L, plan, ss, d_frames_of, live);
  for (int W = 0; W < 2; W++) {
    P.choice[W] = (const int32_t *)L.d_choice[W].p, P.fbits[W] = (const int32_t *)L.d_fbits[W].p, P.mbits[W] = (const int32_t *)L.d_mbits[W].p;
    P.packets[W] = (const uint8_t *)L.d_mpk[W].p;
  }
  int64_t base = 0;  // bytes of the packets laid out so far
  for (const Slice &x : sl) {
    const long nss = x.s1 - x.s0, nbs = x.k1 - x.k0;
    P.order = d_order + x.k0, P.stream_start = d_starts + x.starts;
    P.i0[0] = x.i0[0], P.i0[1] = x.i0[1], P.k0 = x.k0, P.s0 = x.s0;
    // analyse: the slice's fifteen candidates per block
    vamd_batch_desc desc[2];
    vamd_batch_io io[2];
    vamd_managed_io m[2];
    for (int W = 0; W < 2; W++) {
      batch_of(plan, W, x.i0[W], x.n[W], pcm, cs, L.d_status[W], desc[W], io[W]);
      memset(&m[W], 0, sizeof(m[W]));
      if (!x.n[W]) continue;
      m[W].posts = (int32_t *)L.d_mposts[W].p;
      m[W].post_valid = (int32_t *)L.d_mvalid[W].p;
      m[W].iwork = (int32_t *)L.d_miwork[W].p;
      m[W].nonzero = (int32_t *)L.d_mnz[W].p;
      m[W].packets = (uint8_t *)L.d_mpk[W].p;
      m[W].packet_bits = (int32_t *)L.d_mbits[W].p;
      m[W].packet_stride = f->pkcap[W];
    }
    FEED_CALL(vamd_analyze_streams_mixed_managed(L.ctx, &desc[0], &io[0], &m[0], &desc[1], &io[1], &m[1], P.order, P.stream_start, nss, nbs,
                                                 (float *)L.d_amp.p + x.s0));
    // walk: the managers' choice and the size they hand out
    int32_t *choice[2] = {(int32_t *)L.d_choice[0].p, (int32_t *)L.d_choice[1].p};
    int32_t *fbits[2] = {(int32_t *)L.d_fbits[0].p, (int32_t *)L.d_fbits[1].p};
    FEED_CALL(vamd_bitrate_walk(L.ctx, P.order, P.stream_start, nss, P.mbits, P.status, (vamd_bitrate_state *)L.d_bstate.p + x.s0, choice, fbits));
    // sizes, and the wait for their sum
    hipLaunchKernelGGL(k_feed_sid, dim3((unsigned)nss), dim3(64), 0, st, P.stream_start, (int32_t *)L.d_sid.p);
    hipLaunchKernelGGL(k_feed_sizes, dim3((unsigned)nss), dim3(64), 0, st, P, (int64_t *)L.d_rel.p, (int64_t *)L.d_sbytes.p);
    hipLaunchKernelGGL(k_feed_scan, dim3(1), dim3(1024), 0, st, nss, (const int64_t *)L.d_sbytes.p, (int64_t *)L.d_soff.p);
    FEED_TRY(hipGetLastError());
    FEED_TRY(hipMemcpyAsync(h_total, (const int64_t *)L.d_soff.p + nss, 8, hipMemcpyDeviceToHost, st));
    FEED_TRY(hipStreamSynchronize(st));
    // grow the arena (and the mirror) where the slice needs it, the earlier slices' packets kept; copy
    const int64_t need = base + *h_total;
    if (need > (int64_t)L.h_out.bytes) FEED_TRY(L.h_out.grow_keeping((size_t)need + (size_t)need / 8, (size_t)base));
    FeedOut O;
    FEED_OWN(feed_out(f, L, R, nb, (size_t)base, O));
    hipLaunchKernelGGL(k_feed_copy_managed, dim3((unsigned)((nbs + 3) / 4)), dim3(256), 0, st, P, nbs, base, (const int64_t *)L.d_rel.p,
                       (const int64_t *)L.d_soff.p, (const int32_t *)L.d_sid.p, O);
    FEED_TRY(hipGetLastError());
    base = need;
  }
  if (f->ogg && sl.empty()) {  // (a live group without a block: no slice has made the mirror the pager is given)
    FeedOut O;
    FEED_OWN(feed_out(f, L, R, nb, 0, O));
  }
  if (f->ogg) FEED_OWN(run_pager(f, L, plan.stream_start, ns, nb, nullptr));
  FEED_TRY(hipEventRecord(L.ev_end, st));
  FEED_TRY(hipEventSynchronize(L.ev_end));
  if (f->ogg) FEED_OWN(pager_result(f, L, ns, ns_out));
  uint8_t *hrec = (uint8_t *)L.h_rec.p;  // (the total and stream_start, which a VBR group's copy kernel writes, from here)
  *(int64_t *)hrec = base;
  memcpy(hrec + R.start, start.data(), (size_t)(ns + 1) * 8);
  feed_result(L, R, ns_out, nb, base);
  return VAMD_OK;
}

// A decoded feed's group, behind its packets' hand-over: the streams' geometry up, k_synth per size class and the lap
// (vamd_synth_streams: out of what the analysis left in the lane's context), ev_dec behind them.  Stream s takes
// ch * frames[s] floats of the arena whether or not it gets a signal.
static int enqueue_decoded(vamd_feed *f, FeedLane &L, const vamd_stream_plan &plan, long ns) {
  L.dec_frames.resize((size_t)ns), L.dec_offset.resize((size_t)ns + 1);
  FEED_TRY(L.h_dgeo.need((size_t)ns * 16));
  FEED_TRY(L.d_dgeo.need((size_t)ns * 16));
  int64_t *h = (int64_t *)L.h_dgeo.p, at = 0;
  for (long s = 0; s < ns; s++) {
    const int64_t fr = L.frames_of.empty() ? L.frames : L.frames_of[(size_t)s];
    h[s] = L.dec_frames[(size_t)s] = fr;
    h[ns + s] = L.dec_offset[(size_t)s] = at;
    at += fr * f->ch;
  }
  L.dec_offset[(size_t)ns] = at;
  for (int W = 0; W < 2; W++) FEED_TRY(L.d_synth[W].need(((size_t)plan.nblocks[W] * f->ch * (size_t)f->bs[W] + 4) * 4));
  FEED_TRY(L.d_dec.need(((size_t)at + 4) * 4));
  FEED_TRY(hipMemcpyAsync(L.d_dgeo.p, h, (size_t)ns * 16, hipMemcpyHostToDevice, L.stream));
  FEED_CALL(vamd_synth_streams(L.ctx, &plan, ns, L.frames, (const int64_t *)L.d_dgeo.p, (const int64_t *)L.d_dgeo.p + ns,
                               plan.nblocks[0] ? (float *)L.d_synth[0].p : nullptr, plan.nblocks[1] ? (float *)L.d_synth[1].p : nullptr,
                               (float *)L.d_dec.p));
  FEED_TRY(hipEventRecord(L.ev_dec, L.stream));
  return VAMD_OK;
}

// ... and what vamd_feed_decoded hands out, once the group's record is home: a stream that lost a packet has no signal
static void decoded_result(vamd_feed *f, FeedLane &L, long ns) {
  L.dec_status.assign((size_t)ns, 0);
  const vamd_feed_result &r = L.result;
  for (long s = 0; s < ns; s++) {
    for (int64_t k = r.stream_start[s]; k < r.stream_start[s + 1]; k++)
      if (r.bits[k] < 0) {  // no packet, no signal -- whatever the block's status bits say
        L.dec_status[(size_t)s] = (uint8_t)((r.info[k] >> 2) & 3);
        L.dec_frames[(size_t)s] = 0;
        break;
      }
  }
  vamd_feed_decoded_result &o = L.dec_result;
  o.nstreams = ns, o.channels = f->ch;
  o.frames = L.dec_frames.data(), o.offset = L.dec_offset.data(), o.status = L.dec_status.data();
  o.pcm = (const float *)L.d_dec.p, o.total_floats = L.dec_offset[(size_t)ns];
}

// a group from its plan on (whole or live): the analysis, the packets end to end into the pinned arena
static int finish_group(vamd_feed *f, FeedLane &L, const vamd_stream_plan &plan, const float *pcm, long ns, long ss, long cs,
                        const long long *d_frames_of, FeedLive live, long ns_out) {
  hipStream_t st = L.stream;
  if (f->managed) return run_group_managed(f, L, plan, pcm, ns, ss, cs, d_frames_of, live, ns_out);
  const long nb = (long)(plan.nblocks[0] + plan.nblocks[1]);
  vamd_batch_desc desc[2];
  vamd_batch_io io[2];
  for (int W = 0; W < 2; W++) {
    const size_t n = (size_t)plan.nblocks[W];
    FEED_TRY(L.d_pk[W].need((n ? n : 1) * (size_t)f->pkcap[W]));
    FEED_TRY(L.d_bits[W].need((n ? n : 1) * 4));
    FEED_TRY(L.d_status[W].need((n ? n : 1) * (size_t)f->ch));
    batch_of(plan, W, 0, plan.nblocks[W], pcm, cs, L.d_status[W], desc[W], io[W]);
    if (!n) continue;
    io[W].packets = (uint8_t *)L.d_pk[W].p;
    io[W].packet_bits = (int32_t *)L.d_bits[W].p;
    io[W].packet_stride = f->pkcap[W];
  }
  if (nb)
    FEED_CALL(vamd_analyze_streams_mixed(L.ctx, &desc[0], &io[0], &desc[1], &io[1], plan.order, plan.stream_start, ns, nb,
                                         (float *)L.d_amp.p));
  // the packets end to end, into the pinned arena
  FEED_TRY(L.d_rel.need((size_t)(nb ? nb : 1) * 8));
  FEED_TRY(L.d_sid.need((size_t)(nb ? nb : 1) * 4));
  FEED_TRY(L.d_sbytes.need((size_t)ns * 8));
  FEED_TRY(L.d_soff.need((size_t)(ns + 1) * 8));
  const RecLayout R(ns, nb);
  FEED_TRY(L.h_rec.need(R.bytes + R.bytes / 4));
  FeedSlice P = feed_slice_of(f, L, plan, ss, d_frames_of, live);  // (the whole group as one run: k_feed.h)
  P.order = plan.order, P.stream_start = plan.stream_start;
  for (int W = 0; W < 2; W++) P.fbits[W] = (const int32_t *)L.d_bits[W].p, P.packets[W] = (const uint8_t *)L.d_pk[W].p;
  for (int attempt = 0;; attempt++) {
    FeedOut O;
    FEED_OWN(feed_out(f, L, R, nb, 0, O));
    hipLaunchKernelGGL(k_feed_sid, dim3((unsigned)ns), dim3(64), 0, st, plan.stream_start, (int32_t *)L.d_sid.p);
    hipLaunchKernelGGL(k_feed_sizes, dim3((unsigned)ns), dim3(64), 0, st, P, (int64_t *)L.d_rel.p, (int64_t *)L.d_sbytes.p);
    hipLaunchKernelGGL(k_feed_scan, dim3(1), dim3(1024), 0, st, ns, (const int64_t *)L.d_sbytes.p, (int64_t *)L.d_soff.p);
    const long waves = (nb > ns + 1 ? nb : ns + 1);
    hipLaunchKernelGGL(k_feed_copy, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, P, ns, nb, (const int64_t *)L.d_rel.p,
                       (const int64_t *)L.d_soff.p, (const int32_t *)L.d_sid.p, O);
    FEED_TRY(hipGetLastError());
    if (f->ogg) FEED_OWN(run_pager(f, L, plan.stream_start, ns, nb, (const int64_t *)L.d_soff.p + ns));
    FEED_TRY(hipEventRecord(L.ev_end, st));
    // (the decoded signal is enqueued behind the hand-over's event and ahead of the wait for it: the packets are ready no
    // later than without it, and the lane's stream goes on while the host looks at them)
    if (f->decoded && !attempt) FEED_OWN(enqueue_decoded(f, L, plan, ns));
    FEED_TRY(hipEventSynchronize(L.ev_end));
    const int64_t total = *(const int64_t *)L.h_rec.p;
    if (total <= (int64_t)L.h_out.bytes) {
      if (f->ogg) FEED_OWN(pager_result(f, L, ns, ns_out));
      feed_result(L, R, ns_out, nb, total);
      if (f->decoded) decoded_result(f, L, ns);
      return VAMD_OK;
    }
    if (attempt) {
      L.err = "packet arena still too small after growing it";
      return VAMD_EFAULT;
    }
    FEED_TRY(L.h_out.need((size_t)total + (size_t)total / 8));  // the packets are still in HBM: lay them out again
  }
}

// The group's samples up: in_bytes of the pinned input arena into d_in, and a small list beside them (side_bytes from
// side_src, pinned, to side_dst; 0: none), between the events the upload time is read from; returns when they are up.
// ONE upload at a time per device.  The link is a single resource: lanes that upload side by side each get a share
// of it and all finish late together -- and then all compute together while the link idles (measured: three lanes
// in lockstep, 2.3 ms of every 13 without a single kernel on the chip).  Taking turns, a lane has the whole link,
// starts its kernels the moment its samples are up, and the next lane's upload runs beside them: the lanes stagger
// themselves.
static int upload(FeedLane &L, size_t in_bytes, void *side_dst = nullptr, const void *side_src = nullptr, size_t side_bytes = 0) {
  std::lock_guard<std::mutex> turn(*L.upload_turn);
  FEED_TRY(hipEventRecord(L.ev0, L.stream));
  if (in_bytes) FEED_TRY(hipMemcpyAsync(L.d_in.p, L.h_in.p, in_bytes, hipMemcpyHostToDevice, L.stream));
  if (side_bytes) FEED_TRY(hipMemcpyAsync(side_dst, side_src, side_bytes, hipMemcpyHostToDevice, L.stream));
  FEED_TRY(hipEventRecord(L.ev_up, L.stream));
  FEED_TRY(hipEventSynchronize(L.ev_up));
  return VAMD_OK;
}

// an ingest kernel over the group's samples as their type has it (k16: 16-bit, k32: float; d_in in front of args): `items`
// threads' worth of work in workgroups of 256, at most 8192 of them (the kernels stride)
template <typename K16, typename K32, typename... A>
static void launch_ingest(const FeedLane &L, K16 *k16, K32 *k32, long items, A... args) {
  long blocks = (items + 255) / 256;
  if (blocks > 256L * 32) blocks = 256L * 32;
  if (blocks < 1) blocks = 1;
  if (L.format == VAMD_FEED_S16) hipLaunchKernelGGL(k16, dim3((unsigned)blocks), dim3(256), 0, L.stream, (const int16_t *)L.d_in.p, args...);
  else hipLaunchKernelGGL(k32, dim3((unsigned)blocks), dim3(256), 0, L.stream, (const float *)L.d_in.p, args...);
}

// A device-fed group's start, in upload()'s place: the lane's stream waits for the producer's event (recorded by
// vamd_feed_wrote_device on the caller's thread), the side list goes up, and the timing events stand where the ingest begins.
// No upload turn: the link carries a few bytes per stream.
static int source_begin(FeedLane &L, void *side_dst = nullptr, const void *side_src = nullptr, size_t side_bytes = 0) {
  FEED_TRY(hipStreamWaitEvent(L.stream, L.ev_src, 0));
  if (side_bytes) FEED_TRY(hipMemcpyAsync(side_dst, side_src, side_bytes, hipMemcpyHostToDevice, L.stream));
  FEED_TRY(hipEventRecord(L.ev0, L.stream));
  FEED_TRY(hipEventRecord(L.ev_up, L.stream));
  return VAMD_OK;
}

// ... and behind its ingest's launch: the event vamd_feed_source_done hands out, and the word that it stands
static int source_ingested(vamd_feed *f, FeedLane &L) {
  const hipError_t e = hipEventRecord(L.ev_ingest, L.stream);
  {
    std::lock_guard<std::mutex> g(f->m);
    L.ingest_queued = true, L.ingest_recorded = e == hipSuccess;
  }
  f->cv_done.notify_all();
  FEED_TRY(e);
  return VAMD_OK;
}

// a device-fed group's ingest kernel by the group's element type (args: the kernel's)
#define FEED_LAUNCH_DEV(kernel, L, items, ...)                                                                                      \
  do {                                                                                                                              \
    long blocks__ = ((items) + 255) / 256;                                                                                          \
    if (blocks__ > 256L * 32) blocks__ = 256L * 32;                                                                                 \
    if (blocks__ < 1) blocks__ = 1;                                                                                                 \
    const dim3 g__((unsigned)blocks__), b__(256);                                                                                   \
    switch ((L).src_dtype) {                                                                                                        \
      case VAMD_SRC_S16: hipLaunchKernelGGL(kernel<int16_t>, g__, b__, 0, (L).stream, __VA_ARGS__); break;                          \
      case VAMD_SRC_F32: hipLaunchKernelGGL(kernel<float>, g__, b__, 0, (L).stream, __VA_ARGS__); break;                            \
      case VAMD_SRC_F16: hipLaunchKernelGGL(kernel<vamd::src_f16>, g__, b__, 0, (L).stream, __VA_ARGS__); break;                    \
      default: hipLaunchKernelGGL(kernel<vamd::src_bf16>, g__, b__, 0, (L).stream, __VA_ARGS__); break;                             \
    }                                                                                                                               \
  } while (0)

// a whole-stream group from device memory: run_group with the streams' base pointers in first_of's place ([frames_of |
// base_of], one copy), no d_in and no upload; the plan is always the one of streams of unequal length
static int run_group_device(vamd_feed *f, FeedLane &L) {
  const long ns = L.nstreams, frames = L.frames;
  const int ch = f->ch, head = f->bs[1] / 2, pad = 3 * f->bs[1];
  const long cs = (long)al((size_t)head + ((frames + 3) & ~3L) + pad, 64), ss = cs * ch;
  FEED_TRY(L.d_pcm.need((size_t)ns * ss * 4));
  FEED_TRY(L.d_states.need((size_t)ns * sizeof(vamd_envelope_state)));
  FEED_TRY(L.d_amp.need((size_t)ns * 4));
  FEED_TRY(L.h_len.need((size_t)ns * 16));
  FEED_TRY(L.d_len.need((size_t)ns * 16));
  long long *h = (long long *)L.h_len.p;
  for (long i = 0; i < ns; i++) h[i] = L.frames_of[(size_t)i], h[ns + i] = (long long)(uintptr_t)L.src_base[(size_t)i];
  const long long *d_frames_of = (const long long *)L.d_len.p, *d_base_of = d_frames_of + ns;
  FEED_OWN(source_begin(L, L.d_len.p, h, (size_t)ns * 16));
  FEED_LAUNCH_DEV(k_feed_ingest_dev, L, ns * ((long)(head >> 2) + ((frames + 3) >> 2) + (pad >> 2)), ch, ns, frames, head, pad, (float *)L.d_pcm.p,
                  ss, cs, (float *)L.d_amp.p, (vamd_envelope_state *)L.d_states.p, d_frames_of, d_base_of, L.src_cstride, L.src_fstride);
  const hipError_t launched = hipGetLastError();
  FEED_OWN(source_ingested(f, L));
  FEED_TRY(launched);
  vamd_stream_plan plan;
  FEED_CALL(vamd_plan_streams_whole_v(L.ctx, (float *)L.d_pcm.p, ss, cs, ns, frames, L.frames_of.data(), (vamd_envelope_state *)L.d_states.p, &plan));
  FeedLive none;
  none.in = nullptr, none.nan = nullptr;
  return finish_group(f, L, plan, (const float *)L.d_pcm.p, ns, ss, cs, d_frames_of, none, ns);
}

// one group through its lane (the lane's own thread; its device is current)
static int run_group(vamd_feed *f, FeedLane &L) {
  if (L.src_dev) return run_group_device(f, L);
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
  FEED_OWN(upload(L, in_bytes));
  launch_ingest(L, k_feed_ingest<int16_t>, k_feed_ingest<float>, ns * ((long)(head >> 2) + ((frames + 3) >> 2) + (pad >> 2)), ch, ns, frames,
                head, pad, (float *)L.d_pcm.p, ss, cs, (float *)L.d_amp.p, (vamd_envelope_state *)L.d_states.p, d_frames_of, d_first_of);
  FEED_TRY(hipGetLastError());
  vamd_stream_plan plan;
  if (uneven)
    FEED_CALL(vamd_plan_streams_whole_v(L.ctx, (float *)L.d_pcm.p, ss, cs, ns, frames, L.frames_of.data(), (vamd_envelope_state *)L.d_states.p, &plan));
  else
    FEED_CALL(vamd_plan_streams_whole(L.ctx, (float *)L.d_pcm.p, ss, cs, ns, frames, (vamd_envelope_state *)L.d_states.p, &plan));
  FeedLive none;
  none.in = nullptr, none.nan = nullptr;
  return finish_group(f, L, plan, (const float *)L.d_pcm.p, ns, ss, cs, d_frames_of, none, ns);
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
    if (L.src_dev) in.first = i < nsc ? (int64_t)(uintptr_t)L.src_base[(size_t)i] : 0;  // (a device-fed piece: where it lies)
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
  if (L.src_dev) FEED_OWN(source_begin(L, L.d_live.p, hin, (size_t)ns * sizeof(LiveIn)));
  else {
    FEED_TRY(L.d_in.need(in_bytes ? in_bytes : 16));
    FEED_OWN(upload(L, in_bytes, L.d_live.p, hin, (size_t)ns * sizeof(LiveIn)));
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
    if (L.src_dev) {
      FEED_LAUNCH_DEV(k_live_ingest_dev, L, ns * (long)quads, ch, ns, (long)quads, pad + 256, d_live, (const float *)L.d_buf[L.cur].p,
                      (float *)L.d_buf[1 - L.cur].p, ss, cs, (unsigned long long *)L.d_nan.p, (int *)d_lstatus, L.src_cstride, L.src_fstride);
      const hipError_t launched = hipGetLastError();
      FEED_OWN(source_ingested(f, L));
      FEED_TRY(launched);
    } else {
      launch_ingest(L, k_live_ingest<int16_t>, k_live_ingest<float>, ns * (long)quads, ch, ns, (long)quads, pad + 256, d_live,
                    (const float *)L.d_buf[L.cur].p, (float *)L.d_buf[1 - L.cur].p, ss, cs, (unsigned long long *)L.d_nan.p, (int *)d_lstatus);
      FEED_TRY(hipGetLastError());
    }
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
  if (f->ogg) {  // what the pager needs to know of each stream: it begins with this group, ends with it, or is not there
    L.ogg_flags.assign((size_t)ns, 0);
    for (long i = 0; i < ns; i++) {
      const bool absent = hin[i].fresh && !hin[i].frames;
      L.ogg_flags[(size_t)i] = absent ? vamd::OGG_LIVE_ABSENT : (hin[i].fresh ? vamd::OGG_LIVE_BEGIN : 0) | (hin[i].close ? vamd::OGG_LIVE_CLOSE : 0);
      if ((size_t)i < L.flush.size() && L.flush[(size_t)i]) L.ogg_flags[(size_t)i] |= vamd::OGG_LIVE_FLUSH;  // (the pager decides whom it concerns)
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
  f->lanes.clear();  // (~FeedLane, each on its own device)
  (void)hipSetDevice(cur);
}

// why this thread's last vamd_feed_create failed (vamd_feed_last_error(NULL))
thread_local std::string feed_create_err;

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
    r = vamd_create(&L.ctx, setup_blob, blob_bytes, L.device);
    if (r) break;
    hipError_t e = hipSetDevice(L.device);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&L.stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L.ev0, hipEventDefault);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L.ev_up, hipEventBlockingSync);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L.ev_end, hipEventBlockingSync);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L.ev_src, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&L.ev_ingest, hipEventDisableTiming | hipEventBlockingSync);
    if (e == hipSuccess && decoded) e = hipEventCreateWithFlags(&L.ev_dec, hipEventDisableTiming | hipEventBlockingSync);
    if (e == hipSuccess && vamd_set_stream(L.ctx, L.stream) != VAMD_OK) e = hipErrorUnknown;
    if (e == hipSuccess && l == 0) {
      f->ch = vamd_channels(L.ctx);
      for (int W = 0; W < 2; W++) f->bs[W] = vamd_blocksize(L.ctx, W), f->pkcap[W] = vamd_packet_capacity(L.ctx, W);
      if (f->pkcap[0] <= 0 || f->pkcap[1] <= 0) r = VAMD_EIMPL;  // packets of this mode are not assembled on the GPU
      for (int W = 0; W < 2 && !r && decoded; W++) {  // ... or its blocks not synthesised
        if (vamd_synth_check(L.ctx, W) != VAMD_OK) {
          feed_create_err = std::string("VAMD_FEED_DECODED: ") + vamd_last_error(L.ctx);
          r = VAMD_EIMPL;
        }
      }
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
    if (e == hipSuccess && !r && !no_arena) e = L.h_in.need(in_cap);
    const size_t out_cap = f->out_bytes ? (size_t)f->out_bytes : (size_t)max_streams * max_frames * f->ch + (size_t)max_streams * 65536;
    if (e == hipSuccess && !r) e = L.h_out.need(al(out_cap, 4096));
    if (decoded && !r) {  // the decoded arena, and k_synth's scratch for a group of long blocks (half overlapped: twice its samples)
      const size_t group = (size_t)max_streams * max_frames * f->ch;
      if (e == hipSuccess) e = L.d_dec.need((group + 4) * 4);
      if (e == hipSuccess) e = L.d_synth[1].need((2 * group + (size_t)max_streams * 4 * f->bs[1] * f->ch) * 4);
    }
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
// A live group: a serial number belongs to a stream, not to a group -- only a stream that begins with this group (its
// slot is free and the piece has frames) takes one, the counter's next or the one named for it; an open stream keeps its own.
static void ogg_job(vamd_feed *f, FeedLane &L, long nstreams) {
  memset(&L.ogg_result, 0, sizeof(L.ogg_result));
  if (!f->ogg) return;
  L.serials.assign((size_t)nstreams, 0);
  for (long s = 0; s < nstreams; s++)
    if (!f->write_frames) L.serials[(size_t)s] = f->next_serial++;
    else if (!L.live[(size_t)s].open && L.frames_of[(size_t)s])
      L.serials[(size_t)s] = (size_t)s < L.user_serials.size() ? L.user_serials[(size_t)s] : f->next_serial++;
  if (!f->write_frames)
    for (size_t s = 0; s < L.user_serials.size() && s < (size_t)nstreams; s++) L.serials[s] = L.user_serials[s];
  L.user_serials.clear();
  // ... and its comment headers: what vamd_feed_ogg_comments set for the slot, of a live group only those of the streams
  // that begin with it; none left: a group like any other
  L.comments.swap(L.user_comments);
  L.user_comments.clear();
  if (L.comments.size() > (size_t)nstreams) L.comments.resize((size_t)nstreams);
  bool any = false;
  for (size_t s = 0; s < L.comments.size(); s++) {
    if (f->write_frames && (L.live[s].open || !L.frames_of[s])) L.comments[s].clear();
    any |= !L.comments[s].empty();
  }
  if (!any) L.comments.clear();
  // ... and the streams it flushes (vamd_feed_ogg_flush), of the caller's streams only
  L.flush.swap(L.user_flush);
  L.user_flush.clear();
  if (L.flush.size() > (size_t)nstreams) L.flush.resize((size_t)nstreams);
}

// the tail of vamd_feed_wrote / _wrote_v / _wrote_live (f->m held; the lane's frames_of / close_of are set): the group
// goes to its lane's thread
static int queue_group(vamd_feed *f, FeedLane &L, long nstreams, long frames, bool src_dev = false) {
  L.nstreams = nstreams, L.frames = frames, L.format = f->format;
  L.src_dev = src_dev, L.ingest_queued = L.ingest_recorded = false;
  L.status = 0;
  memset(&L.result, 0, sizeof(L.result));
  memset(&L.dec_result, 0, sizeof(L.dec_result));
  ogg_job(f, L, nstreams);
  L.t_wrote = now_s();
  L.state = LANE_QUEUED;
  f->cv_work.notify_all();
  return VAMD_OK;
}

// vamd_feed_packets / vamd_feed_ogg: waits for the slot's group, then hands out what its lane holds for the caller
template <typename R>
static int await_group(vamd_feed *f, int slot, R FeedLane::*result, R *out, bool ogg) {
  if (!f || !out || slot < 0 || slot >= (int)f->lanes.size()) return VAMD_EINVAL;
  std::unique_lock<std::mutex> g(f->m);
  if (ogg && !f->ogg) {
    f->err = "vamd_feed_ogg: the feed has no Ogg headers (vamd_feed_ogg_headers / vamd_feed_ogg_headers_live)";
    return VAMD_EINVAL;
  }
  FeedLane &L = f->lanes[(size_t)slot];
  if (L.state != LANE_QUEUED && L.state != LANE_DONE) return VAMD_EINVAL;
  f->cv_done.wait(g, [&] { return f->stop || L.state == LANE_DONE; });
  if (L.state != LANE_DONE) return VAMD_EFAULT;
  *out = L.*result;
  return L.status;
}

static uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24; }

// vamd_feed_ogg_headers / _live (f->m held; `call` names the one): the three packets validated, the feed an Ogg feed
static int ogg_headers_set(vamd_feed *f, const char *call, const void *id, long id_bytes, const void *comment, long comment_bytes,
                           const void *setup, long setup_bytes) {
  if (f->turn) {
    f->err = std::string(call) + " comes before the first vamd_feed_buffer";
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

int vamd_feed_ogg_comments(vamd_feed *f, int slot, const void *const *comment, const long *bytes, long n) {
  if (!f || slot < 0 || slot >= (int)f->lanes.size()) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  FeedLane &L = f->lanes[(size_t)slot];
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
  L.user_comments.swap(all);
  return VAMD_OK;
}

int vamd_feed_ogg_flush(vamd_feed *f, int slot, const uint8_t *flush, long n) {
  if (!f || slot < 0 || slot >= (int)f->lanes.size()) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  FeedLane &L = f->lanes[(size_t)slot];
  if (!f->write_frames || !f->ogg || L.state != LANE_FILLING || n < 0 || n > f->max_streams) {
    f->err = !f->write_frames ? "vamd_feed_ogg_flush is for a live Ogg feed (vamd_feed_create_live, vamd_feed_ogg_headers_live): a whole stream's file has no open page to flush"
             : !f->ogg        ? "vamd_feed_ogg_flush: the feed has no Ogg headers (vamd_feed_ogg_headers_live)"
                              : "vamd_feed_ogg_flush: a slot between vamd_feed_buffer and vamd_feed_wrote_live, 0 to max_streams flags";
    return VAMD_EINVAL;
  }
  L.user_flush.assign((size_t)n, 1);  // (flush == NULL: every one of the first n)
  if (flush)
    for (long s = 0; s < n; s++) L.user_flush[(size_t)s] = flush[s] != 0;
  return VAMD_OK;
}

int vamd_feed_ogg(vamd_feed *f, int slot, vamd_feed_ogg_result *out) { return await_group(f, slot, &FeedLane::ogg_result, out, true); }

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

// the tail of the two: the source is the lane's, the producer's event recorded (the lane's device current), the group queued
static int queue_group_device(vamd_feed *f, FeedLane &L, long nstreams, long frames, const vamd_feed_source *src) {
  const hipError_t e = hipEventRecord(L.ev_src, (hipStream_t)src->producer);
  if (e != hipSuccess) {
    f->err = std::string("device-fed group: hipEventRecord on the producer's stream: ") + hipGetErrorString(e);
    return VAMD_EINVAL;
  }
  L.src_base.assign(src->base, src->base + nstreams);
  L.src_dtype = src->dtype, L.src_cstride = src->channel_stride, L.src_fstride = src->frame_stride;
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
  if (!f || !frames || slot < 0 || slot >= (int)f->lanes.size()) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  if (f->write_frames) {
    f->err = "vamd_feed_wrote_device is for a whole-stream feed; a live feed takes vamd_feed_wrote_live_device";
    return VAMD_EINVAL;
  }
  FeedLane &L = f->lanes[(size_t)slot];
  if (nstreams < 1 || nstreams > f->max_streams || L.state != LANE_FILLING) {
    f->err = "vamd_feed_wrote_device: a slot between vamd_feed_buffer and its group, 1 to max_streams streams";
    return VAMD_EINVAL;
  }
  long longest = 0;
  for (long i = 0; i < nstreams; i++) {
    if (frames[i] < 1 || frames[i] > f->max_frames) {
      f->err = "vamd_feed_wrote_device: stream " + std::to_string(i) + " has " + std::to_string(frames[i]) + " frames, not 1 to max_frames";
      return VAMD_EINVAL;
    }
    if (frames[i] > longest) longest = (long)frames[i];
  }
  DeviceScope on(L.device);
  FEED_OWN(source_check(f, L, nstreams, frames, src));
  L.frames_of.assign(frames, frames + nstreams);
  return queue_group_device(f, L, nstreams, longest, src);
}

int vamd_feed_wrote_live_device(vamd_feed *f, int slot, long nstreams, const int64_t *frames, const uint8_t *close, const vamd_feed_source *src) {
  if (!f || !frames || slot < 0 || slot >= (int)f->lanes.size()) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  if (!f->write_frames) {
    f->err = "vamd_feed_wrote_live_device is for a live feed (vamd_feed_create_live); a whole-stream feed takes vamd_feed_wrote_device";
    return VAMD_EINVAL;
  }
  FeedLane &L = f->lanes[(size_t)slot];
  if (nstreams < 1 || nstreams > f->max_streams || L.state != LANE_FILLING) {
    f->err = "vamd_feed_wrote_live_device: a slot between vamd_feed_buffer and its group, 1 to max_streams streams";
    return VAMD_EINVAL;
  }
  for (long i = 0; i < nstreams; i++) {
    if (frames[i] < 0 || frames[i] > f->max_frames) {
      f->err = "vamd_feed_wrote_live_device: stream " + std::to_string(i) + " has " + std::to_string(frames[i]) + " frames, not 0 to max_frames";
      return VAMD_EINVAL;
    }
    if (close && close[i] && !frames[i] && !L.live[(size_t)i].open) {  // (closing a stream that never had a frame)
      f->err = "vamd_feed_wrote_live_device: stream " + std::to_string(i) + " is closed and never had a frame";
      return VAMD_EINVAL;
    }
  }
  DeviceScope on(L.device);
  FEED_OWN(source_check(f, L, nstreams, frames, src));
  L.frames_of.assign(frames, frames + nstreams);
  L.close_of.assign((size_t)nstreams, 0);
  if (close)
    for (long i = 0; i < nstreams; i++) L.close_of[(size_t)i] = close[i] != 0;
  return queue_group_device(f, L, nstreams, f->max_frames, src);
}

int vamd_feed_source_done(vamd_feed *f, int slot, void *consumer, int wait_on_host) {
  if (!f || slot < 0 || slot >= (int)f->lanes.size()) return VAMD_EINVAL;
  std::unique_lock<std::mutex> g(f->m);
  FeedLane &L = f->lanes[(size_t)slot];
  if ((L.state != LANE_QUEUED && L.state != LANE_DONE) || !L.src_dev) {
    f->err = "vamd_feed_source_done: the slot holds no device-fed group";
    return VAMD_EINVAL;
  }
  f->cv_done.wait(g, [&] { return f->stop || L.ingest_queued || L.state == LANE_DONE; });
  if (f->stop) return VAMD_EFAULT;
  if (!L.ingest_recorded) return VAMD_OK;  // (the group failed before its ingest: nothing of the lane's reads the source)
  const hipEvent_t ev = L.ev_ingest;
  g.unlock();  // (the event is this group's until the slot is released, which is the caller's to do)
  if (consumer && hipStreamWaitEvent((hipStream_t)consumer, ev, 0) != hipSuccess) return VAMD_EFAULT;
  if (wait_on_host && hipEventSynchronize(ev) != hipSuccess) return VAMD_EFAULT;
  return VAMD_OK;
}

int vamd_feed_wrote(vamd_feed *f, int slot, long nstreams, long frames) {
  if (!f || slot < 0 || slot >= (int)f->lanes.size() || f->write_frames || f->no_arena) return VAMD_EINVAL;
  if (nstreams < 1 || nstreams > f->max_streams || frames < 1 || frames > f->max_frames) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  FeedLane &L = f->lanes[(size_t)slot];
  if (L.state != LANE_FILLING) return VAMD_EINVAL;
  L.frames_of.clear();
  return queue_group(f, L, nstreams, frames);
}

int vamd_feed_wrote_v(vamd_feed *f, int slot, long nstreams, const int64_t *frames) {
  if (!f || !frames || slot < 0 || slot >= (int)f->lanes.size() || f->write_frames || f->no_arena) return VAMD_EINVAL;
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
  L.frames_of.assign(frames, frames + nstreams);
  return queue_group(f, L, nstreams, longest);
}

int vamd_feed_wrote_live(vamd_feed *f, int slot, long nstreams, const int64_t *frames, const uint8_t *close) {
  if (!f || !frames || slot < 0 || slot >= (int)f->lanes.size() || !f->write_frames || f->no_arena) return VAMD_EINVAL;
  if (nstreams < 1 || nstreams > f->max_streams) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  FeedLane &L = f->lanes[(size_t)slot];
  if (L.state != LANE_FILLING) return VAMD_EINVAL;
  for (long i = 0; i < nstreams; i++) {
    if (frames[i] < 0 || frames[i] > f->max_frames) return VAMD_EINVAL;
    if (close && close[i] && !frames[i] && !L.live[(size_t)i].open) return VAMD_EINVAL;  // (closing a stream that never had a frame)
  }
  L.frames_of.assign(frames, frames + nstreams);
  L.close_of.assign((size_t)nstreams, 0);
  if (close)
    for (long i = 0; i < nstreams; i++) L.close_of[(size_t)i] = close[i] != 0;
  return queue_group(f, L, nstreams, f->max_frames);
}

int vamd_feed_packets(vamd_feed *f, int slot, vamd_feed_result *out) { return await_group(f, slot, &FeedLane::result, out, false); }

int vamd_feed_decoded(vamd_feed *f, int slot, vamd_feed_decoded_result *out) {
  if (!f || !out || slot < 0 || slot >= (int)f->lanes.size()) return VAMD_EINVAL;
  memset(out, 0, sizeof(*out));
  if (!f->decoded) {
    std::lock_guard<std::mutex> g(f->m);
    f->err = "vamd_feed_decoded: the feed was not created with VAMD_FEED_DECODED";
    return VAMD_EINVAL;
  }
  const int r = await_group(f, slot, &FeedLane::dec_result, out, false);
  if (r) {
    memset(out, 0, sizeof(*out));
    return r;
  }
  FeedLane &L = f->lanes[(size_t)slot];
  if (hipEventSynchronize(L.ev_dec) != hipSuccess) {
    std::lock_guard<std::mutex> g(f->m);
    f->err = "vamd_feed_decoded: the decoded signal's kernels failed";
    memset(out, 0, sizeof(*out));
    return VAMD_EFAULT;
  }
  return VAMD_OK;
}

int vamd_feed_release(vamd_feed *f, int slot) {
  if (!f || slot < 0 || slot >= (int)f->lanes.size()) return VAMD_EINVAL;
  std::lock_guard<std::mutex> g(f->m);
  FeedLane &L = f->lanes[(size_t)slot];
  if (L.state != LANE_DONE && L.state != LANE_FILLING) return VAMD_EINVAL;
  L.user_serials.clear();
  L.user_comments.clear();
  L.comments.clear();
  L.user_flush.clear();
  L.flush.clear();
  L.state = LANE_FREE;
  f->cv_done.notify_all();
  return VAMD_OK;
}

const char *vamd_feed_last_error(const vamd_feed *f) { return f ? f->err.c_str() : feed_create_err.c_str(); }

}  // extern "C"
