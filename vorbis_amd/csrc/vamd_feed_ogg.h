// vamd_feed_ogg.h -- a part of vamd_feed.hip's translation unit: an Ogg feed's host side.  The mirror the copy kernels
// fill, the pager behind a group's last packet and its result (k_ogg.h holds the kernels), a group's serial numbers,
// comment headers and flushes as it is queued, and the check of the three header packets.
#pragma once
#include "vamd_feed_lane.h"
#include "k_feed.h"
#include "k_ogg.h"

// ---- the mirror the copy kernels fill, the pager behind the last packet (k_ogg.h) ----
// The mirror's buffers for a group of nb packets, as large as the packet arena (+ 16: the pager reads whole words), the
// first `keep` bytes kept when it has to grow in mid-group (a managed group's earlier slices); O's mirror pointers set, or
// null on a feed without Ogg headers.
static int feed_mirror(vamd_feed *f, FeedLane &L, FeedOut &O, long nb, size_t keep) {
  FeedLane::Ogg &G = L.ogg;
  O.m_bytes = O.m_info = nullptr, O.m_off = O.m_gp = nullptr, O.m_bits = nullptr;
  if (!f->ogg) return VAMD_OK;
  const size_t want = L.h_out.bytes + 16, n = nz(nb);
  if (G.d_mirror.bytes < want) {
    if (keep && G.d_mirror.p) {
      void *q = nullptr;
      FEED_TRY(L, hipMalloc(&q, want));
      FEED_TRY(L, hipMemcpyAsync(q, G.d_mirror.p, keep < G.d_mirror.bytes ? keep : G.d_mirror.bytes, hipMemcpyDeviceToDevice, L.stream));
      FEED_TRY(L, hipStreamSynchronize(L.stream));
      G.d_mirror.adopt(q, want);
    } else {
      FEED_TRY(L, hipStreamSynchronize(L.stream));  // (nothing in flight reads the old one when it goes)
      FEED_TRY(L, G.d_mirror.need(want));
    }
  }
  FEED_TRY(L, G.d_moff.need(n * 8));
  FEED_TRY(L, G.d_mgp.need(n * 8));
  FEED_TRY(L, G.d_mrbits.need(n * 4));
  FEED_TRY(L, G.d_minfo.need(n));
  O.m_bytes = (uint8_t *)G.d_mirror.p, O.m_info = (uint8_t *)G.d_minfo.p;
  O.m_off = (int64_t *)G.d_moff.p, O.m_gp = (int64_t *)G.d_mgp.p, O.m_bits = (int32_t *)G.d_mrbits.p;
  return VAMD_OK;
}

// The pager, queued behind the group's last copy kernel: k_ogg_plan (a wave per stream) -> k_feed_scan (the files end to
// end) -> k_ogg_pages (a wave per page slot; the pages cross the link inside it).  Nothing here waits: the page table is
// sized by ogg_slots_per_packet, the arena by ogg_file_bound of the PACKET arena's size -- packets that fit theirs make
// files that fit this one.  d_packet_total (VBR): the packets' bytes on the device; beyond the arena nothing was mirrored
// and nothing is paged (finish_group lays the group out again).
// A group with comment headers of its own (L.ogg.comments, vamd_feed_ogg_comments): they go up beside the serial numbers, the
// header slots are those of the group's longest comment and the file arena is sized from their sum (ogg_file_bound_v).
// A live group (f->write_frames): the streams' states and carries go along (OggLiveIO), k_ogg_carry runs behind the pages;
// what it and k_ogg_plan write is the OTHER state and carry, which pager_result makes the current ones -- so a group that
// is laid out twice (finish_group) advances its streams once.
// Its four parts, run_pager last:

// a live lane's streams' states and carries: once per lane, for every stream it may carry
static int pager_live_state(vamd_feed *f, FeedLane &L) {
  FeedLane::OggLiveState &V = L.ogg_live;
  if (V.d_gstart.p) return VAMD_OK;
  const size_t n = (size_t)f->max_streams;
  for (int b = 0; b < 2; b++) {
    FEED_TRY(L, V.d_olive[b].need(n * sizeof(vamd::OggLive)));
    FEED_TRY(L, V.d_crec[b].need(n * 2 * vamd::OGG_MAX_SEGS * 4));
    FEED_TRY(L, V.d_cbytes[b].need(n * vamd::OGG_CARRY_BYTES + 16));
    FEED_TRY(L, hipMemsetAsync(V.d_olive[b].p, 0, V.d_olive[b].bytes, L.stream));
    FEED_TRY(L, hipMemsetAsync(V.d_crec[b].p, 0, V.d_crec[b].bytes, L.stream));
    FEED_TRY(L, hipMemsetAsync(V.d_cbytes[b].p, 0, V.d_cbytes[b].bytes, L.stream));
  }
  FEED_TRY(L, V.d_gstart.need(n * 8));
  return VAMD_OK;
}

// the feed's three header packets on the device, each at a multiple of 4: once per lane
static int pager_headers(vamd_feed *f, FeedLane &L) {
  FeedLane::Ogg &G = L.ogg;
  if (G.d_hdr.p) return VAMD_OK;
  size_t at = 0;
  for (int i = 0; i < 3; i++) G.hdr_off[i] = (int32_t)at, at += al(f->ogg_hdr[i].size(), 4);
  std::vector<uint8_t> img(at + 16, 0);
  for (int i = 0; i < 3; i++) memcpy(img.data() + G.hdr_off[i], f->ogg_hdr[i].data(), f->ogg_hdr[i].size());
  FEED_TRY(L, G.d_hdr.need(img.size()));
  FEED_TRY(L, hipMemcpy(G.d_hdr.p, img.data(), img.size(), hipMemcpyHostToDevice));
  return VAMD_OK;
}

// what the group itself sends up: [serial (ns) | a live group's flags (ns)], and its own comment headers -- the table and
// the bytes in one copy (T: the table's measures; a group without comments of its own sends none and T is left alone)
static int pager_upload(vamd_feed *f, FeedLane &L, long ns, CommentTable &T) {
  FeedLane::Ogg &G = L.ogg;
  hipStream_t st = L.stream;
  const bool live = f->write_frames != 0;
  FEED_TRY(L, G.h_serial.need((size_t)ns * 8));
  FEED_TRY(L, G.d_serial.need((size_t)ns * 8));
  memcpy(G.h_serial.p, G.serials.data(), (size_t)ns * 4);
  if (live) memcpy((uint32_t *)G.h_serial.p + ns, L.ogg_live.flags.data(), (size_t)ns * 4);
  FEED_TRY(L, hipMemcpyAsync(G.d_serial.p, G.h_serial.p, (size_t)ns * (live ? 8 : 4), hipMemcpyHostToDevice, st));
  if (G.comments.empty()) return VAMD_OK;
  T = comment_table(G.comments, ns, (int32_t)f->ogg_hdr[1].size());
  FEED_TRY(L, G.h_cmt.need(T.bytes));
  FEED_TRY(L, G.d_cmt.need(T.bytes));
  comment_table_image(G.comments, ns, T, (uint8_t *)G.h_cmt.p);
  FEED_TRY(L, hipMemcpyAsync(G.d_cmt.p, G.h_cmt.p, T.bytes, hipMemcpyHostToDevice, st));
  return VAMD_OK;
}

// the bytes a group's files take at most, by the kind of group: live or whole streams, comment headers of its own (cmt_sum:
// their sum) or the feed's
static int64_t pager_file_bound(bool live, bool tagged, int64_t packet_bytes, long nb, long ns, const int32_t hb[3], int64_t cmt_sum) {
  if (tagged) return live ? vamd::ogg_live_file_bound_v(packet_bytes, nb, ns, hb, cmt_sum) : vamd::ogg_file_bound_v(packet_bytes, nb, ns, hb, cmt_sum);
  return live ? vamd::ogg_live_file_bound(packet_bytes, nb, ns, hb) : vamd::ogg_file_bound(packet_bytes, nb, ns, hb);
}

static int run_pager(vamd_feed *f, FeedLane &L, const int64_t *d_stream_start, long ns, long nb, const int64_t *d_packet_total) {
  FeedLane::Ogg &G = L.ogg;
  hipStream_t st = L.stream;
  const bool live = f->write_frames != 0;
  if (live) FEED_OWN(pager_live_state(f, L));
  FEED_OWN(pager_headers(f, L));
  if (live) G.serials.resize((size_t)ns, 0);  // (the lane's open streams beyond the caller's begin nothing)
  if ((long)G.serials.size() != ns || !G.d_mirror.p || (live && (long)L.ogg_live.flags.size() != ns)) {
    L.err = "Ogg feed: the group has no serial numbers or no mirror";
    return VAMD_EFAULT;
  }
  const bool tagged = !G.comments.empty();
  int32_t hb[3];
  for (int i = 0; i < 3; i++) hb[i] = (int32_t)f->ogg_hdr[i].size();
  CommentTable T = {0, 0, 0};
  FEED_OWN(pager_upload(f, L, ns, T));
  if (tagged) hb[1] = T.longest;  // (from here on hb sizes the slots; the pager's own copy of the shared lengths is f->ogg_hdr's)
  const int64_t hs = live ? vamd::ogg_live_slots(hb) : vamd::ogg_header_slots(hb);
  const int64_t sp = vamd::ogg_slots_per_packet(f->pkcap[0] > f->pkcap[1] ? f->pkcap[0] : f->pkcap[1]);
  const int64_t nslots = ns * hs + sp * nb;
  const OggRecLayout R(ns);
  FEED_TRY(L, G.d_pages.need((size_t)nslots * sizeof(vamd::OggPage)));
  FEED_TRY(L, G.d_fbytes.need((size_t)ns * 8));
  FEED_TRY(L, G.d_foff.need((size_t)(ns + 1) * 8));
  FEED_TRY(L, G.d_npages.need((size_t)ns * 4));
  FEED_TRY(L, G.d_ostatus.need((size_t)ns));
  FEED_TRY(L, G.h_orec.need(R.bytes));
  const int64_t bound = pager_file_bound(live, tagged, (int64_t)L.h_out.bytes, nb, ns, hb, T.sum);
  FEED_TRY(L, G.h_ogg.need(al((size_t)bound + 16, 4096)));
  vamd::OggIn I;
  I.stream_start = d_stream_start;
  I.off = (const int64_t *)G.d_moff.p, I.gp = (const int64_t *)G.d_mgp.p, I.bits = (const int32_t *)G.d_mrbits.p;
  I.info = (const uint8_t *)G.d_minfo.p, I.bytes = (const uint8_t *)G.d_mirror.p, I.cap = (int64_t)L.h_out.bytes;
  I.packet_total = d_packet_total;
  I.hdr = (const uint8_t *)G.d_hdr.p;
  for (int i = 0; i < 3; i++) I.hdr_off[i] = G.hdr_off[i], I.hdr_bytes[i] = (int32_t)f->ogg_hdr[i].size();
  I.serial = (const uint32_t *)G.d_serial.p;
  I.header_slots = hs, I.slots_per_packet = sp;
  I.cmt = tagged ? (const uint8_t *)G.d_cmt.p : nullptr;
  vamd::OggOut O;
  uint8_t *dr = nullptr;
  FEED_TRY(L, G.h_orec.mapped(&dr));
  FEED_TRY(L, G.h_ogg.mapped(&O.bytes));
  O.total = (int64_t *)dr, O.cap = (int64_t)G.h_ogg.bytes;
  R.point(dr, O);
  vamd::OggLiveIO V;
  memset(&V, 0, sizeof(V));
  if (live) {
    const FeedLane::OggLiveState &S = L.ogg_live;
    const int a = S.cur, b = 1 - a;
    V.in = (const vamd::OggLive *)S.d_olive[a].p, V.out = (vamd::OggLive *)S.d_olive[b].p;
    V.rec_in = (const int32_t *)S.d_crec[a].p, V.rec_out = (int32_t *)S.d_crec[b].p;
    V.bytes_in = (const uint8_t *)S.d_cbytes[a].p, V.bytes_out = (uint8_t *)S.d_cbytes[b].p;
    V.flags = (const uint32_t *)G.d_serial.p + ns, V.gstart = (int64_t *)S.d_gstart.p;
  }
  hipLaunchKernelGGL(vamd::k_ogg_plan, dim3((unsigned)ns), dim3(64), 0, st, I, ns, (vamd::OggPage *)G.d_pages.p, (int64_t *)G.d_fbytes.p,
                     (int32_t *)G.d_npages.p, (uint8_t *)G.d_ostatus.p, V);
  hipLaunchKernelGGL(k_feed_scan, dim3(1), dim3(1024), 0, st, ns, (const int64_t *)G.d_fbytes.p, (int64_t *)G.d_foff.p);
  hipLaunchKernelGGL(vamd::k_ogg_pages, dim3((unsigned)nslots), dim3(64), 0, st, I, ns, (const vamd::OggPage *)G.d_pages.p,
                     (const int64_t *)G.d_foff.p, (const int32_t *)G.d_npages.p, (const uint8_t *)G.d_ostatus.p, O, V);
  if (live) hipLaunchKernelGGL(vamd::k_ogg_carry, dim3((unsigned)ns), dim3(64), 0, st, I, ns, V);
  FEED_TRY(L, hipGetLastError());
  return VAMD_OK;
}

// ... and after the group's wait: what vamd_feed_ogg hands out (of a live group's ns streams the caller's first ns_out;
// the others completed no page), and the live streams' states advance
static int pager_result(vamd_feed *f, FeedLane &L, long ns, long ns_out) {
  uint8_t *hr = (uint8_t *)L.ogg.h_orec.p;
  vamd_feed_ogg_result &R = L.ogg.result;
  R.nstreams = ns_out;
  OggRecLayout(ns).point(hr, R);
  R.bytes = (const uint8_t *)L.ogg.h_ogg.p, R.total_bytes = *(const int64_t *)hr;
  for (long s = 0; s < ns; s++)
    if (R.status[s] & 0x80) {
      L.err = f->write_frames ? "Ogg feed: a stream needed more pages than its slots of the page table, or its live state does not hold"
                              : "Ogg feed: a stream needed more pages than its slots of the page table";
      return VAMD_EFAULT;
    }
  if (R.total_bytes + 4 > (int64_t)L.ogg.h_ogg.bytes) {
    L.err = "Ogg feed: the files exceed the bound their arena was sized by";
    return VAMD_EFAULT;
  }
  if (f->write_frames) {
    if (R.stream_offset[ns_out] != R.total_bytes) {
      L.err = "Ogg feed: a stream outside the group completed a page";
      return VAMD_EFAULT;
    }
    L.ogg_live.cur = 1 - L.ogg_live.cur;
  }
  return VAMD_OK;
}

// ---- a group as it is queued, and the feed's header packets ----
// an Ogg feed's group (f->m held): its serial numbers -- the next nstreams of the feed's running counter, then what
// vamd_feed_ogg_serials set for the slot in their place
// A live group: a serial number belongs to a stream, not to a group -- only a stream that begins with this group (its
// slot is free and the piece has frames) takes one, the counter's next or the one named for it; an open stream keeps its own.
static void ogg_job(vamd_feed *f, FeedLane &L, long nstreams) {
  FeedLane::Ogg &G = L.ogg;
  memset(&G.result, 0, sizeof(G.result));
  if (!f->ogg) return;
  G.serials.assign((size_t)nstreams, 0);
  for (long s = 0; s < nstreams; s++)
    if (!f->write_frames) G.serials[(size_t)s] = f->next_serial++;
    else if (!L.live.streams[(size_t)s].open && L.frames_of[(size_t)s])
      G.serials[(size_t)s] = (size_t)s < G.user_serials.size() ? G.user_serials[(size_t)s] : f->next_serial++;
  if (!f->write_frames)
    for (size_t s = 0; s < G.user_serials.size() && s < (size_t)nstreams; s++) G.serials[s] = G.user_serials[s];
  G.user_serials.clear();
  // ... and its comment headers: what vamd_feed_ogg_comments set for the slot, of a live group only those of the streams
  // that begin with it; none left: a group like any other
  G.comments.swap(G.user_comments);
  G.user_comments.clear();
  if (G.comments.size() > (size_t)nstreams) G.comments.resize((size_t)nstreams);
  bool any = false;
  for (size_t s = 0; s < G.comments.size(); s++) {
    if (f->write_frames && (L.live.streams[s].open || !L.frames_of[s])) G.comments[s].clear();
    any |= !G.comments[s].empty();
  }
  if (!any) G.comments.clear();
  // ... and the streams it flushes (vamd_feed_ogg_flush), of the caller's streams only
  FeedLane::OggLiveState &V = L.ogg_live;
  V.flush.swap(V.user_flush);
  V.user_flush.clear();
  if (V.flush.size() > (size_t)nstreams) V.flush.resize((size_t)nstreams);
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
