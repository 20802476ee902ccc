// vamd_feed_group.h -- a part of vamd_feed.hip's translation unit: a group from its plan on, whole or live.  The group's
// record and where the copy kernels write, a size class's batch, the run the hand-over kernels take, a bitrate-managed
// group in slices, the decoded signal behind the packets, and finish_group, which every ingest path ends in.
#pragma once
#include "vamd_feed_ogg.h"

// ---- what the two group paths share: the group's record, a size class's batch, the run the hand-over kernels take ----
// where a copy kernel writes: the record (RecLayout, vamd_feed_host.h) and the packet arena as the device sees them, and
// the Ogg mirror (feed_mirror; the first `keep` bytes of the mirror are a managed group's earlier slices)
static int feed_out(vamd_feed *f, FeedLane &L, const RecLayout &R, long nb, size_t keep, FeedOut &O) {
  uint8_t *dr = nullptr;
  FEED_TRY(L, L.h_rec.mapped(&dr));
  FEED_TRY(L, L.h_out.mapped(&O.bytes));
  O.total = (int64_t *)dr, O.cap = (int64_t)L.h_out.bytes;
  R.point(dr, O);
  return feed_mirror(f, L, O, nb, keep);
}

// ... and behind the group's wait: what vamd_feed_packets hands out, and the two timings
static void feed_result(FeedLane &L, const RecLayout &R, long ns_out, long nb, int64_t total) {
  vamd_feed_result &out = L.result;
  out.nstreams = ns_out, out.nblocks = nb;
  R.point((uint8_t *)L.h_rec.p, out);
  out.bytes = (const uint8_t *)L.h_out.p, out.total_bytes = total;
  float up = 0.f, dev = 0.f;
  (void)hipEventElapsedTime(&up, L.ev0, L.ev_up);
  (void)hipEventElapsedTime(&dev, L.ev0, L.ev_end);
  out.upload_ms = L.src.dev ? 0. : up, out.device_ms = dev;  // (a device-fed group: nothing went up, ev0 stands before the ingest)
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

// the sizes of run P's packets over its ns streams, in front of either copy kernel: the stream of each packet (d_sid), each
// packet's place in its stream (d_rel), the streams' bytes (d_sbytes) and the streams end to end (d_soff; [ns]: their sum)
static void launch_sizes(const FeedLane &L, const FeedSlice &P, long ns) {
  hipStream_t st = L.stream;
  hipLaunchKernelGGL(k_feed_sid, dim3((unsigned)ns), dim3(64), 0, st, P.stream_start, (int32_t *)L.d_sid.p);
  hipLaunchKernelGGL(k_feed_sizes, dim3((unsigned)ns), dim3(64), 0, st, P, (int64_t *)L.d_rel.p, (int64_t *)L.d_sbytes.p);
  hipLaunchKernelGGL(k_feed_scan, dim3(1), dim3(1024), 0, st, ns, (const int64_t *)L.d_sbytes.p, (int64_t *)L.d_soff.p);
}

// ---- a bitrate-managed group ----
// A bitrate-managed group, from its plan on: the blocks in slices of at most f->slice (plan_slices, vamd_feed_host.h), each
// slice through
//   vamd_analyze_streams_mixed_managed (fifteen candidate packets per block; the ampmax chains resume per stream) ->
//   vamd_bitrate_walk (the managers resume per stream) -> the handed-out packets laid end to end behind the previous
//   slice's, straight into the pinned arena
// The workspace is bounded by the slice, not the group: a long stereo block's candidates alone take 15 x its integer
// residue (120 KB) and 15 packet rows.  The host waits once per slice for the slice's byte count (to grow the arena
// before anything is written into it: the candidates do not outlive their slice).
// (live: `live` set, ns streams planned of which the caller's first ns_out are reported; the managers carried across groups)
static int run_group_managed(vamd_feed *f, FeedLane &L, const vamd_stream_plan &plan, const float *pcm, long ns, long ss, long cs,
                             const long long *d_frames_of, FeedLive live, long ns_out) {
  FeedLane::Managed &M = L.managed;
  const int ch = f->ch;
  const long nb = (long)(plan.nblocks[0] + plan.nblocks[1]);
  hipStream_t st = L.stream;
  std::vector<int32_t> order(nz(nb));
  std::vector<int64_t> start((size_t)ns + 1), starts;
  FEED_CALL(L, vamd_plan_fetch(L.ctx, &plan, nullptr, nullptr, nullptr, nullptr, order.data(), start.data()));
  const char *why = nullptr;
  const std::vector<Slice> sl = plan_slices(order, start, ns, nb, f->slice, starts, &why);
  if (why) {
    L.err = why;
    return VAMD_EFAULT;
  }
  // all slices' lists in one upload: [the slice's byte count on its way back (16) | order[] rebased | the stream_starts]
  const size_t order_bytes = al(nz(nb) * 4, 8), lists = order_bytes + starts.size() * 8;
  FEED_TRY(L, M.h_slice.need(lists + 16));
  FEED_TRY(L, M.d_slice.need(lists + 16));
  int64_t *h_total = (int64_t *)M.h_slice.p;
  uint8_t *hl = (uint8_t *)M.h_slice.p + 16, *dl = (uint8_t *)M.d_slice.p + 16;
  memcpy(hl, order.data(), (size_t)nb * 4);
  memcpy(hl + order_bytes, starts.data(), starts.size() * 8);
  FEED_TRY(L, hipMemcpyAsync(dl, hl, lists, hipMemcpyHostToDevice, st));
  const int32_t *d_order = (const int32_t *)dl;
  const int64_t *d_starts = (const int64_t *)(dl + order_bytes);
  // the slice's buffers, sized for the largest slice of each class
  const int K = VAMD_PACKETBLOBS;
  for (int W = 0; W < 2; W++) {
    int64_t most = 1;
    for (const Slice &x : sl) most = x.n[W] > most ? x.n[W] : most;
    const size_t m = (size_t)most, n2 = (size_t)f->bs[W] / 2;
    FEED_TRY(L, M.d_mpk[W].need(m * K * (size_t)f->pkcap[W]));
    FEED_TRY(L, M.d_mbits[W].need(m * K * 4));
    FEED_TRY(L, M.d_mposts[W].need(m * K * ch * VAMD_POSTS_STRIDE * 4));
    FEED_TRY(L, M.d_mvalid[W].need(m * K * ch * 4));
    FEED_TRY(L, M.d_miwork[W].need(m * K * ch * n2 * 4));
    FEED_TRY(L, M.d_mnz[W].need(m * K * ch * 4));
    FEED_TRY(L, L.d_status[W].need(m * (size_t)ch));
    FEED_TRY(L, M.d_choice[W].need(m * 4));
    FEED_TRY(L, M.d_fbits[W].need(m * 4));
  }
  const size_t most_slice = f->slice < nb ? (size_t)f->slice : nz(nb);
  FEED_TRY(L, L.d_rel.need(most_slice * 8));
  FEED_TRY(L, L.d_sid.need(most_slice * 4));
  FEED_TRY(L, L.d_sbytes.need((size_t)ns * 8));
  FEED_TRY(L, L.d_soff.need((size_t)(ns + 1) * 8));
  if (!live.in) {  // (a live lane's managers live across groups: k_live_begin starts the fresh ones)
    FEED_TRY(L, M.d_bstate.need((size_t)ns * sizeof(vamd_bitrate_state)));
    FEED_CALL(L, vamd_bitrate_init_states(L.ctx, (vamd_bitrate_state *)M.d_bstate.p, ns));
  }
  const RecLayout R(ns, nb);
  FEED_TRY(L, L.h_rec.need(R.bytes + R.bytes / 4));
  FeedSlice P = feed_slice_of(f, L, plan, ss, d_frames_of, live);
  for (int W = 0; W < 2; W++) {
    P.choice[W] = (const int32_t *)M.d_choice[W].p, P.fbits[W] = (const int32_t *)M.d_fbits[W].p, P.mbits[W] = (const int32_t *)M.d_mbits[W].p;
    P.packets[W] = (const uint8_t *)M.d_mpk[W].p;
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
      m[W].posts = (int32_t *)M.d_mposts[W].p;
      m[W].post_valid = (int32_t *)M.d_mvalid[W].p;
      m[W].iwork = (int32_t *)M.d_miwork[W].p;
      m[W].nonzero = (int32_t *)M.d_mnz[W].p;
      m[W].packets = (uint8_t *)M.d_mpk[W].p;
      m[W].packet_bits = (int32_t *)M.d_mbits[W].p;
      m[W].packet_stride = f->pkcap[W];
    }
    FEED_CALL(L, vamd_analyze_streams_mixed_managed(L.ctx, &desc[0], &io[0], &m[0], &desc[1], &io[1], &m[1], P.order, P.stream_start, nss, nbs,
                                                    (float *)L.d_amp.p + x.s0));
    // walk: the managers' choice and the size they hand out
    int32_t *choice[2] = {(int32_t *)M.d_choice[0].p, (int32_t *)M.d_choice[1].p};
    int32_t *fbits[2] = {(int32_t *)M.d_fbits[0].p, (int32_t *)M.d_fbits[1].p};
    FEED_CALL(L, vamd_bitrate_walk(L.ctx, P.order, P.stream_start, nss, P.mbits, P.status, (vamd_bitrate_state *)M.d_bstate.p + x.s0, choice, fbits));
    // sizes, and the wait for their sum
    launch_sizes(L, P, nss);
    FEED_TRY(L, hipGetLastError());
    FEED_TRY(L, hipMemcpyAsync(h_total, (const int64_t *)L.d_soff.p + nss, 8, hipMemcpyDeviceToHost, st));
    FEED_TRY(L, hipStreamSynchronize(st));
    // grow the arena (and the mirror) where the slice needs it, the earlier slices' packets kept; copy
    const int64_t need = base + *h_total;
    if (need > (int64_t)L.h_out.bytes) FEED_TRY(L, L.h_out.grow_keeping((size_t)need + (size_t)need / 8, (size_t)base));
    FeedOut O;
    FEED_OWN(feed_out(f, L, R, nb, (size_t)base, O));
    hipLaunchKernelGGL(k_feed_copy_managed, dim3((unsigned)((nbs + 3) / 4)), dim3(256), 0, st, P, nbs, base, (const int64_t *)L.d_rel.p,
                       (const int64_t *)L.d_soff.p, (const int32_t *)L.d_sid.p, O);
    FEED_TRY(L, hipGetLastError());
    base = need;
  }
  if (f->ogg && sl.empty()) {  // (a live group without a block: no slice has made the mirror the pager is given)
    FeedOut O;
    FEED_OWN(feed_out(f, L, R, nb, 0, O));
  }
  if (f->ogg) FEED_OWN(run_pager(f, L, plan.stream_start, ns, nb, nullptr));
  FEED_TRY(L, hipEventRecord(L.ev_end, st));
  FEED_TRY(L, hipEventSynchronize(L.ev_end));
  if (f->ogg) FEED_OWN(pager_result(f, L, ns, ns_out));
  uint8_t *hrec = (uint8_t *)L.h_rec.p;  // (the total and stream_start, which a VBR group's copy kernel writes, from here)
  *(int64_t *)hrec = base;
  memcpy(hrec + R.start, start.data(), (size_t)(ns + 1) * 8);
  feed_result(L, R, ns_out, nb, base);
  return VAMD_OK;
}

// ---- the decoded signal ----
// A decoded feed's group, behind its packets' hand-over: the streams' geometry up, k_synth per size class and the lap
// (vamd_synth_streams: out of what the analysis left in the lane's context), the event behind them.  Stream s takes
// ch * frames[s] floats of the arena whether or not it gets a signal.
static int enqueue_decoded(vamd_feed *f, FeedLane &L, const vamd_stream_plan &plan, long ns) {
  FeedLane::Decoded &D = L.dec;
  D.frames.resize((size_t)ns), D.offset.resize((size_t)ns + 1);
  FEED_TRY(L, D.h_dgeo.need((size_t)ns * 16));
  FEED_TRY(L, D.d_dgeo.need((size_t)ns * 16));
  int64_t *h = (int64_t *)D.h_dgeo.p, at = 0;
  for (long s = 0; s < ns; s++) {
    const int64_t fr = L.frames_of.empty() ? L.frames : L.frames_of[(size_t)s];
    h[s] = D.frames[(size_t)s] = fr;
    h[ns + s] = D.offset[(size_t)s] = at;
    at += fr * f->ch;
  }
  D.offset[(size_t)ns] = at;
  for (int W = 0; W < 2; W++) FEED_TRY(L, D.d_synth[W].need(((size_t)plan.nblocks[W] * f->ch * (size_t)f->bs[W] + 4) * 4));
  FEED_TRY(L, D.d_dec.need(((size_t)at + 4) * 4));
  FEED_TRY(L, hipMemcpyAsync(D.d_dgeo.p, h, (size_t)ns * 16, hipMemcpyHostToDevice, L.stream));
  FEED_CALL(L, vamd_synth_streams(L.ctx, &plan, ns, L.frames, (const int64_t *)D.d_dgeo.p, (const int64_t *)D.d_dgeo.p + ns,
                                  plan.nblocks[0] ? (float *)D.d_synth[0].p : nullptr, plan.nblocks[1] ? (float *)D.d_synth[1].p : nullptr,
                                  (float *)D.d_dec.p));
  FEED_TRY(L, hipEventRecord(D.ev, L.stream));
  return VAMD_OK;
}

// ... and what vamd_feed_decoded hands out, once the group's record is home: a stream that lost a packet has no signal
static void decoded_result(vamd_feed *f, FeedLane &L, long ns) {
  FeedLane::Decoded &D = L.dec;
  D.status.assign((size_t)ns, 0);
  const vamd_feed_result &r = L.result;
  for (long s = 0; s < ns; s++) {
    for (int64_t k = r.stream_start[s]; k < r.stream_start[s + 1]; k++)
      if (r.bits[k] < 0) {  // no packet, no signal -- whatever the block's status bits say
        D.status[(size_t)s] = (uint8_t)((r.info[k] >> 2) & 3);
        D.frames[(size_t)s] = 0;
        break;
      }
  }
  vamd_feed_decoded_result &o = D.result;
  o.nstreams = ns, o.channels = f->ch;
  o.frames = D.frames.data(), o.offset = D.offset.data(), o.status = D.status.data();
  o.pcm = (const float *)D.d_dec.p, o.total_floats = D.offset[(size_t)ns];
}

// ---- a group from its plan on (whole or live): the analysis, the packets end to end into the pinned arena ----
static int finish_group(vamd_feed *f, FeedLane &L, const vamd_stream_plan &plan, const float *pcm, long ns, long ss, long cs,
                        const long long *d_frames_of, FeedLive live, long ns_out) {
  hipStream_t st = L.stream;
  if (f->managed) return run_group_managed(f, L, plan, pcm, ns, ss, cs, d_frames_of, live, ns_out);
  const long nb = (long)(plan.nblocks[0] + plan.nblocks[1]);
  vamd_batch_desc desc[2];
  vamd_batch_io io[2];
  for (int W = 0; W < 2; W++) {
    const size_t n = nz((long)plan.nblocks[W]);
    FEED_TRY(L, L.d_pk[W].need(n * (size_t)f->pkcap[W]));
    FEED_TRY(L, L.d_bits[W].need(n * 4));
    FEED_TRY(L, L.d_status[W].need(n * (size_t)f->ch));
    batch_of(plan, W, 0, plan.nblocks[W], pcm, cs, L.d_status[W], desc[W], io[W]);
    if (!plan.nblocks[W]) continue;
    io[W].packets = (uint8_t *)L.d_pk[W].p;
    io[W].packet_bits = (int32_t *)L.d_bits[W].p;
    io[W].packet_stride = f->pkcap[W];
  }
  if (nb)
    FEED_CALL(L, vamd_analyze_streams_mixed(L.ctx, &desc[0], &io[0], &desc[1], &io[1], plan.order, plan.stream_start, ns, nb,
                                            (float *)L.d_amp.p));
  // the packets end to end, into the pinned arena
  FEED_TRY(L, L.d_rel.need(nz(nb) * 8));
  FEED_TRY(L, L.d_sid.need(nz(nb) * 4));
  FEED_TRY(L, L.d_sbytes.need((size_t)ns * 8));
  FEED_TRY(L, L.d_soff.need((size_t)(ns + 1) * 8));
  const RecLayout R(ns, nb);
  FEED_TRY(L, L.h_rec.need(R.bytes + R.bytes / 4));
  FeedSlice P = feed_slice_of(f, L, plan, ss, d_frames_of, live);  // (the whole group as one run: k_feed.h)
  P.order = plan.order, P.stream_start = plan.stream_start;
  for (int W = 0; W < 2; W++) P.fbits[W] = (const int32_t *)L.d_bits[W].p, P.packets[W] = (const uint8_t *)L.d_pk[W].p;
  for (int attempt = 0;; attempt++) {
    FeedOut O;
    FEED_OWN(feed_out(f, L, R, nb, 0, O));
    launch_sizes(L, P, ns);
    const long waves = (nb > ns + 1 ? nb : ns + 1);
    hipLaunchKernelGGL(k_feed_copy, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, P, ns, nb, (const int64_t *)L.d_rel.p,
                       (const int64_t *)L.d_soff.p, (const int32_t *)L.d_sid.p, O);
    FEED_TRY(L, hipGetLastError());
    if (f->ogg) FEED_OWN(run_pager(f, L, plan.stream_start, ns, nb, (const int64_t *)L.d_soff.p + ns));
    FEED_TRY(L, hipEventRecord(L.ev_end, st));
    // (the decoded signal is enqueued behind the hand-over's event and ahead of the wait for it: the packets are ready no
    // later than without it, and the lane's stream goes on while the host looks at them)
    if (f->decoded && !attempt) FEED_OWN(enqueue_decoded(f, L, plan, ns));
    FEED_TRY(L, hipEventSynchronize(L.ev_end));
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
    FEED_TRY(L, L.h_out.need((size_t)total + (size_t)total / 8));  // the packets are still in HBM: lay them out again
  }
}
