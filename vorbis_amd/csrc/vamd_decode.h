// vamd_decode.h -- the packet decoder's host side (include/vorbis_amd.h: vamd_decode_plan, vamd_decode_streams): audio
// packets in host memory to PCM in device memory.  Part of the library's single translation unit, after vamd_batch.h
// (launch_synth, synth_covered).  The plan is made on the host before anything is enqueued (vamd_decode_plan.h); then, on
// the context's stream: the packets and the plan go up, one copy each; k_unpack turns every packet into its block's rows
// (k_unpack.h); k_synth runs per size class on those rows (k_synth.h, the launch the encoder's tensors take); k_lap
// gathers the streams' samples; the statuses come back.
// The Ogg entry (vamd_decode_ogg_plan, vamd_decode_ogg) takes whole files instead: the host walks their page headers and
// lacing tables (vamd_demux.h), the files go up in one copy as they lie, and k_ogg_depage (k_demux.h) checks every page's
// checksum and moves the audio bytes into the same packed arena -- from k_unpack on the two entries are one function.
// The live decoder (vamd_decode_live.h) takes the next pieces of continuing streams through the same function, with the
// blocks carried between pieces standing in the plan and two carry kernels between k_synth and k_lap (DecodeCarry).
// The live Ogg decoder (vamd_decode_ogg_live.h) takes the next BYTES of continuing Ogg streams: both of the above at once,
// with the packet that whole pages leave open carried on the device by two more kernels around k_ogg_depage.
// The window entries (vamd_decode_window.h) take WINDOWS of streams or of indexed files through the same function too: the
// plan's "streams" are the windows, only their packets or pages go up, and k_lap_window stands in k_lap's place.
// The marked entries (vamd_decode_plan_marked, vamd_decode_streams_marked) and, under vamd_decode_follow, the Ogg entry take
// the plan from per-packet marks instead (decode_plan_build_marked: the reader's granule walk, links from a fresh lap): the
// same function again, with the plan's runs of kept frames as rows for k_lap_segments in k_lap's place.
//
// Workspace per block, in the context, grown on demand and released with it (ch channels, n the block's size, S submaps):
//   rows     4 ch (post_valid) + ch n/2 (the integer curves) + S * 2048 (res_class) + 2 * vamd_residue_capacity
//            (res_entries) + 8 S (res_count)
//   k_synth  4 ch n (vb->pcm)
//   plan     4 (order) + 8 (src) + 16 (the packet's bits) + 1 (status), and the packet itself
//   files    (the Ogg entry) the files' bytes once more, and per page 32 (its row) + 1 (status)
// -- for a stereo block of 2048 some 29 KiB, of which vb->pcm is 16.
#pragma once
#include "vamd_decode_plan.h"
#include "vamd_decode_live_plan.h"
#include "vamd_demux.h"
#include "vamd_demux_live.h"

static_assert(OGG_DEPAGE_BADCRC == VAMD_STATUS_BADPAGE, "k_ogg_depage's status byte is the stream's");

static int dev_need(vamd_ctx *c, DevBuf &b, size_t bytes) {
  if (b.bytes < bytes) {
    if (b.p) HIP_TRY(c, hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    const size_t want = bytes + bytes / 4;
    HIP_TRY(c, hipMalloc(&b.p, want));
    b.bytes = want;
  }
  return VAMD_OK;
}

static void decode_release(vamd_ctx *c) {
  vamd_ctx::Decode &D = c->dec;
  DevBuf *all[] = {&D.bytes, &D.plan, &D.status, &D.files, &D.post_valid[0], &D.post_valid[1], &D.ilogmask[0], &D.ilogmask[1], &D.res_class[0], &D.res_class[1],
                   &D.res_entries[0], &D.res_entries[1], &D.res_count[0], &D.res_count[1], &D.synth[0], &D.synth[1]};
  for (DevBuf *b : all)
    if (b->p) (void)hipFree(b->p);
  if (D.h_plan.p) (void)hipHostFree(D.h_plan.p);
  if (D.h_stage.p) (void)hipHostFree(D.h_stage.p);
  if (D.d_tab) (void)hipFree(D.d_tab);
}

// what the decoder refuses: the setups vamd_synth_check refuses, with its text; a setup k_unpack's walk is not safe on.
// At first use it also builds the codebooks' decode tables, from the image as the device holds it.
static int decode_ready(vamd_ctx *c) {
  vamd_ctx::Decode &D = c->dec;
  if (!D.ready) {
    std::vector<unsigned char> image(c->image_bytes), tab;
    HIP_TRY(c, hipMemcpy(image.data(), c->d_image, image.size(), hipMemcpyDeviceToHost));
    std::string err;
    if (!unpack_check_setup(image, &err)) return fail(c, VAMD_EIMPL, err.c_str());
    UnpackP U;
    unpack_build_tables(image, &tab, &U);
    HIP_TRY(c, hipMalloc((void **)&D.d_tab, tab.size()));
    HIP_TRY(c, hipMemcpy(D.d_tab, tab.data(), tab.size(), hipMemcpyHostToDevice));
    U.tab = D.d_tab;
    D.U = U;
    D.lanes = c->K.unpack_lanes;  // (a test knob, vamd_knobs.h: 64 unless set)
    D.ready = true;
  }
  for (int W = 0; W < D.U.modes; W++) {
    SynthFloorP S;
    int r = synth_covered(c, W, &S);
    if (r) return r;
  }
  return VAMD_OK;
}

// a context made from a stream's headers holds every file's third packet to its own setup header packet where the call
// names none (vamd_create_decoder); a blob context has none to hold it to
static void demux_own_setup(const vamd_ctx *c, DemuxSetup *S) {
  if (!S->setup_header && !S->setup_header_bytes && !c->setup_packet.empty())
    S->setup_header = c->setup_packet.data(), S->setup_header_bytes = (int64_t)c->setup_packet.size();
}

static int decode_plan(vamd_ctx *c, const vamd_decode_desc *d, DecodePlan *P) {
  if (!d) return fail(c, VAMD_EINVAL, "decode: null descriptor");
  int r = decode_ready(c);
  if (r) return r;
  std::string err;
  if (!decode_plan_build(c->B.bs, c->dec.U.modes, c->dec.U.modebits, d->nstreams, d->npackets, d->bytes, d->offset, d->stream_start, d->end_granule, P,
                         &err))
    return fail(c, VAMD_EINVAL, err.c_str());
  return VAMD_OK;
}

int vamd_decode_plan(vamd_ctx *c, const vamd_decode_desc *d, int64_t *frames, int64_t *nblocks) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  DecodePlan P;
  int r = decode_plan(c, d, &P);
  if (r) return r;
  for (int64_t s = 0; frames && s < d->nstreams; s++) frames[s] = P.frames[(size_t)s];
  if (nblocks) nblocks[0] = P.nblocks[0], nblocks[1] = P.nblocks[1];
  return VAMD_OK;
}

// What the two entries hand the shared tail: the packed arena's packet table, and where its bytes come from -- the
// caller's host memory as they are (the packet entry), or the files' pages by way of k_ogg_depage (the Ogg entry).
struct DecodeInput {
  const int64_t *offset = nullptr;   // [npackets + 1] bytes; the arena is [byte0, byte0 + nbytes) of this numbering
  const int64_t *begin = nullptr;    // or [npackets]: where each packet begins, where they do not lie back to back (offset[]
                                     // then gives the lengths alone: a live Ogg call's arena, vamd_demux_live.h)
  int64_t byte0 = 0, nbytes = 0;
  const uint8_t *packets = nullptr;  // the packet entry: the arena in host memory, from byte0 on
  const DemuxScan *scan = nullptr;   // the Ogg entry: the page table, the pages' streams ...
  const uint8_t *files = nullptr;    // ... and the group's files in host memory, one copy as they lie
  int64_t files_bytes = 0;
};

// What a live decoder's call adds (vamd_decode_live.h): the plan's lists of the blocks that have a packet, the carry
// kernels' tables, and the slots' carries on the device.
struct DecodeCarry {
  const DecodeLivePlan *plan = nullptr;
  float *carry = nullptr;
  // the live Ogg decoder's byte carry (vamd_decode_ogg_live.h): k_ogg_packet_carry_in ahead of k_ogg_depage, _out behind it
  const std::vector<OggCarryRow> *bytes_in = nullptr, *bytes_out = nullptr;
  uint8_t *bytes_carry = nullptr;  // [slots][stride]
  int64_t slots = 0, stride = 0;
};

// What a window call adds (vamd_decode_window.h): P's "streams" are windows, and k_lap_window takes k_lap's place with
// each window's first frame in its stream and its channel stride in pcm.
struct DecodeWindows {
  const int64_t *first = nullptr, *stride = nullptr;  // [ns]
};

// The last launch under a format other than F32 planar (vamd_decode_output): the _as form of the gather decode_run would
// have taken, its grid's x sized by the format's elements per thread (k_synth.h, PcmOut) where the F32 gathers take four
// frames per thread.
struct LapLaunch {
  hipStream_t s;
  int64_t ns;
  size_t nseg;
  int64_t max_frames;
  const long long *first, *frames, *stride, *offset;
  const LapSegment *seg;
  int kind;  // 0 k_lap, 1 k_lap_window, 2 k_lap_segments
  void *pcm;
};
extern "C++" {
template <int D, bool IL>
static void launch_lap_as(const LapP &L, const LapLaunch &A) {
  typedef typename PcmElem<D>::T T;
  const long long threads = (IL ? A.max_frames * L.ch : A.max_frames) / PcmOut<D, IL>::per_thread + 2, per = (threads + 255) / 256;
  const unsigned gx = (unsigned)(per < 1024 ? per : 1024);
  if (A.kind == 2)
    hipLaunchKernelGGL((k_lap_segments_as<D, IL>), dim3(gx, (unsigned)(A.nseg < 1024 ? A.nseg : 1024)), dim3(256), 0, A.s, L, (long)A.nseg, A.seg, (T *)A.pcm);
  else if (A.kind == 1)
    hipLaunchKernelGGL((k_lap_window_as<D, IL>), dim3(gx, (unsigned)(A.ns < 1024 ? A.ns : 1024)), dim3(256), 0, A.s, L, (long)A.ns, A.first, A.frames, A.stride,
                       A.offset, (T *)A.pcm);
  else
    hipLaunchKernelGGL((k_lap_as<D, IL>), dim3(gx, (unsigned)(A.ns < 1024 ? A.ns : 1024)), dim3(256), 0, A.s, L, (long)A.ns, A.frames, A.offset, (T *)A.pcm);
}
}  // extern "C++"

static size_t pcm_elem_bytes(int dtype) { return dtype == VAMD_PCM_F32 ? 4 : 2; }

// The tail all entries share, behind a plan that holds and statuses the host has already set: workspace, the plan's
// upload, the arena (uploaded, or unpaged on the device), k_unpack, k_synth, k_lap, and the statuses back in one copy --
// the blocks' and, behind them, the pages' -- folded into their streams.  With `live`, P is live->plan->P: order[] holds
// carried blocks that have no packet, k_unpack takes the plan's own list, and the carries move between k_synth and k_lap;
// without, nothing is enqueued or uploaded that was not before.  With `win`, the two lists go up behind the plan and the
// lap is k_lap_window's; without, likewise nothing changes.  With `seg` (a plan made from marks: decode_plan_build_marked)
// the rows of kept frames go up behind those and the lap is k_lap_segments'; without, likewise.
static int decode_run(vamd_ctx *c, const DecodePlan &P, int64_t ns, const DecodeInput &in, const int64_t *offset_out, float *pcm, uint8_t *status,
                      const DecodeCarry *live = nullptr, const DecodeWindows *win = nullptr, const std::vector<DecodePlan::Segment> *seg = nullptr) {
  int r;
  const std::vector<int32_t> &unpack = live ? live->plan->unpack : P.order;
  const std::vector<int64_t> &unpack_start = live ? live->plan->unpack_start : P.lap_start;
  const size_t nb = unpack.size(), nlap = P.order.size(), npg = in.scan ? in.scan->pages.size() : 0;
  const size_t nin = live ? live->plan->in.size() : 0, nout = live ? live->plan->out.size() : 0;
  const size_t nbin = live && live->bytes_in ? live->bytes_in->size() : 0, nbout = live && live->bytes_out ? live->bytes_out->size() : 0;
  const size_t nseg = seg ? seg->size() : 0;
  if (!nb && !npg) return VAMD_OK;
  vamd_ctx::Decode &D = c->dec;
  const int ch = c->B.channels;
  // the workspace
  const int64_t byte0 = in.byte0, nbytes = in.nbytes;
  const long long nwords = (long long)((nbytes + 3) / 4);
  if ((r = dev_need(c, D.bytes, (size_t)nwords * 4 + 16))) return r;
  if ((r = dev_need(c, D.status, nb + npg + 16))) return r;
  if (npg && (r = dev_need(c, D.files, (((size_t)in.files_bytes + 3) & ~(size_t)3) + 16))) return r;
  UnpackRows rows[2];
  vamd_ctx::SynthSrc src[2];
  for (int W = 0; W < 2; W++) {
    const size_t n = (size_t)P.nblocks[W], n2 = (size_t)c->B.bs[W] / 2, S = (size_t)c->B.chmap[W].submaps;
    if ((r = dev_need(c, D.post_valid[W], n * ch * 4 + 16))) return r;
    if ((r = dev_need(c, D.ilogmask[W], n * ch * n2 + 16))) return r;
    if ((r = dev_need(c, D.res_class[W], n * S * VAMD_RES_CLASS_STRIDE * 4 + 16))) return r;
    if ((r = dev_need(c, D.res_entries[W], n * (size_t)c->B.res_cap[W] * 2 + 16))) return r;
    if ((r = dev_need(c, D.res_count[W], n * S * 8 + 16))) return r;
    if ((r = dev_need(c, D.synth[W], (n + (size_t)P.extra[W]) * ch * n2 * 8 + 16))) return r;
    rows[W].post_valid = (int *)D.post_valid[W].p, rows[W].ilogmask = (ilog_t *)D.ilogmask[W].p, rows[W].res_class = (int *)D.res_class[W].p;
    rows[W].res_entries = (unsigned short *)D.res_entries[W].p, rows[W].res_count = (int *)D.res_count[W].p;
    src[W].nb = (long)n, src[W].post_valid = rows[W].post_valid, src[W].ilogmask = rows[W].ilogmask, src[W].res_class = rows[W].res_class;
    src[W].res_entries = rows[W].res_entries, src[W].res_count = rows[W].res_count;
  }
  // the plan, one piece: order | stream_start | src per size class | the packets' bits | frames | offset_out | the page table
  // | a live call's list for k_unpack and its two carry tables | a live Ogg call's two byte-carry tables
  Arena a;
  const size_t o_order = a.take(4 * nlap), o_start = a.take(8 * ((size_t)ns + 1)), o_src0 = a.take(8 * P.src[0].size() + 8),
               o_src1 = a.take(8 * P.src[1].size() + 8), o_bits = a.take(16 * nb), o_frames = a.take(8 * (size_t)ns), o_off = a.take(8 * (size_t)ns),
               o_pages = a.take(sizeof(OggDepage) * npg), o_unpack = live ? a.take(4 * nb) : o_order, o_in = a.take(sizeof(CarryRow) * nin),
               o_out = a.take(sizeof(CarryRow) * nout), o_bin = a.take(sizeof(OggCarryRow) * nbin), o_bout = a.take(sizeof(OggCarryRow) * nbout),
               o_first = a.take(win ? 8 * (size_t)ns : 0), o_stride = a.take(win ? 8 * (size_t)ns : 0), o_seg = a.take(sizeof(LapSegment) * nseg);
  const size_t plan_bytes = a.at, o_status = a.take(nb + npg);
  if ((r = pinned_get(c, D.h_plan, a.at, true))) return r;
  if ((r = dev_need(c, D.plan, plan_bytes))) return r;
  unsigned char *h = (unsigned char *)D.h_plan.p, *dp = (unsigned char *)D.plan.p;
  if (nlap) memcpy(h + o_order, P.order.data(), 4 * nlap);
  if (live && nb) memcpy(h + o_unpack, unpack.data(), 4 * nb);
  if (nin) memcpy(h + o_in, live->plan->in.data(), sizeof(CarryRow) * nin);
  if (nout) memcpy(h + o_out, live->plan->out.data(), sizeof(CarryRow) * nout);
  if (nbin) memcpy(h + o_bin, live->bytes_in->data(), sizeof(OggCarryRow) * nbin);
  if (nbout) memcpy(h + o_bout, live->bytes_out->data(), sizeof(OggCarryRow) * nbout);
  memcpy(h + o_start, P.lap_start.data(), 8 * ((size_t)ns + 1));
  if (!P.src[0].empty()) memcpy(h + o_src0, P.src[0].data(), 8 * P.src[0].size());
  if (!P.src[1].empty()) memcpy(h + o_src1, P.src[1].data(), 8 * P.src[1].size());
  for (size_t k = 0; k < nb; k++) {
    const int64_t p = P.packet[k];
    const int64_t at = in.begin ? in.begin[p] : in.offset[p];
    ((int64_t *)(h + o_bits))[2 * k] = 8 * (at - byte0);
    ((int64_t *)(h + o_bits))[2 * k + 1] = 8 * (at + (in.offset[p + 1] - in.offset[p]) - byte0);
  }
  memcpy(h + o_frames, P.frames.data(), 8 * (size_t)ns);
  for (int64_t s = 0; s < ns; s++) ((int64_t *)(h + o_off))[s] = P.frames[(size_t)s] > 0 ? offset_out[s] : 0;
  if (npg) memcpy(h + o_pages, in.scan->pages.data(), sizeof(OggDepage) * npg);
  if (win && ns) memcpy(h + o_first, win->first, 8 * (size_t)ns), memcpy(h + o_stride, win->stride, 8 * (size_t)ns);
  for (size_t g = 0; g < nseg; g++) {  // (a stream's rows fill its [ch][frames] from 0 to frames, in order)
    const DecodePlan::Segment &e = (*seg)[g];
    LapSegment row = {e.k0, e.k1, e.first, e.count, P.frames[(size_t)e.stream], offset_out[e.stream] + e.out_at * (D.pcm_interleaved ? ch : 1)};
    memcpy(h + o_seg + g * sizeof(LapSegment), &row, sizeof(row));
  }
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(dp, h, plan_bytes, hipMemcpyHostToDevice, s));
  if (npg) {
    HIP_TRY(c, hipMemcpyAsync(D.files.p, in.files, (size_t)in.files_bytes, hipMemcpyHostToDevice, s));
    if (nbin)
      hipLaunchKernelGGL(k_ogg_packet_carry_in, dim3((unsigned)nbin), dim3(64), 0, s, (const OggCarryRow *)(dp + o_bin), (uint8_t *)D.bytes.p, nbytes,
                         live->bytes_carry, live->slots, live->stride);
    hipLaunchKernelGGL(k_ogg_depage, dim3((unsigned)npg), dim3(64), 0, s, (const uint8_t *)D.files.p, in.files_bytes, (const OggDepage *)(dp + o_pages),
                       (uint8_t *)D.bytes.p, nbytes, (uint8_t *)D.status.p + nb);
    if (nbout)
      hipLaunchKernelGGL(k_ogg_packet_carry_out, dim3((unsigned)nbout), dim3(64), 0, s, (const OggCarryRow *)(dp + o_bout), (uint8_t *)D.bytes.p, nbytes,
                         live->bytes_carry, live->slots, live->stride);
    HIP_TRY(c, hipGetLastError());
  } else if (nbytes) {
    HIP_TRY(c, hipMemcpyAsync(D.bytes.p, in.packets, (size_t)nbytes, hipMemcpyHostToDevice, s));
  }
  const int lanes = D.lanes;
  if (nb && D.partial) {
    hipLaunchKernelGGL(k_unpack_partial, dim3((unsigned)((nb + lanes - 1) / lanes)), dim3(64), (size_t)VAMD_POSIT * lanes * 4, s, (const Bound *)c->d_bound, D.U, lanes, (long)nb,
                       (const uint32_t *)D.bytes.p, nwords,
                       (const long long *)(dp + o_bits), (const int *)(dp + o_unpack), c->B.res_cap[0], c->B.res_cap[1], c->d_dbg ? c->d_dbg + 56 : nullptr,
                       rows[0], rows[1], (unsigned char *)D.status.p);
    HIP_TRY(c, hipGetLastError());
  } else if (nb) {
    hipLaunchKernelGGL(k_unpack, dim3((unsigned)((nb + lanes - 1) / lanes)), dim3(64), (size_t)VAMD_POSIT * lanes * 4, s, (const Bound *)c->d_bound, D.U, lanes, (long)nb,
                       (const uint32_t *)D.bytes.p, nwords,
                       (const long long *)(dp + o_bits), (const int *)(dp + o_unpack), c->B.res_cap[0], c->B.res_cap[1], c->d_dbg ? c->d_dbg + 56 : nullptr,
                       rows[0], rows[1], (unsigned char *)D.status.p);
    HIP_TRY(c, hipGetLastError());
  }
  for (int W = 0; W < 2; W++)
    if (src[W].nb > 0 && (r = launch_synth(c, W, src[W], (float *)D.synth[W].p, D.partial))) return r;
  if (nin || nout) {
    CarryP C;
    C.ch = ch, C.bs0 = c->B.bs[0], C.bs1 = c->B.bs[1];
    C.carry = live->carry, C.synth0 = (float *)D.synth[0].p, C.synth1 = (float *)D.synth[1].p;
    if (nin) hipLaunchKernelGGL(k_decode_carry_in, dim3((unsigned)std::min<size_t>(nin * ch, 256)), dim3(64), 0, s, C, (const CarryRow *)(dp + o_in), (long)nin);
    if (nout) hipLaunchKernelGGL(k_decode_carry_out, dim3((unsigned)std::min<size_t>(nout * ch, 256)), dim3(64), 0, s, C, (const CarryRow *)(dp + o_out), (long)nout);
    HIP_TRY(c, hipGetLastError());
  }
  if (P.max_frames > 0) {
    LapP L;
    L.ch = ch, L.bs0 = c->B.bs[0], L.bs1 = c->B.bs[1];
    L.win0 = c->B.xf[0].win_short, L.win1 = c->B.xf[0].win_long;
    L.order = (const int *)(dp + o_order), L.stream_start = (const long long *)(dp + o_start);
    L.src0 = (const long long *)(dp + o_src0), L.src1 = (const long long *)(dp + o_src1);
    L.synth0 = (const float *)D.synth[0].p, L.synth1 = (const float *)D.synth[1].p;
    const long per_stream = (long)((P.max_frames + 1023) / 1024);  // (as vamd_synth_streams sizes it)
    if (D.pcm_dtype != VAMD_PCM_F32 || D.pcm_interleaved) {
      const LapLaunch A = {s, ns, nseg, P.max_frames, (const long long *)(dp + o_first), (const long long *)(dp + o_frames), (const long long *)(dp + o_stride),
                           (const long long *)(dp + o_off), (const LapSegment *)(dp + o_seg), seg ? 2 : win ? 1 : 0, pcm};
      switch (D.pcm_dtype * 2 + (D.pcm_interleaved ? 1 : 0)) {
        case 1: launch_lap_as<VAMD_PCM_F32, true>(L, A); break;
        case 2: launch_lap_as<VAMD_PCM_S16, false>(L, A); break;
        case 3: launch_lap_as<VAMD_PCM_S16, true>(L, A); break;
        case 4: launch_lap_as<VAMD_PCM_F16, false>(L, A); break;
        case 5: launch_lap_as<VAMD_PCM_F16, true>(L, A); break;
        case 6: launch_lap_as<VAMD_PCM_BF16, false>(L, A); break;
        default: launch_lap_as<VAMD_PCM_BF16, true>(L, A); break;
      }
    } else if (seg)
      hipLaunchKernelGGL(k_lap_segments, dim3((unsigned)(per_stream < 1024 ? per_stream : 1024), (unsigned)(nseg < 1024 ? nseg : 1024)), dim3(256), 0, s, L, (long)nseg,
                         (const LapSegment *)(dp + o_seg), pcm);
    else if (win)
      hipLaunchKernelGGL(k_lap_window, dim3((unsigned)(per_stream < 1024 ? per_stream : 1024), (unsigned)(ns < 1024 ? ns : 1024)), dim3(256), 0, s, L, (long)ns,
                         (const long long *)(dp + o_first), (const long long *)(dp + o_frames), (const long long *)(dp + o_stride),
                         (const long long *)(dp + o_off), pcm);
    else
      hipLaunchKernelGGL(k_lap, dim3((unsigned)(per_stream < 1024 ? per_stream : 1024), (unsigned)(ns < 1024 ? ns : 1024)), dim3(256), 0, s, L, (long)ns,
                         (const long long *)(dp + o_frames), (const long long *)(dp + o_off), pcm);
    HIP_TRY(c, hipGetLastError());
  }
  HIP_TRY(c, hipMemcpyAsync(h + o_status, D.status.p, nb + npg, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  for (int64_t st = 0; st < ns; st++)
    for (int64_t k = unpack_start[(size_t)st]; k < unpack_start[(size_t)st + 1]; k++) status[st] |= h[o_status + (size_t)k];
  for (size_t k = 0; k < npg; k++) status[in.scan->pages[k].stream] |= h[o_status + nb + k];
  return VAMD_OK;
}

// what both entries ask of their outputs, once the plan holds; then the host's statuses go out
static int decode_outputs(vamd_ctx *c, const DecodePlan &P, int64_t ns, const int64_t *offset_out, const float *pcm, uint8_t *status) {
  if (ns && !status) return fail(c, VAMD_EINVAL, "decode: null status");
  if (P.max_frames > 0 && (!offset_out || !pcm)) return fail(c, VAMD_EINVAL, "decode: null offset_out / pcm");
  if ((uintptr_t)pcm % pcm_elem_bytes(c->dec.pcm_dtype)) return fail(c, VAMD_EINVAL, "decode: pcm is not aligned to the output format's element type");
  for (int64_t s = 0; s < ns; s++) {
    if (P.frames[(size_t)s] > 0 && offset_out[s] < 0) return fail(c, VAMD_EINVAL, "decode: negative offset_out");
    status[s] = P.status[(size_t)s];
  }
  return VAMD_OK;
}

// the policy for packets libvorbis decodes in part (include/vorbis_amd.h; k_unpack.h, "TRUNCATED PACKETS"): decode_run picks
// its kernels by it, so every entry follows
int vamd_decode_partial(vamd_ctx *c, int keep) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  int r = decode_ready(c);
  if (r) return r;
  const int was = c->dec.partial ? 1 : 0;
  if (keep < 0) return was;  // (a query)
  if (keep && !was) {  // (as vamd_create opts k_synth in to the full LDS; a no-op where the runtime does not require it)
    (void)hipFuncSetAttribute((const void *)k_synth_bounded, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_per_block);
    (void)hipFuncSetAttribute((const void *)k_synth_values_bounded, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_per_block);
    (void)hipGetLastError();
  }
  c->dec.partial = keep != 0;
  return was;
}

// the policy for the decoded signal's element type and layout (include/vorbis_amd.h, "the decoded signal in the caller's
// format"): decode_run picks its last launch by it, so every entry follows, a live decoder at each call
static int pcm_format_check(vamd_ctx *c, const vamd_pcm_format *fmt) {
  if (fmt && (fmt->dtype < VAMD_PCM_F32 || fmt->dtype > VAMD_PCM_BF16)) return fail(c, VAMD_EINVAL, "pcm format: an unknown dtype");
  return VAMD_OK;
}

int vamd_decode_output(vamd_ctx *c, const vamd_pcm_format *fmt) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  int r = pcm_format_check(c, fmt);
  if (r) return r;
  c->dec.pcm_dtype = fmt ? fmt->dtype : VAMD_PCM_F32;
  c->dec.pcm_interleaved = fmt && fmt->interleaved != 0;
  return VAMD_OK;
}

extern "C++" {
template <int D, bool IL>
static void launch_pcm_convert(hipStream_t s, const float *src, int64_t frames, int ch, void *dst) {
  const long long blocks = (frames * ch + 255) / 256;
  hipLaunchKernelGGL((k_pcm_convert<D, IL>), dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, src, (long long)frames, ch,
                     (typename PcmElem<D>::T *)dst);
}
}  // extern "C++"

int vamd_pcm_convert(vamd_ctx *c, const float *src, int64_t frames, int ch, const vamd_pcm_format *fmt, void *dst) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  int r = pcm_format_check(c, fmt);
  if (r) return r;
  const int dtype = fmt ? fmt->dtype : VAMD_PCM_F32;
  const bool il = fmt && fmt->interleaved != 0;
  if (frames < 0 || ch < 1 || ch > VAMD_MAX_CH || frames > ((int64_t)1 << 56)) return fail(c, VAMD_EINVAL, "pcm_convert: frames < 0 or channels outside 1 .. 8");
  if (!frames) return VAMD_OK;
  if (!src || !dst) return fail(c, VAMD_EINVAL, "pcm_convert: null src / dst");
  if ((uintptr_t)src % 4 || (uintptr_t)dst % pcm_elem_bytes(dtype)) return fail(c, VAMD_EINVAL, "pcm_convert: src / dst is not aligned to its element type");
  switch (dtype * 2 + (il ? 1 : 0)) {
    case 0: launch_pcm_convert<VAMD_PCM_F32, false>(c->stream, src, frames, ch, dst); break;
    case 1: launch_pcm_convert<VAMD_PCM_F32, true>(c->stream, src, frames, ch, dst); break;
    case 2: launch_pcm_convert<VAMD_PCM_S16, false>(c->stream, src, frames, ch, dst); break;
    case 3: launch_pcm_convert<VAMD_PCM_S16, true>(c->stream, src, frames, ch, dst); break;
    case 4: launch_pcm_convert<VAMD_PCM_F16, false>(c->stream, src, frames, ch, dst); break;
    case 5: launch_pcm_convert<VAMD_PCM_F16, true>(c->stream, src, frames, ch, dst); break;
    case 6: launch_pcm_convert<VAMD_PCM_BF16, false>(c->stream, src, frames, ch, dst); break;
    default: launch_pcm_convert<VAMD_PCM_BF16, true>(c->stream, src, frames, ch, dst); break;
  }
  HIP_TRY(c, hipGetLastError());
  return VAMD_OK;
}

int vamd_decode_streams(vamd_ctx *c, const vamd_decode_desc *d, const int64_t *offset_out, float *pcm, uint8_t *status) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  DecodePlan P;
  int r = decode_plan(c, d, &P);
  if (r) return r;
  if ((r = decode_outputs(c, P, d->nstreams, offset_out, pcm, status))) return r;
  if (P.order.empty()) return VAMD_OK;
  DecodeInput in;
  in.offset = d->offset, in.byte0 = d->offset[0], in.nbytes = d->offset[d->npackets] - d->offset[0];
  in.packets = d->bytes + in.byte0;
  return decode_run(c, P, d->nstreams, in, offset_out, pcm, status);
}

// ---- packets with marks: vamd_decode_plan_marked, vamd_decode_streams_marked ----
// The reader's granule walk (vamd_decode_plan.h, decode_plan_build_marked) in the block plan's place; the rest is the
// packet entry, with the plan's segments for the lap.
static int decode_plan_marked(vamd_ctx *c, const vamd_decode_desc *d, const vamd_decode_marks *m, DecodePlan *P) {
  if (!d) return fail(c, VAMD_EINVAL, "decode: null descriptor");
  if (!m) return fail(c, VAMD_EINVAL, "decode: null marks");
  int r = decode_ready(c);
  if (r) return r;
  std::string err;
  if (!decode_plan_build_marked(c->B.bs, c->dec.U.modes, c->dec.U.modebits, d->nstreams, d->npackets, d->bytes, d->offset, d->stream_start, m->granule,
                                m->eos, P, &err))
    return fail(c, VAMD_EINVAL, err.c_str());
  return VAMD_OK;
}

int vamd_decode_plan_marked(vamd_ctx *c, const vamd_decode_desc *d, const vamd_decode_marks *m, int64_t *frames, int64_t *nblocks) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  DecodePlan P;
  int r = decode_plan_marked(c, d, m, &P);
  if (r) return r;
  for (int64_t s = 0; frames && s < d->nstreams; s++) frames[s] = P.frames[(size_t)s];
  if (nblocks) nblocks[0] = P.nblocks[0], nblocks[1] = P.nblocks[1];
  return VAMD_OK;
}

int vamd_decode_streams_marked(vamd_ctx *c, const vamd_decode_desc *d, const vamd_decode_marks *m, const int64_t *offset_out, float *pcm, uint8_t *status) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  DecodePlan P;
  int r = decode_plan_marked(c, d, m, &P);
  if (r) return r;
  if ((r = decode_outputs(c, P, d->nstreams, offset_out, pcm, status))) return r;
  if (P.order.empty()) return VAMD_OK;
  DecodeInput in;
  in.offset = d->offset, in.byte0 = d->offset[0], in.nbytes = d->offset[d->npackets] - d->offset[0];
  in.packets = d->bytes + in.byte0;
  return decode_run(c, P, d->nstreams, in, offset_out, pcm, status, nullptr, nullptr, &P.segments);
}

// the policy for files as a reader takes them (include/vorbis_amd.h; vamd_demux.h, "links and foreign pages"): the two
// whole-file entries below read it, no other entry does
int vamd_decode_follow(vamd_ctx *c, int on) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  const int was = c->dec.follow ? 1 : 0;
  if (on >= 0) c->dec.follow = on != 0;  // (a negative value is a query)
  return was;
}

// ---- files in: vamd_decode_ogg_plan, vamd_decode_ogg ----
// The host's walk (vamd_demux.h), then the block plan over its packet table with the first bytes it read in place.
static int decode_ogg_plan(vamd_ctx *c, const vamd_decode_ogg_desc *d, DemuxScan *X, DecodePlan *P) {
  if (!d) return fail(c, VAMD_EINVAL, "decode_ogg: null descriptor");
  int r = decode_ready(c);
  if (r) return r;
  DemuxSetup S;
  S.channels = c->B.channels, S.rate = c->B.rate, S.bs[0] = c->B.bs[0], S.bs[1] = c->B.bs[1];
  S.setup_header = d->setup_header, S.setup_header_bytes = d->setup_header_bytes;
  demux_own_setup(c, &S);
  std::string err;
  if (!demux_scan(d->nstreams, d->bytes, d->file_offset, S, X, &err, c->dec.follow)) return fail(c, VAMD_EINVAL, err.c_str());
  if (X->pages.size() > 0x7fffffffu) return fail(c, VAMD_EINVAL, "decode_ogg: more than 2^31 pages");
  if (c->dec.follow) {  // (the marks the walk read off the pages, and its links, in the end granule's place)
    if (!decode_plan_build_marked(c->B.bs, c->dec.U.modes, c->dec.U.modebits, d->nstreams, (int64_t)X->first.size(), nullptr, X->offset.data(),
                                  X->stream_start.data(), X->granule.data(), X->eos.data(), P, &err, X->first.data(), X->links.data(), (int64_t)X->links.size()))
      return fail(c, VAMD_EINVAL, err.c_str());
  } else if (!decode_plan_build(c->B.bs, c->dec.U.modes, c->dec.U.modebits, d->nstreams, (int64_t)X->first.size(), nullptr, X->offset.data(),
                         X->stream_start.data(), X->end_granule.data(), P, &err, X->first.data()))
    return fail(c, VAMD_EINVAL, err.c_str());
  for (int64_t s = 0; s < d->nstreams; s++) P->status[(size_t)s] |= X->status[(size_t)s];
  return VAMD_OK;
}

int vamd_decode_ogg_plan(vamd_ctx *c, const vamd_decode_ogg_desc *d, int64_t *frames, int64_t *nblocks) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  DemuxScan X;
  DecodePlan P;
  int r = decode_ogg_plan(c, d, &X, &P);
  if (r) return r;
  for (int64_t s = 0; frames && s < d->nstreams; s++) frames[s] = P.frames[(size_t)s];
  if (nblocks) nblocks[0] = P.nblocks[0], nblocks[1] = P.nblocks[1];
  return VAMD_OK;
}

int vamd_decode_ogg(vamd_ctx *c, const vamd_decode_ogg_desc *d, const int64_t *offset_out, float *pcm, uint8_t *status) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  DemuxScan X;
  DecodePlan P;
  int r = decode_ogg_plan(c, d, &X, &P);
  if (r) return r;
  if ((r = decode_outputs(c, P, d->nstreams, offset_out, pcm, status))) return r;
  DecodeInput in;
  in.offset = X.offset.data(), in.byte0 = 0, in.nbytes = X.offset.back();
  in.scan = &X, in.files = d->bytes + d->file_offset[0], in.files_bytes = d->file_offset[d->nstreams] - d->file_offset[0];
  return decode_run(c, P, d->nstreams, in, offset_out, pcm, status, nullptr, nullptr, c->dec.follow ? &P.segments : nullptr);
}

// ---- a file's three header packets, a file's links (host only) ----
static int ogg_read_headers(const uint8_t *file, int64_t bytes, const uint32_t *serial, uint8_t *out, int64_t cap, int64_t len[3]) {
  if (!file || bytes < 0 || !len || cap < 0 || (cap > 0 && !out)) return VAMD_EINVAL;
  std::vector<uint8_t> header[3];
  len[0] = len[1] = len[2] = 0;
  if (!demux_read_headers(file, bytes, header, serial)) return VAMD_EBADHEADER;
  int64_t total = 0;
  for (int k = 0; k < 3; k++) total += len[k] = (int64_t)header[k].size();
  if (total > cap) return VAMD_EINVAL;
  for (int k = 0; k < 3; k++) {
    if (!header[k].empty()) memcpy(out, header[k].data(), header[k].size());
    out += header[k].size();
  }
  return VAMD_OK;
}

int vamd_ogg_read_headers(const uint8_t *file, int64_t bytes, uint8_t *out, int64_t cap, int64_t len[3]) {
  return ogg_read_headers(file, bytes, nullptr, out, cap, len);
}

int vamd_ogg_read_headers_serial(const uint8_t *file, int64_t bytes, uint32_t serial, uint8_t *out, int64_t cap, int64_t len[3]) {
  return ogg_read_headers(file, bytes, &serial, out, cap, len);
}

int vamd_ogg_links(const uint8_t *file, int64_t bytes, vamd_ogg_link *out, int64_t cap, int64_t *nlinks) {
  if (!file || bytes < 0 || !nlinks || cap < 0 || (cap > 0 && !out)) return VAMD_EINVAL;
  std::vector<DemuxLink> links;
  const bool whole = demux_links(file, bytes, &links);
  *nlinks = (int64_t)links.size();
  for (int64_t k = 0; k < *nlinks && k < cap; k++) out[k].begin = links[(size_t)k].begin, out[k].end = links[(size_t)k].end, out[k].serial = links[(size_t)k].serial;
  if (!whole) return VAMD_EBADHEADER;
  return *nlinks > cap ? VAMD_EINVAL : VAMD_OK;
}
