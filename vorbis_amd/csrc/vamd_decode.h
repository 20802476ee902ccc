// vamd_decode.h -- the packet decoder's host side (include/vorbis_amd.h: vamd_decode_plan, vamd_decode_streams): audio
// packets in host memory to PCM in device memory.  Part of the library's single translation unit, after vamd_batch.h
// (launch_synth, synth_covered).  Every entry makes its plan on the host before anything is enqueued (vamd_decode_plan.h)
// and then hands decode_run that plan, where its bytes come from (DecodeInput) and what it adds to the plain case
// (DecodeAdds).  decode_run is these steps on the context's stream, each a function below that tests for itself whether
// the call gives it anything to do:
//   workspace  the context's buffers, grown on demand (the table decode_class_bufs, and the arena, statuses and files)
//   layout     where the plan image's parts lie (vamd_decode_layout.h), and the pinned and device buffers for it
//   fill       the image, written on the host (vamd_decode_layout.h)
//   upload     the image, one copy; the packets, or the files' pages as they lie, one copy
//   depage     (pages) k_ogg_depage checks every page's checksum and moves the audio bytes into the packed arena (k_demux.h);
//              a live Ogg call's open packets are carried around it by k_ogg_packet_carry_in / _out
//   unpack     k_unpack, or under vamd_decode_partial k_unpack_partial: every packet into its block's rows (k_unpack.h)
//   synth      k_synth per size class on those rows (k_synth.h, the launch the encoder's tensors take)
//   carry      (live) the carried blocks in, the last blocks out: k_decode_carry_in / _out
//   lap        the streams' samples gathered in the caller's format: k_lap, for windows k_lap_window, for a plan made from
//              marks k_lap_segments, or their _as forms (vamd_decode_output)
//   statuses   the blocks' and the pages' back in one copy, one synchronise, folded into their streams
// The entries: packets (here); packets with marks and, under vamd_decode_follow, whole files, whose plan is the reader's
// granule walk with its runs of kept frames as the lap's rows (decode_plan_build_marked); whole Ogg files, walked by the
// host (vamd_demux.h) and unpaged on the device; windows of streams or of indexed files, the plan's "streams" being the
// windows (vamd_decode_window.h); the next pieces of continuing streams, with the blocks carried between pieces standing
// in the plan (vamd_decode_live.h); and the next BYTES of continuing Ogg streams, both of the last two at once
// (vamd_decode_ogg_live.h).
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

// The workspace per size class: each buffer and the bytes a block of class W takes of it.  decode_workspace grows them by
// this table and decode_release frees them by it.  `carried`: a live call's carried blocks have rows in it too.
struct DecodeClassBuf {
  DevBuf (vamd_ctx::Decode::*buf)[2];
  size_t (*per_block)(const Bound &B, int W);
  bool carried;
};
static const DecodeClassBuf decode_class_bufs[] = {
    {&vamd_ctx::Decode::post_valid, [](const Bound &B, int) { return (size_t)B.channels * 4; }, false},
    {&vamd_ctx::Decode::ilogmask, [](const Bound &B, int W) { return (size_t)B.channels * ((size_t)B.bs[W] / 2); }, false},
    {&vamd_ctx::Decode::res_class, [](const Bound &B, int W) { return (size_t)B.chmap[W].submaps * VAMD_RES_CLASS_STRIDE * 4; }, false},
    {&vamd_ctx::Decode::res_entries, [](const Bound &B, int W) { return (size_t)B.res_cap[W] * 2; }, false},
    {&vamd_ctx::Decode::res_count, [](const Bound &B, int W) { return (size_t)B.chmap[W].submaps * 8; }, false},
    {&vamd_ctx::Decode::synth, [](const Bound &B, int W) { return (size_t)B.channels * ((size_t)B.bs[W] / 2) * 8; }, true},
};

static void decode_release(vamd_ctx *c) {
  vamd_ctx::Decode &D = c->dec;
  for (DevBuf *b : {&D.bytes, &D.plan, &D.status, &D.files})
    if (b->p) (void)hipFree(b->p);
  for (const DecodeClassBuf &t : decode_class_bufs)
    for (int W = 0; W < 2; W++)
      if ((D.*t.buf)[W].p) (void)hipFree((D.*t.buf)[W].p);
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

// What the host's page walks hold a file to: the context's stream shape and a setup header packet -- the call's, or, where
// the call names none, the one a context made from a stream's headers was made from (vamd_create_decoder; a blob context
// has none to hold it to).
static DemuxSetup demux_setup(const vamd_ctx *c, const uint8_t *header, int64_t bytes) {
  DemuxSetup S;
  S.channels = c->B.channels, S.rate = c->B.rate, S.bs[0] = c->B.bs[0], S.bs[1] = c->B.bs[1];
  S.setup_header = header, S.setup_header_bytes = bytes;
  if (!S.setup_header && !S.setup_header_bytes && !c->setup_packet.empty())
    S.setup_header = c->setup_packet.data(), S.setup_header_bytes = (int64_t)c->setup_packet.size();
  return S;
}

// what every _plan entry reports of a plan that holds: the frames of its ns streams (or windows), the blocks per size class
static void decode_report(const DecodePlan &P, int64_t ns, int64_t *frames, int64_t *nblocks) {
  for (int64_t s = 0; frames && s < ns; s++) frames[s] = P.frames[(size_t)s];
  if (nblocks) nblocks[0] = P.nblocks[0], nblocks[1] = P.nblocks[1];
}

// The block plan of a packet descriptor.  With marks (m may be null: none), the reader's granule walk over them in its
// place (vamd_decode_plan.h, decode_plan_build_marked), links from a fresh lap.
static int decode_plan(vamd_ctx *c, const vamd_decode_desc *d, const vamd_decode_marks *m, DecodePlan *P) {
  if (!d) return fail(c, VAMD_EINVAL, "decode: null descriptor");
  int r = decode_ready(c);
  if (r) return r;
  std::string err;
  const bool ok = m ? decode_plan_build_marked(c->B.bs, c->dec.U.modes, c->dec.U.modebits, d->nstreams, d->npackets, d->bytes, d->offset, d->stream_start,
                                                    m->granule, m->eos, P, &err)
                         : decode_plan_build(c->B.bs, c->dec.U.modes, c->dec.U.modebits, d->nstreams, d->npackets, d->bytes, d->offset, d->stream_start,
                                             d->end_granule, P, &err);
  if (!ok) return fail(c, VAMD_EINVAL, err.c_str());
  return VAMD_OK;
}

// What an entry hands decode_run: the packed arena's packet table, and where its bytes come from -- the caller's host
// memory as they are (the packet entries), or the files' pages by way of k_ogg_depage (the Ogg entries).
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

// the packet form: npackets packets back to back in host memory, packet p at bytes[offset[p] .. offset[p + 1])
static DecodeInput decode_input_packets(const uint8_t *bytes, const int64_t *offset, int64_t npackets) {
  DecodeInput in;
  in.offset = offset, in.byte0 = offset[0], in.nbytes = offset[npackets] - offset[0];
  in.packets = bytes + in.byte0;
  return in;
}

// What a call adds to the plain case (packets or files, whole streams, a block plan); a default one adds nothing.
struct DecodeAdds {
  // a live decoder's call (vamd_decode_live.h): P is live->P, whose order[] holds carried blocks that have no packet;
  // k_unpack and the statuses take the plan's own list, and the carries move between k_synth and the lap
  const DecodeLivePlan *live = nullptr;
  float *carry = nullptr;  // [slots][ch][bs[1]/2]
  // ... and a live Ogg decoder's byte carry (vamd_decode_ogg_live.h): k_ogg_packet_carry_in ahead of k_ogg_depage, _out behind it
  const std::vector<OggCarryRow> *bytes_in = nullptr, *bytes_out = nullptr;
  uint8_t *bytes_carry = nullptr;  // [slots][bytes_stride]
  int64_t slots = 0, bytes_stride = 0;
  // a window call (vamd_decode_window.h): P's "streams" are windows, each with its first frame in its stream and its channel
  // stride in pcm, [ns] each; the lap is k_lap_window's
  const int64_t *first = nullptr, *stride = nullptr;
  // a plan made from marks (decode_plan_build_marked): its runs of kept frames; the lap is k_lap_segments'
  const std::vector<DecodePlan::Segment> *segments = nullptr;
};

// A call on its way through decode_run's steps: what it was handed, its counts, and what the steps before have made.
extern "C++" {
struct DecodeCall {
  const DecodePlan &P;
  const DecodeInput &in;
  const DecodeAdds &add;
  int64_t ns;
  DecodeCounts n;
  long long nwords = 0;                       // the packed arena in 32-bit words
  UnpackRows rows[2];                         // workspace: k_unpack's rows per size class ...
  vamd_ctx::SynthSrc src[2];                  // ... as k_synth takes them
  DecodeLayout o;                             // layout
  unsigned char *h = nullptr, *dp = nullptr;  // the image in pinned memory and on the device
  template <class T> const T *dev(size_t at) const { return (const T *)(dp + at); }  // a part of the image as the kernels take it
};
}  // extern "C++"

static DecodeCounts decode_counts(const DecodePlan &P, int64_t ns, const DecodeInput &in, const DecodeAdds &add) {
  DecodeCounts n;
  n.live = add.live != nullptr, n.win = add.first != nullptr;
  n.nb = n.live ? add.live->unpack.size() : P.order.size();
  n.nlap = P.order.size(), n.ns = (size_t)ns, n.nsrc[0] = P.src[0].size(), n.nsrc[1] = P.src[1].size();
  n.npg = in.scan ? in.scan->pages.size() : 0;
  if (n.live) n.nin = add.live->in.size(), n.nout = add.live->out.size();
  if (n.live && add.bytes_in) n.nbin = add.bytes_in->size();
  if (n.live && add.bytes_out) n.nbout = add.bytes_out->size();
  if (add.segments) n.nseg = add.segments->size();
  return n;
}

static int decode_workspace(vamd_ctx *c, DecodeCall &K) {
  vamd_ctx::Decode &D = c->dec;
  int r;
  K.nwords = (long long)((K.in.nbytes + 3) / 4);
  if ((r = dev_need(c, D.bytes, (size_t)K.nwords * 4 + 16))) return r;
  if ((r = dev_need(c, D.status, K.n.nb + K.n.npg + 16))) return r;
  if (K.n.npg && (r = dev_need(c, D.files, (((size_t)K.in.files_bytes + 3) & ~(size_t)3) + 16))) return r;
  for (int W = 0; W < 2; W++) {
    const size_t n = (size_t)K.P.nblocks[W];
    for (const DecodeClassBuf &t : decode_class_bufs)
      if ((r = dev_need(c, (D.*t.buf)[W], (n + (t.carried ? (size_t)K.P.extra[W] : 0)) * t.per_block(c->B, W) + 16))) return r;
    UnpackRows &R = K.rows[W];
    R.post_valid = (int *)D.post_valid[W].p, R.ilogmask = (ilog_t *)D.ilogmask[W].p, R.res_class = (int *)D.res_class[W].p;
    R.res_entries = (unsigned short *)D.res_entries[W].p, R.res_count = (int *)D.res_count[W].p;
    vamd_ctx::SynthSrc &S = K.src[W];
    S.nb = (long)n, S.post_valid = R.post_valid, S.ilogmask = R.ilogmask, S.res_class = R.res_class;
    S.res_entries = R.res_entries, S.res_count = R.res_count;
  }
  return VAMD_OK;
}

static int decode_layout_buffers(vamd_ctx *c, DecodeCall &K) {
  vamd_ctx::Decode &D = c->dec;
  int r;
  K.o = decode_layout(K.n);
  if ((r = pinned_get(c, D.h_plan, K.o.total, true))) return r;
  if ((r = dev_need(c, D.plan, K.o.plan_bytes))) return r;
  K.h = (unsigned char *)D.h_plan.p, K.dp = (unsigned char *)D.plan.p;
  return VAMD_OK;
}

static void decode_fill(const vamd_ctx *c, const DecodeCall &K, const int64_t *offset_out) {
  const DecodePlan &P = K.P;
  DecodeImage s;
  s.order = P.order.data(), s.start = P.lap_start.data(), s.src[0] = P.src[0].data(), s.src[1] = P.src[1].data();
  s.packet = P.packet.data(), s.offset = K.in.offset, s.begin = K.in.begin, s.byte0 = K.in.byte0;
  s.frames = P.frames.data(), s.offset_out = offset_out;
  if (K.n.npg) s.pages = K.in.scan->pages.data();
  if (K.n.live) s.unpack = K.add.live->unpack.data(), s.in = K.add.live->in.data(), s.out = K.add.live->out.data();
  if (K.n.nbin) s.bin = K.add.bytes_in->data();
  if (K.n.nbout) s.bout = K.add.bytes_out->data();
  s.first = K.add.first, s.stride = K.add.stride;
  if (K.n.nseg) s.seg = K.add.segments->data();
  s.out_scale = c->dec.pcm_interleaved ? c->B.channels : 1;
  decode_image_fill(K.n, K.o, s, K.h);
}

static int decode_upload(vamd_ctx *c, const DecodeCall &K) {
  vamd_ctx::Decode &D = c->dec;
  HIP_TRY(c, hipMemcpyAsync(K.dp, K.h, K.o.plan_bytes, hipMemcpyHostToDevice, c->stream));
  if (K.n.npg) HIP_TRY(c, hipMemcpyAsync(D.files.p, K.in.files, (size_t)K.in.files_bytes, hipMemcpyHostToDevice, c->stream));
  else if (K.in.nbytes) HIP_TRY(c, hipMemcpyAsync(D.bytes.p, K.in.packets, (size_t)K.in.nbytes, hipMemcpyHostToDevice, c->stream));
  return VAMD_OK;
}

static int decode_depage(vamd_ctx *c, const DecodeCall &K) {
  if (!K.n.npg) return VAMD_OK;
  vamd_ctx::Decode &D = c->dec;
  const DecodeAdds &A = K.add;
  hipStream_t s = c->stream;
  const int64_t nbytes = K.in.nbytes;
  if (K.n.nbin)
    hipLaunchKernelGGL(k_ogg_packet_carry_in, dim3((unsigned)K.n.nbin), dim3(64), 0, s, K.dev<OggCarryRow>(K.o.bin), (uint8_t *)D.bytes.p, nbytes, A.bytes_carry,
                       A.slots, A.bytes_stride);
  hipLaunchKernelGGL(k_ogg_depage, dim3((unsigned)K.n.npg), dim3(64), 0, s, (const uint8_t *)D.files.p, K.in.files_bytes, K.dev<OggDepage>(K.o.pages),
                     (uint8_t *)D.bytes.p, nbytes, (uint8_t *)D.status.p + K.n.nb);
  if (K.n.nbout)
    hipLaunchKernelGGL(k_ogg_packet_carry_out, dim3((unsigned)K.n.nbout), dim3(64), 0, s, K.dev<OggCarryRow>(K.o.bout), (uint8_t *)D.bytes.p, nbytes, A.bytes_carry,
                       A.slots, A.bytes_stride);
  HIP_TRY(c, hipGetLastError());
  return VAMD_OK;
}

static int decode_unpack(vamd_ctx *c, const DecodeCall &K) {
  if (!K.n.nb) return VAMD_OK;
  vamd_ctx::Decode &D = c->dec;
  const int lanes = D.lanes;
  hipLaunchKernelGGL(D.partial ? k_unpack_partial : k_unpack, dim3((unsigned)((K.n.nb + lanes - 1) / lanes)), dim3(64), (size_t)VAMD_POSIT * lanes * 4, c->stream,
                     (const Bound *)c->d_bound, D.U, lanes, (long)K.n.nb, (const uint32_t *)D.bytes.p, K.nwords, K.dev<long long>(K.o.bits), K.dev<int>(K.o.unpack),
                     c->B.res_cap[0], c->B.res_cap[1], c->d_dbg ? c->d_dbg + 56 : nullptr, K.rows[0], K.rows[1], (unsigned char *)D.status.p);
  HIP_TRY(c, hipGetLastError());
  return VAMD_OK;
}

static int decode_synth(vamd_ctx *c, const DecodeCall &K) {
  int r;
  for (int W = 0; W < 2; W++)
    if (K.src[W].nb > 0 && (r = launch_synth(c, W, K.src[W], (float *)c->dec.synth[W].p, c->dec.partial))) return r;
  return VAMD_OK;
}

static int decode_carry(vamd_ctx *c, const DecodeCall &K) {
  const size_t nin = K.n.nin, nout = K.n.nout;
  if (!nin && !nout) return VAMD_OK;
  vamd_ctx::Decode &D = c->dec;
  const int ch = c->B.channels;
  CarryP C;
  C.ch = ch, C.bs0 = c->B.bs[0], C.bs1 = c->B.bs[1];
  C.carry = K.add.carry, C.synth0 = (float *)D.synth[0].p, C.synth1 = (float *)D.synth[1].p;
  if (nin) hipLaunchKernelGGL(k_decode_carry_in, dim3((unsigned)std::min<size_t>(nin * ch, 256)), dim3(64), 0, c->stream, C, K.dev<CarryRow>(K.o.in), (long)nin);
  if (nout) hipLaunchKernelGGL(k_decode_carry_out, dim3((unsigned)std::min<size_t>(nout * ch, 256)), dim3(64), 0, c->stream, C, K.dev<CarryRow>(K.o.out), (long)nout);
  HIP_TRY(c, hipGetLastError());
  return VAMD_OK;
}

static size_t pcm_elem_bytes(int dtype) { return dtype == VAMD_PCM_F32 ? 4 : 2; }

extern "C++" {
// One element type and layout (include/vorbis_amd.h, vamd_pcm_format) as template arguments: f(dtype, interleaved), both
// constants -- f<VAMD_PCM_S16, true> is f(std::integral_constant<int, VAMD_PCM_S16>(), std::true_type()).
template <class F>
static void pcm_dispatch(int dtype, bool interleaved, F f) {
  switch (dtype * 2 + (interleaved ? 1 : 0)) {
    case 0: f(std::integral_constant<int, VAMD_PCM_F32>(), std::false_type()); break;
    case 1: f(std::integral_constant<int, VAMD_PCM_F32>(), std::true_type()); break;
    case 2: f(std::integral_constant<int, VAMD_PCM_S16>(), std::false_type()); break;
    case 3: f(std::integral_constant<int, VAMD_PCM_S16>(), std::true_type()); break;
    case 4: f(std::integral_constant<int, VAMD_PCM_F16>(), std::false_type()); break;
    case 5: f(std::integral_constant<int, VAMD_PCM_F16>(), std::true_type()); break;
    case 6: f(std::integral_constant<int, VAMD_PCM_BF16>(), std::false_type()); break;
    default: f(std::integral_constant<int, VAMD_PCM_BF16>(), std::true_type()); break;
  }
}

// The three gathers of a format.  F32 planar's are the kernels every decode took before there were formats, four frames a
// thread; the other seven formats' are the _as forms, PcmOut's elements a thread (k_synth.h).
template <int D, bool IL> struct LapKernels {
  static auto lap() { return k_lap_as<D, IL>; }
  static auto window() { return k_lap_window_as<D, IL>; }
  static auto segments() { return k_lap_segments_as<D, IL>; }
  static long long threads(long long max_frames, int ch) { return (IL ? max_frames * ch : max_frames) / PcmOut<D, IL>::per_thread + 2; }
};
template <> struct LapKernels<VAMD_PCM_F32, false> {
  static auto lap() { return k_lap; }
  static auto window() { return k_lap_window; }
  static auto segments() { return k_lap_segments; }
  static long long threads(long long max_frames, int) { return (max_frames + 3) / 4; }  // (as vamd_synth_streams sizes it)
};
}  // extern "C++"

static int decode_lap(vamd_ctx *c, const DecodeCall &K, void *pcm) {
  if (K.P.max_frames <= 0) return VAMD_OK;
  vamd_ctx::Decode &D = c->dec;
  LapP L;
  L.ch = c->B.channels, L.bs0 = c->B.bs[0], L.bs1 = c->B.bs[1];
  L.win0 = c->B.xf[0].win_short, L.win1 = c->B.xf[0].win_long;
  L.order = K.dev<int>(K.o.order), L.stream_start = K.dev<long long>(K.o.start);
  L.src0 = K.dev<long long>(K.o.src[0]), L.src1 = K.dev<long long>(K.o.src[1]);
  L.synth0 = (const float *)D.synth[0].p, L.synth1 = (const float *)D.synth[1].p;
  const long ns = (long)K.ns, nseg = (long)K.n.nseg;
  const bool marked = K.add.segments != nullptr;
  pcm_dispatch(D.pcm_dtype, D.pcm_interleaved, [&](auto dtype, auto interleaved) {
    typedef LapKernels<decltype(dtype)::value, decltype(interleaved)::value> Kernels;
    typedef typename PcmElem<decltype(dtype)::value>::T T;
    // the grid: x over a row's threads in workgroups of 256, y over the streams (windows, segments), at most 1024 each way
    // (the kernels stride)
    auto cap = [](long long v) { return (unsigned)(v < 1024 ? v : 1024); };
    const dim3 grid(cap((Kernels::threads(K.P.max_frames, L.ch) + 255) / 256), cap(marked ? nseg : ns)), wg(256);
    hipStream_t s = c->stream;
    if (marked) hipLaunchKernelGGL(Kernels::segments(), grid, wg, 0, s, L, nseg, K.dev<LapSegment>(K.o.seg), (T *)pcm);
    else if (K.n.win)
      hipLaunchKernelGGL(Kernels::window(), grid, wg, 0, s, L, ns, K.dev<long long>(K.o.first), K.dev<long long>(K.o.frames), K.dev<long long>(K.o.stride),
                         K.dev<long long>(K.o.off), (T *)pcm);
    else hipLaunchKernelGGL(Kernels::lap(), grid, wg, 0, s, L, ns, K.dev<long long>(K.o.frames), K.dev<long long>(K.o.off), (T *)pcm);
  });
  HIP_TRY(c, hipGetLastError());
  return VAMD_OK;
}

static int decode_statuses(vamd_ctx *c, const DecodeCall &K, uint8_t *status) {
  const size_t nb = K.n.nb, npg = K.n.npg;
  const unsigned char *got = K.h + K.o.status;
  HIP_TRY(c, hipMemcpyAsync(K.h + K.o.status, c->dec.status.p, nb + npg, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  const std::vector<int64_t> &start = K.n.live ? K.add.live->unpack_start : K.P.lap_start;
  for (int64_t st = 0; st < K.ns; st++)
    for (int64_t k = start[(size_t)st]; k < start[(size_t)st + 1]; k++) status[st] |= got[(size_t)k];
  for (size_t k = 0; k < npg; k++) status[K.in.scan->pages[k].stream] |= got[nb + k];
  return VAMD_OK;
}

// The tail all entries share, behind a plan that holds and statuses the host has already set: the steps of the header
// comment, in its order.  P's ns "streams" are `add`'s windows where it has any, and add.live->P where it is live.
static int decode_run(vamd_ctx *c, const DecodePlan &P, int64_t ns, const DecodeInput &in, const int64_t *offset_out, float *pcm, uint8_t *status,
                      const DecodeAdds &add = DecodeAdds()) {
  DecodeCall K = {P, in, add, ns, decode_counts(P, ns, in, add)};
  if (!K.n.nb && !K.n.npg) return VAMD_OK;
  int r;
  if ((r = decode_workspace(c, K))) return r;
  if ((r = decode_layout_buffers(c, K))) return r;
  decode_fill(c, K, offset_out);
  if ((r = decode_upload(c, K))) return r;
  if ((r = decode_depage(c, K))) return r;
  if ((r = decode_unpack(c, K))) return r;
  if ((r = decode_synth(c, K))) return r;
  if ((r = decode_carry(c, K))) return r;
  if ((r = decode_lap(c, K, pcm))) return r;
  return decode_statuses(c, K, status);
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
  const long long blocks = (frames * ch + 255) / 256;
  pcm_dispatch(dtype, il, [&](auto d, auto interleaved) {
    hipLaunchKernelGGL((k_pcm_convert<decltype(d)::value, decltype(interleaved)::value>), dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, c->stream,
                       src, (long long)frames, ch, (typename PcmElem<decltype(d)::value>::T *)dst);
  });
  HIP_TRY(c, hipGetLastError());
  return VAMD_OK;
}

// ---- packets, and packets with marks: vamd_decode_plan, vamd_decode_streams and their _marked forms ----
static int decode_plan_entry(vamd_ctx *c, const vamd_decode_desc *d, const vamd_decode_marks *m, int64_t *frames, int64_t *nblocks) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  DecodePlan P;
  int r = decode_plan(c, d, m, &P);
  if (r) return r;
  decode_report(P, d->nstreams, frames, nblocks);
  return VAMD_OK;
}

static int decode_streams_entry(vamd_ctx *c, const vamd_decode_desc *d, const vamd_decode_marks *m, const int64_t *offset_out, float *pcm,
                                uint8_t *status) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  DecodePlan P;
  int r = decode_plan(c, d, m, &P);
  if (r) return r;
  if ((r = decode_outputs(c, P, d->nstreams, offset_out, pcm, status))) return r;
  if (P.order.empty()) return VAMD_OK;
  DecodeAdds add;
  if (m) add.segments = &P.segments;
  return decode_run(c, P, d->nstreams, decode_input_packets(d->bytes, d->offset, d->npackets), offset_out, pcm, status, add);
}

int vamd_decode_plan(vamd_ctx *c, const vamd_decode_desc *d, int64_t *frames, int64_t *nblocks) { return decode_plan_entry(c, d, nullptr, frames, nblocks); }

int vamd_decode_streams(vamd_ctx *c, const vamd_decode_desc *d, const int64_t *offset_out, float *pcm, uint8_t *status) {
  return decode_streams_entry(c, d, nullptr, offset_out, pcm, status);
}

int vamd_decode_plan_marked(vamd_ctx *c, const vamd_decode_desc *d, const vamd_decode_marks *m, int64_t *frames, int64_t *nblocks) {
  if (c && d && !m) return fail(c, VAMD_EINVAL, "decode: null marks");  // (behind the entry's own refusals of a null c or d)
  return decode_plan_entry(c, d, m, frames, nblocks);
}

int vamd_decode_streams_marked(vamd_ctx *c, const vamd_decode_desc *d, const vamd_decode_marks *m, const int64_t *offset_out, float *pcm, uint8_t *status) {
  if (c && d && !m) return fail(c, VAMD_EINVAL, "decode: null marks");
  return decode_streams_entry(c, d, m, offset_out, pcm, status);
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
  const DemuxSetup S = demux_setup(c, d->setup_header, d->setup_header_bytes);
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
  decode_report(P, d->nstreams, frames, nblocks);
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
  DecodeAdds add;
  if (c->dec.follow) add.segments = &P.segments;
  return decode_run(c, P, d->nstreams, in, offset_out, pcm, status, add);
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
