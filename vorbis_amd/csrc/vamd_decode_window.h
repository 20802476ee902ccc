// vamd_decode_window.h -- windows of streams and of Ogg files (include/vorbis_amd.h: vamd_decode_window_plan,
// vamd_decode_window; vamd_ogg_index_create, vamd_decode_ogg_window_plan, vamd_decode_ogg_window).  Part of the library's
// single translation unit, after vamd_decode.h.  The host picks each window's blocks (vamd_decode_window_plan.h), gathers
// only what those blocks need into the context's pinned staging buffer -- their packets, or for files the pages they lie
// in -- and hands decode_run a plan whose "streams" are the windows: one upload, k_ogg_depage over the windows' page rows
// (files), k_unpack, k_synth, and k_lap_window in k_lap's place.  A block two windows share is unpacked once per window.
#pragma once
#include "vamd_decode_window_plan.h"

static int decode_window_plan(vamd_ctx *c, const vamd_decode_desc *d, int64_t nwindows, const int64_t *stream, const int64_t *start,
                              const int64_t *count, WindowPlan *WP) {
  DecodePlan whole;
  int r = decode_plan(c, d, nullptr, &whole);
  if (r) return r;
  std::string err;
  if (!window_plan_build(whole, c->B.bs, nwindows, stream, start, count, WP, &err)) return fail(c, VAMD_EINVAL, err.c_str());
  return VAMD_OK;
}

int vamd_decode_window_plan(vamd_ctx *c, const vamd_decode_desc *d, int64_t nwindows, const int64_t *stream, const int64_t *start,
                            const int64_t *count, int64_t *frames, int64_t *nblocks) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  WindowPlan WP;
  int r = decode_window_plan(c, d, nwindows, stream, start, count, &WP);
  if (r) return r;
  decode_report(WP.P, nwindows, frames, nblocks);
  return VAMD_OK;
}

// the windows' channel strides: the caller's, held against the frames, or the frames themselves
static int decode_window_strides(vamd_ctx *c, const WindowPlan &WP, const int64_t *channel_stride, std::vector<int64_t> *stride) {
  *stride = WP.P.frames;
  for (size_t w = 0; channel_stride && w < stride->size(); w++) {
    if (channel_stride[w] < WP.P.frames[w] || channel_stride[w] > ((int64_t)1 << 62)) return fail(c, VAMD_EINVAL, "decode_window: a channel stride below the window's frames");
    (*stride)[w] = channel_stride[w];
  }
  return VAMD_OK;
}

int vamd_decode_window(vamd_ctx *c, const vamd_decode_desc *d, int64_t nwindows, const int64_t *stream, const int64_t *start, const int64_t *count,
                       const int64_t *offset_out, float *pcm, uint8_t *status) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  WindowPlan WP;
  int r = decode_window_plan(c, d, nwindows, stream, start, count, &WP);
  if (r) return r;
  if ((r = decode_outputs(c, WP.P, nwindows, offset_out, pcm, status))) return r;
  if (WP.P.order.empty()) return VAMD_OK;
  std::vector<int64_t> offs, stride;
  if ((r = decode_window_strides(c, WP, nullptr, &stride))) return r;
  window_packet_layout(WP, d->offset, &offs);
  if ((r = pinned_get(c, c->dec.h_stage, (size_t)offs.back() + 16, true))) return r;
  window_packet_gather(WP, d->bytes, d->offset, offs, (uint8_t *)c->dec.h_stage.p);
  DecodeInput in;
  in.offset = offs.data(), in.byte0 = 0, in.nbytes = offs.back();
  in.packets = (const uint8_t *)c->dec.h_stage.p;
  DecodeAdds add;
  add.first = WP.first.data(), add.stride = stride.data();
  return decode_run(c, WP.P, nwindows, in, offset_out, pcm, status, add);
}

// ---- files: the seek index, then windows of the files it was made of ----
struct vamd_ogg_index {
  vamd_ctx *c = nullptr;
  OggIndex I;
};

int vamd_ogg_index_create(vamd_ctx *c, const vamd_decode_ogg_desc *d, vamd_ogg_index **out) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!out) return fail(c, VAMD_EINVAL, "ogg_index: null out");
  *out = nullptr;
  if (!d) return fail(c, VAMD_EINVAL, "ogg_index: null descriptor");
  int r = decode_ready(c);
  if (r) return r;
  vamd_ogg_index *x = new (std::nothrow) vamd_ogg_index;
  if (!x) return fail(c, VAMD_EFAULT, "ogg_index: out of memory");
  x->c = c;
  const DemuxSetup S = demux_setup(c, d->setup_header, d->setup_header_bytes);
  std::string err;
  if (!ogg_index_build(c->B.bs, c->dec.U.modes, c->dec.U.modebits, d->nstreams, d->bytes, d->file_offset, S, &x->I, &err)) {
    delete x;
    return fail(c, VAMD_EINVAL, err.c_str());
  }
  *out = x;
  return VAMD_OK;
}

void vamd_ogg_index_destroy(vamd_ogg_index *x) { delete x; }

int vamd_ogg_index_info(const vamd_ogg_index *x, int64_t *nstreams, int64_t *frames, uint8_t *status) {
  if (!x) return VAMD_EINVAL;
  const int64_t ns = (int64_t)x->I.file_bytes.size();
  if (nstreams) *nstreams = ns;
  for (int64_t s = 0; s < ns; s++) {
    if (frames) frames[s] = x->I.whole.frames[(size_t)s];
    if (status) status[s] = x->I.whole.status[(size_t)s];
  }
  return VAMD_OK;
}

static int decode_ogg_window_plan(vamd_ctx *c, const vamd_ogg_index *x, const vamd_ogg_window_desc *d, WindowPlan *WP, OggWindowStage *G) {
  if (!x) return fail(c, VAMD_EINVAL, "decode_ogg_window: null index");
  if (x->c != c) return fail(c, VAMD_EINVAL, "decode_ogg_window: the index is another context's");
  if (!d) return fail(c, VAMD_EINVAL, "decode_ogg_window: null descriptor");
  std::string err;
  if (!ogg_window_files_check(x->I, d->bytes, d->file_offset, &err)) return fail(c, VAMD_EINVAL, err.c_str());
  if (!window_plan_build(x->I.whole, c->B.bs, d->nwindows, d->stream, d->start, d->count, WP, &err)) return fail(c, VAMD_EINVAL, err.c_str());
  if (!ogg_window_stage(x->I, *WP, d->stream, G, &err)) return fail(c, VAMD_EINVAL, err.c_str());
  return VAMD_OK;
}

int vamd_decode_ogg_window_plan(vamd_ctx *c, const vamd_ogg_index *x, const vamd_ogg_window_desc *d, int64_t *frames, int64_t *nblocks, int64_t *staged) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  WindowPlan WP;
  OggWindowStage G;
  int r = decode_ogg_window_plan(c, x, d, &WP, &G);
  if (r) return r;
  decode_report(WP.P, d->nwindows, frames, nblocks);
  if (staged) staged[0] = G.stage_bytes, staged[1] = (int64_t)G.pages.size();
  return VAMD_OK;
}

int vamd_decode_ogg_window(vamd_ctx *c, const vamd_ogg_index *x, const vamd_ogg_window_desc *d, const int64_t *offset_out, float *pcm, uint8_t *status) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  WindowPlan WP;
  OggWindowStage G;
  std::vector<int64_t> stride;
  int r = decode_ogg_window_plan(c, x, d, &WP, &G);
  if (r) return r;
  if (d->channel_stride && c->dec.pcm_interleaved)  // (an interleaved window is one row: frame k's channels lie side by side)
    return fail(c, VAMD_EINVAL, "decode_ogg_window: channel_stride has no meaning under an interleaved output format (vamd_decode_output)");
  if ((r = decode_window_strides(c, WP, d->channel_stride, &stride))) return r;
  if ((r = decode_outputs(c, WP.P, d->nwindows, offset_out, pcm, status))) return r;
  if (WP.P.order.empty()) return VAMD_OK;
  if ((r = pinned_get(c, c->dec.h_stage, (size_t)G.stage_bytes + 16, true))) return r;
  ogg_window_gather(G, d->bytes, d->file_offset, (uint8_t *)c->dec.h_stage.p);
  DemuxScan rows;  // (decode_run reads the page table alone)
  rows.pages.swap(G.pages);
  DecodeInput in;
  in.offset = G.offs.data(), in.begin = G.begin.data(), in.byte0 = 0, in.nbytes = G.arena_bytes;
  in.scan = &rows, in.files = (const uint8_t *)c->dec.h_stage.p, in.files_bytes = G.stage_bytes;
  DecodeAdds add;
  add.first = WP.first.data(), add.stride = stride.data();
  return decode_run(c, WP.P, d->nwindows, in, offset_out, pcm, status, add);
}
