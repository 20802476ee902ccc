// vamd_decode_ogg_live.h -- the live Ogg decoder (include/vorbis_amd.h: vamd_decode_ogg_live_*): the next BYTES of continuing
// Ogg Vorbis streams, in host memory and cut anywhere, to PCM in device memory.  Part of the library's single translation
// unit, behind vamd_decode_live.h.  It joins the two entries in front of it: the host's page walk with its state per slot
// (vamd_demux_live.h) in place of vamd_demux.h's walk of a whole file, and the live packet decoder's slots and float carry
// (vamd_decode_live_plan.h) behind it -- one call of decode_run with both DecodeInput::scan and DecodeAdds::live.  What the object
// adds to those is a byte carry on the device, [max_streams][max_packet_bytes rounded up to 4]: the audio packet that a
// slot's whole pages have left open (k_ogg_packet_carry_in / _out, k_demux.h).
// A call's whole pages are gathered on the host -- the held tail and the piece, stream after stream, into one staging
// vector -- and go up in ONE copy, as the whole-file entry's files do.
#pragma once

struct vamd_decode_ogg_live {
  vamd_ctx *c = nullptr;
  LiveLap lap;                       // the blocks' side: the lap carried between pieces
  std::vector<DemuxLiveSlot> demux;  // the container's side
  uint8_t *bytes_carry = nullptr;
  int64_t max_packet_bytes = 0, max_header_bytes = 0, stride = 0;
  std::vector<uint8_t> setup_header;
  bool has_setup_header = false;
};

int vamd_decode_ogg_live_create(vamd_ctx *c, int64_t max_streams, const vamd_decode_ogg_live_opts *opts, vamd_decode_ogg_live **out) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!out) return fail(c, VAMD_EINVAL, "decode_ogg_live: null out");
  *out = nullptr;
  int r = LiveLap::streams(c, "decode_ogg_live", max_streams);
  if (r) return r;
  if (opts && (opts->setup_header_bytes < 0 || (opts->setup_header_bytes > 0 && !opts->setup_header)))
    return fail(c, VAMD_EINVAL, "decode_ogg_live: setup_header_bytes without a setup header");
  if (opts && (opts->max_packet_bytes < 0 || opts->max_packet_bytes > (1 << 24))) return fail(c, VAMD_EINVAL, "decode_ogg_live: max_packet_bytes outside 0 .. 2^24");
  if (opts && (opts->max_header_bytes < 0 || opts->max_header_bytes > ((int64_t)1 << 30))) return fail(c, VAMD_EINVAL, "decode_ogg_live: max_header_bytes outside 0 .. 2^30");
  if ((r = LiveLap::ready(c, "decode_ogg_live"))) return r;
  vamd_decode_ogg_live *d = new (std::nothrow) vamd_decode_ogg_live;
  if (!d) return fail(c, VAMD_EFAULT, "decode_ogg_live: out of memory");
  d->c = c;
  d->demux.assign((size_t)max_streams, DemuxLiveSlot());
  d->max_packet_bytes = opts && opts->max_packet_bytes ? opts->max_packet_bytes : std::max(vamd_packet_capacity(c, 0), vamd_packet_capacity(c, 1));
  d->max_header_bytes = opts && opts->max_header_bytes ? opts->max_header_bytes : (int64_t)1 << 20;
  d->stride = (d->max_packet_bytes + 3) & ~(int64_t)3;
  if (opts && opts->setup_header) d->setup_header.assign(opts->setup_header, opts->setup_header + opts->setup_header_bytes), d->has_setup_header = true;
  if ((uint64_t)max_streams * (uint64_t)d->stride > ((uint64_t)1 << 36)) {
    delete d;
    return fail(c, VAMD_EINVAL, "decode_ogg_live: more than 2^36 bytes of packet carry");
  }
  if ((r = d->lap.make(c, "decode_ogg_live", max_streams))) {
    delete d;
    return r;
  }
  const hipError_t e = LiveLap::zeros((void **)&d->bytes_carry, (size_t)max_streams * (size_t)d->stride + 16);
  if (e != hipSuccess) {
    vamd_decode_ogg_live_destroy(d);
    return fail(c, VAMD_EFAULT, "decode_ogg_live: the carries", e);
  }
  *out = d;
  return VAMD_OK;
}

void vamd_decode_ogg_live_destroy(vamd_decode_ogg_live *d) {
  if (!d) return;
  DeviceGuard dev_guard(d->c);
  d->lap.release();
  if (d->bytes_carry) (void)hipFree(d->bytes_carry);
  delete d;
}

// The host's walk of the pieces, then the live block plan over its packet table with the first bytes it kept in place.
static int decode_ogg_live_plan(vamd_decode_ogg_live *d, const vamd_decode_ogg_live_desc *desc, DemuxLiveCall *X, DecodeLivePlan *L) {
  vamd_ctx *c = d->c;
  if (!desc) return fail(c, VAMD_EINVAL, "decode_ogg_live: null descriptor");
  int r = decode_ready(c);
  if (r) return r;
  const DemuxSetup S = demux_setup(c, d->has_setup_header ? d->setup_header.data() : nullptr, (int64_t)d->setup_header.size());
  std::string err;
  if (!demux_live_scan(d->demux, desc->nstreams, desc->slot, desc->bytes, desc->piece_offset, desc->close, S, d->max_packet_bytes, d->max_header_bytes, X, &err))
    return fail(c, VAMD_EINVAL, err.c_str());
  if (!decode_live_plan_build(c->B.bs, c->dec.U.modes, c->dec.U.modebits, d->lap.slots, desc->nstreams, (int64_t)X->X.first.size(), desc->slot, nullptr,
                              X->X.offset.data(), X->X.stream_start.data(), X->close.data(), X->X.end_granule.data(), L, &err, X->X.first.data()))
    return fail(c, VAMD_EINVAL, err.c_str());
  for (int64_t s = 0; s < desc->nstreams; s++) L->P.status[(size_t)s] |= X->X.status[(size_t)s];
  return VAMD_OK;
}

int vamd_decode_ogg_live_plan(vamd_decode_ogg_live *d, const vamd_decode_ogg_live_desc *desc, int64_t *frames, int64_t *nblocks) {
  if (!d) return VAMD_EINVAL;
  DeviceGuard dev_guard(d->c);
  DemuxLiveCall X;
  DecodeLivePlan L;
  int r = decode_ogg_live_plan(d, desc, &X, &L);
  if (r) return r;
  decode_report(L.P, desc->nstreams, frames, nblocks);
  return VAMD_OK;
}

int vamd_decode_ogg_live_wrote(vamd_decode_ogg_live *d, const vamd_decode_ogg_live_desc *desc, const int64_t *offset_out, float *pcm, uint8_t *status) {
  if (!d) return VAMD_EINVAL;
  vamd_ctx *c = d->c;
  DeviceGuard dev_guard(c);
  DemuxLiveCall X;
  DecodeLivePlan L;
  int r = decode_ogg_live_plan(d, desc, &X, &L);
  if (r) return r;
  if ((r = decode_outputs(c, L.P, desc->nstreams, offset_out, pcm, status))) return r;
  if (!L.unpack.empty() || !X.X.pages.empty()) {
    DecodeInput in;
    in.offset = X.X.offset.data(), in.begin = X.begin.data(), in.byte0 = 0, in.nbytes = X.arena_bytes;
    in.scan = &X.X, in.files = X.upload.data(), in.files_bytes = (int64_t)X.upload.size();
    DecodeAdds add;
    add.live = &L, add.carry = d->lap.carry;
    add.bytes_in = &X.in, add.bytes_out = &X.out, add.bytes_carry = d->bytes_carry, add.slots = (int64_t)d->demux.size(), add.bytes_stride = d->stride;
    if ((r = decode_run(c, L.P, desc->nstreams, in, offset_out, pcm, status, add))) return r;
  }
  decode_live_commit(&d->lap.slots, L, desc->nstreams, desc->slot, X.close.data(), status);
  demux_live_commit(&d->demux, &X, desc->nstreams, desc->slot, desc->close, status);
  return VAMD_OK;
}
