// vamd_decode_live.h -- the live decoder (include/vorbis_amd.h: vamd_decode_live_*): the next pieces of continuing streams,
// lists of audio packets in host memory, to PCM in device memory.  Part of the library's single translation unit, behind
// vamd_decode.h, whose workspace and launch sequence a call takes (decode_run).  What is carried between a stream's pieces
// is its last block's second half, on the device -- one buffer [max_streams][ch][bs[1]/2] -- and, on the host, that
// block's size class, the frames handed out and whether the stream is dead (vamd_decode_live_plan.h: LiveSlot).  A call
// plans on the host, runs, and commits the slots only once it has succeeded.
#pragma once

struct vamd_decode_live {
  vamd_ctx *c = nullptr;
  std::vector<LiveSlot> slots;
  float *carry = nullptr;
};

int vamd_decode_live_create(vamd_ctx *c, int64_t max_streams, vamd_decode_live **out) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!out) return fail(c, VAMD_EINVAL, "decode_live: null out");
  *out = nullptr;
  if (max_streams < 1 || max_streams > (1 << 20)) return fail(c, VAMD_EINVAL, "decode_live: max_streams outside 1 .. 2^20");
  int r = decode_ready(c);
  if (r) return r;
  if (c->B.bs[1] < c->B.bs[0]) return fail(c, VAMD_EIMPL, "decode_live: a long block shorter than the short one");
  vamd_decode_live *d = new (std::nothrow) vamd_decode_live;
  if (!d) return fail(c, VAMD_EFAULT, "decode_live: out of memory");
  d->c = c;
  d->slots.assign((size_t)max_streams, LiveSlot());
  const size_t bytes = (size_t)max_streams * c->B.channels * (c->B.bs[1] / 2) * 4;
  hipError_t e = hipMalloc((void **)&d->carry, bytes);
  if (e == hipSuccess) e = hipMemset(d->carry, 0, bytes);
  if (e != hipSuccess) {
    if (d->carry) (void)hipFree(d->carry);
    delete d;
    return fail(c, VAMD_EFAULT, "decode_live: the carries", e);
  }
  *out = d;
  return VAMD_OK;
}

void vamd_decode_live_destroy(vamd_decode_live *d) {
  if (!d) return;
  DeviceGuard dev_guard(d->c);
  if (d->carry) (void)hipFree(d->carry);
  delete d;
}

static int decode_live_plan(vamd_decode_live *d, const vamd_decode_live_desc *desc, DecodeLivePlan *L) {
  vamd_ctx *c = d->c;
  if (!desc) return fail(c, VAMD_EINVAL, "decode_live: null descriptor");
  int r = decode_ready(c);
  if (r) return r;
  std::string err;
  if (!decode_live_plan_build(c->B.bs, c->dec.U.modes, c->dec.U.modebits, d->slots, desc->nstreams, desc->npackets, desc->slot, desc->bytes, desc->offset,
                              desc->stream_start, desc->close, desc->end_granule, L, &err))
    return fail(c, VAMD_EINVAL, err.c_str());
  return VAMD_OK;
}

int vamd_decode_live_plan(vamd_decode_live *d, const vamd_decode_live_desc *desc, int64_t *frames, int64_t *nblocks) {
  if (!d) return VAMD_EINVAL;
  DeviceGuard dev_guard(d->c);
  DecodeLivePlan L;
  int r = decode_live_plan(d, desc, &L);
  if (r) return r;
  for (int64_t s = 0; frames && s < desc->nstreams; s++) frames[s] = L.P.frames[(size_t)s];
  if (nblocks) nblocks[0] = L.P.nblocks[0], nblocks[1] = L.P.nblocks[1];
  return VAMD_OK;
}

int vamd_decode_live_wrote(vamd_decode_live *d, const vamd_decode_live_desc *desc, const int64_t *offset_out, float *pcm, uint8_t *status) {
  if (!d) return VAMD_EINVAL;
  vamd_ctx *c = d->c;
  DeviceGuard dev_guard(c);
  DecodeLivePlan L;
  int r = decode_live_plan(d, desc, &L);
  if (r) return r;
  if ((r = decode_outputs(c, L.P, desc->nstreams, offset_out, pcm, status))) return r;
  if (!L.unpack.empty()) {
    DecodeInput in;
    in.offset = desc->offset, in.byte0 = desc->offset[0], in.nbytes = desc->offset[desc->npackets] - desc->offset[0];
    in.packets = desc->bytes + in.byte0;
    DecodeCarry live;
    live.plan = &L, live.carry = d->carry;
    if ((r = decode_run(c, L.P, desc->nstreams, in, offset_out, pcm, status, &live))) return r;
  }
  decode_live_commit(&d->slots, L, desc->nstreams, desc->slot, desc->close, status);
  return VAMD_OK;
}
