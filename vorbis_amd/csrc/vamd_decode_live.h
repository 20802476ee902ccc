// vamd_decode_live.h -- the live decoder (include/vorbis_amd.h: vamd_decode_live_*): the next pieces of continuing streams,
// lists of audio packets in host memory, to PCM in device memory.  Part of the library's single translation unit, behind
// vamd_decode.h, whose workspace and launch sequence a call takes (decode_run).  What is carried between a stream's pieces
// is its last block's second half, on the device -- one buffer [max_streams][ch][bs[1]/2] -- and, on the host, that
// block's size class, the frames handed out and whether the stream is dead (vamd_decode_live_plan.h: LiveSlot).  A call
// plans on the host, runs, and commits the slots only once it has succeeded.
#pragma once

// What both live decoders carry of the blocks between a stream's pieces: the slots on the host, the last blocks' second
// halves on the device.  `name` is the call's, in front of its texts.
struct LiveLap {
  std::vector<LiveSlot> slots;
  float *carry = nullptr;

  static std::string text(const char *name, const char *what) { return std::string(name) + ": " + what; }
  // what a _create asks of its stream count, and then -- behind its own checks -- of the context
  static int streams(vamd_ctx *c, const char *name, int64_t max_streams) {
    if (max_streams < 1 || max_streams > (1 << 20)) return fail(c, VAMD_EINVAL, text(name, "max_streams outside 1 .. 2^20").c_str());
    return VAMD_OK;
  }
  static int ready(vamd_ctx *c, const char *name) {
    int r = decode_ready(c);
    if (r) return r;
    if (c->B.bs[1] < c->B.bs[0]) return fail(c, VAMD_EIMPL, text(name, "a long block shorter than the short one").c_str());
    return VAMD_OK;
  }
  // a device buffer of `bytes` zeros; on failure *p is what was allocated, the caller's to free
  static hipError_t zeros(void **p, size_t bytes) {
    const hipError_t e = hipMalloc(p, bytes);
    return e == hipSuccess ? hipMemset(*p, 0, bytes) : e;
  }
  // the slots, and the carry allocated and zeroed; on failure nothing is held
  int make(vamd_ctx *c, const char *name, int64_t max_streams) {
    slots.assign((size_t)max_streams, LiveSlot());
    const hipError_t e = zeros((void **)&carry, (size_t)max_streams * c->B.channels * (c->B.bs[1] / 2) * 4);
    if (e == hipSuccess) return VAMD_OK;
    release();
    return fail(c, VAMD_EFAULT, text(name, "the carries").c_str(), e);
  }
  void release() {
    if (carry) (void)hipFree(carry);
    carry = nullptr;
  }
};

struct vamd_decode_live {
  vamd_ctx *c = nullptr;
  LiveLap lap;
};

int vamd_decode_live_create(vamd_ctx *c, int64_t max_streams, vamd_decode_live **out) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!out) return fail(c, VAMD_EINVAL, "decode_live: null out");
  *out = nullptr;
  int r = LiveLap::streams(c, "decode_live", max_streams);
  if (r) return r;
  if ((r = LiveLap::ready(c, "decode_live"))) return r;
  vamd_decode_live *d = new (std::nothrow) vamd_decode_live;
  if (!d) return fail(c, VAMD_EFAULT, "decode_live: out of memory");
  d->c = c;
  if ((r = d->lap.make(c, "decode_live", max_streams))) {
    delete d;
    return r;
  }
  *out = d;
  return VAMD_OK;
}

void vamd_decode_live_destroy(vamd_decode_live *d) {
  if (!d) return;
  DeviceGuard dev_guard(d->c);
  d->lap.release();
  delete d;
}

static int decode_live_plan(vamd_decode_live *d, const vamd_decode_live_desc *desc, DecodeLivePlan *L) {
  vamd_ctx *c = d->c;
  if (!desc) return fail(c, VAMD_EINVAL, "decode_live: null descriptor");
  int r = decode_ready(c);
  if (r) return r;
  std::string err;
  if (!decode_live_plan_build(c->B.bs, c->dec.U.modes, c->dec.U.modebits, d->lap.slots, desc->nstreams, desc->npackets, desc->slot, desc->bytes, desc->offset,
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
  decode_report(L.P, desc->nstreams, frames, nblocks);
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
    DecodeAdds add;
    add.live = &L, add.carry = d->lap.carry;
    if ((r = decode_run(c, L.P, desc->nstreams, decode_input_packets(desc->bytes, desc->offset, desc->npackets), offset_out, pcm, status, add))) return r;
  }
  decode_live_commit(&d->lap.slots, L, desc->nstreams, desc->slot, desc->close, status);
  return VAMD_OK;
}
