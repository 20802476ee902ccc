// vamd_plan.h -- stream planning on the device: the block-switch detector over batches of streams, the walk that turns
// its flags into blocks (whole streams, streams of unequal length, the live feed's continuing ones), the plan's arrays,
// gather and fetch.  Part of the library's single translation unit: included by vamd_hip.hip, once, after vamd_batch.h.
#pragma once
// `bad`: the word (device) that counts detector steps outside the input domain
// count_of / first_of (device, optional): streams of unequal length in one launch -- stream s takes its first count_of[s] steps
// only (its state is left after exactly those), and its first step starts first_of[s] samples into its buffer
static int envelope_search_batch(vamd_ctx *c, const float *pcm, long stream_stride, long channel_stride, long nstreams,
                                 long nsteps, vamd_envelope_state *states, unsigned char *ret, unsigned int *bad,
                                 const int *count_of = nullptr, const long long *first_of = nullptr) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (nstreams < 0 || nsteps < 0) return fail(c, VAMD_EINVAL, "negative stream / step count");
  if (nstreams == 0 || nsteps == 0) return VAMD_OK;
  if (!pcm || !states || !ret) return fail(c, VAMD_EINVAL, "null pcm / states / ret");
  const EnvP &E = c->B.env;
  const int ch = c->B.channels, n = E.mdct.n, n2 = n / 2;
  const long nsc = nstreams * ch;
  void *v_near, *v_raw, *v_amp, *v_bits;
  int r;
  if ((r = ws_get(c, 0, vamd_ctx::WS_ENV_NEAR, (size_t)nsc * (VAMD_VE_NEAR_HIST + nsteps) * 4, &v_near))) return r;
  if ((r = ws_get(c, 0, vamd_ctx::WS_ENV_RAW, (size_t)nsc * nsteps * VAMD_VE_SPREAD * 4, &v_raw))) return r;
  if ((r = ws_get(c, 0, vamd_ctx::WS_ENV_AMP, (size_t)nsc * (VAMD_VE_AMP_HIST + nsteps) * 8 * 4, &v_amp))) return r;
  if ((r = ws_get(c, 0, vamd_ctx::WS_ENV_BITS, (size_t)nstreams * nsteps * 4, &v_bits))) return r;
  float *near = (float *)v_near, *raw = (float *)v_raw, *amp = (float *)v_amp;
  uint32_t *bits = (uint32_t *)v_bits;
  hipStream_t s = c->stream;
  {
    const long t = nsc * (VAMD_VE_NEAR_HIST + VAMD_VE_AMP_HIST * 8);
    hipLaunchKernelGGL(k_env_prolog, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, ch, nstreams, nsteps, states,
                       near, amp);
  }
  {
    const long items = nsc * ((nsteps + VAMD_ENV_STEPS - 1) / VAMD_ENV_STEPS);
    if (items > 0x7fffffffL) return fail(c, VAMD_EINVAL, "detector: more than 2^31 groups of steps in one call");
    const long groups = (items + VAMD_ENV_WAVES - 1) / VAMD_ENV_WAVES;
    const size_t lds = ((size_t)VAMD_ENV_WAVES * (2 * VAMD_ENV_STAGE_FLOATS + VAMD_ENV_STEPS * (n2 + VAMD_PW_SIZE(n2))) + (n + n / 4) + n + n / 4) * 4;  // + the transform's tables
    const unsigned grid = persistent_grid(c, (const void *)k_env_spectrum, 64 * VAMD_ENV_WAVES, lds, groups);
    hipLaunchKernelGGL(k_env_spectrum, dim3(grid), dim3(64 * VAMD_ENV_WAVES), lds, s, E,
                       ch, nstreams, nsteps, pcm, stream_stride, channel_stride, near, raw, bad, first_of, c->d_dbg);
  }
  const bool env_untiled = c->K.env_untiled;  // (measurement aid: the thread-per-item forms)
  const bool big = nstreams * nsteps > 65536 && !env_untiled;
  if (big) {
    const long tiles = (nsteps + VAMD_ENV_TJ - 1) / VAMD_ENV_TJ;
    hipLaunchKernelGGL(k_env_amp_tiled, dim3((unsigned)(nsc * tiles)), dim3(8 * VAMD_ENV_TJ), 0, s, E, nsc, nsteps, states, ch,
                       near, raw, amp);
  } else {
    const long t = nsc * nsteps * 8;
    hipLaunchKernelGGL(k_env_amp, dim3((unsigned)((t + 255) / 256)), dim3(256), 0, s, E, nsc, nsteps, states, ch,
                       near, raw, amp);
  }
  if (nstreams * nsteps <= 65536)
    hipLaunchKernelGGL(k_env_bits, dim3((unsigned)((nstreams * nsteps * 16 + 255) / 256)), dim3(256), 0, s, E, ch, nstreams, nsteps,
                       amp, bits);
  else if (!env_untiled && (size_t)4 * ch * VAMD_ENV_BROWS * 9 * 4 <= c->lds_per_block) {  // (the tile of 7.1 wants 88.7 KB: a part
    // with 64 KB of LDS per workgroup takes the thread-per-step form below instead of failing the launch)
    const long items = nstreams * ((nsteps + 63) / 64);
    hipLaunchKernelGGL(k_env_bits_tiled, dim3((unsigned)((items + 3) / 4)), dim3(256), (size_t)4 * ch * VAMD_ENV_BROWS * 9 * 4, s, E, ch,
                       nstreams, nsteps, amp, bits);
  } else
    hipLaunchKernelGGL(k_env_bits_batch, dim3((unsigned)((nstreams * nsteps + 255) / 256)), dim3(256), 0, s, E, ch, nstreams,
                       nsteps, amp, bits);
  hipLaunchKernelGGL(k_env_walk, dim3((unsigned)nstreams), dim3(64), 0, s, ch, nstreams, nsteps, bits, near, amp,
                     states, ret, count_of);
  HIP_TRY(c, hipGetLastError());
  return VAMD_OK;
}

int vamd_envelope_search_batch(vamd_ctx *c, const float *pcm, long stream_stride, long channel_stride, long nstreams,
                               long nsteps, vamd_envelope_state *states, unsigned char *ret) {
  VAMD_NEEDS_ENCODER(c);
  return envelope_search_batch(c, pcm, stream_stride, channel_stride, nstreams, nsteps, states, ret, c ? c->d_bad + 1 : nullptr);
}

// ---- what plan_streams and vamd_live_plan (vamd_live.h; vamd_feed.hip is its caller) share ----
static long live_n_head(const vamd_ctx *c, int write_frames) { return ((long)c->B.bs[1] / write_frames + 1) * write_frames; }  // lib/block.c:525-526

// the walk's parameters for buffers of `nsamples` per channel, a stream's row of blocks sized for `room` samples
static BlockoutP blockout_params(const vamd_ctx *c, long nsamples, long room) {
  BlockoutP B;
  B.bs[0] = c->B.bs[0];
  B.bs[1] = c->B.bs[1];
  blockout_set_step(B, c->B.env.searchstep);
  B.nsamples = nsamples;
  B.eof = 0;
  B.nsteps = 0;
  B.maxblocks = (int)(room / (B.bs[0] / 2)) + 2;  // a block advances the stream by at least blocksizes[0]/2
  return B;
}

// the LDS of the two extrapolations at a stream's ends (k_lpc_head over its first n_head frames, k_lpc_tail), and the
// opt-in they need above the default 64 KB of dynamic LDS
static size_t lpc_lds(const vamd_ctx *c, long n_head) {
  const long bs1 = c->B.bs[1], head = bs1 / 2, pad = 3 * bs1, n = n_head + head;
  return 80 * 8 + VAMD_LPC_MAX_ORDER * 4 + (size_t)(n > bs1 + pad ? n : bs1 + pad) * 4;
}
static int lpc_opt_in(vamd_ctx *c) {
  HIP_TRY(c, hipFuncSetAttribute((const void *)k_lpc_head, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_per_block));
  HIP_TRY(c, hipFuncSetAttribute((const void *)k_lpc_tail, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_per_block));
  return VAMD_OK;
}

// a plan's workspace: `flag_bytes` of detector flags, a row of `maxblocks` blocks per stream, the counts, the bases, and
// where every stream's walk stands when its data runs out
struct PlanWs {
  void *flags, *blocks, *counts, *base, *pending;
};
static int plan_ws(vamd_ctx *c, long nstreams, size_t flag_bytes, int maxblocks, PlanWs *w) {
  int r;
  if ((r = ws_get(c, 0, vamd_ctx::WS_PLAN_FLAGS, flag_bytes, &w->flags))) return r;
  if ((r = ws_get(c, 0, vamd_ctx::WS_PLAN_BLOCKS, (size_t)nstreams * maxblocks * sizeof(PlannedBlock), &w->blocks))) return r;
  if ((r = ws_get(c, 0, vamd_ctx::WS_PLAN_COUNTS, (size_t)nstreams * 2 * sizeof(int), &w->counts))) return r;
  if ((r = ws_get(c, 0, vamd_ctx::WS_PLAN_BASE, (size_t)(3 * nstreams + 1) * sizeof(long long), &w->base))) return r;
  return ws_get(c, 0, vamd_ctx::WS_PLAN_PENDING, (size_t)nstreams * sizeof(long long), &w->pending);
}

// The walk's blocks of every stream -> the plan's per-class arrays and order[]: the block counts come home (the plan's one
// wait; `extra_bytes` more of the device's `extra_dev` beside them, into `extra_host`), the bases go up, k_plan_emit lays
// the blocks out.  (The tail of plan_streams and of vamd_live_plan.)
static int plan_emit(vamd_ctx *c, const BlockoutP &B, long nstreams, long stream_stride, const PlanWs &ws, vamd_stream_plan *plan,
                     void *extra_host = nullptr, const void *extra_dev = nullptr, size_t extra_bytes = 0) {
  void *v_blocks = ws.blocks, *v_counts = ws.counts, *v_base = ws.base;
  hipStream_t s = c->stream;
  int r;
  std::vector<int> counts((size_t)nstreams * 2);
  HIP_TRY(c, hipMemcpyAsync(counts.data(), v_counts, counts.size() * sizeof(int), hipMemcpyDeviceToHost, s));
  if (extra_bytes) HIP_TRY(c, hipMemcpyAsync(extra_host, extra_dev, extra_bytes, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  for (long i = 0; i < nstreams; i++)
    if (counts[2 * i] < 0 || counts[2 * i + 1] < 0 || (long)counts[2 * i] + counts[2 * i + 1] > B.maxblocks)
      return fail(c, VAMD_EFAULT, "stream plan: a block count outside its bound (the planning kernel did not run to completion)");
  // [2s + W] then start[nstreams + 1]; pinned and the context's own, so that its upload needs no wait: the next plan on this
  // context cannot write it before its own count read-back, which is queued behind the upload, has come home
  const size_t base_bytes = ((size_t)3 * nstreams + 1) * sizeof(long long);
  if ((r = pinned_get(c, c->h_plan, base_bytes, false))) return r;
  long long *base = (long long *)c->h_plan.p;
  long long tot[2] = {0, 0}, all = 0;
  for (long i = 0; i < nstreams; i++) {
    base[2 * i] = tot[0];
    base[2 * i + 1] = tot[1];
    base[2 * nstreams + i] = all;
    tot[0] += counts[2 * i];
    tot[1] += counts[2 * i + 1];
    all += counts[2 * i] + counts[2 * i + 1];
  }
  base[3 * nstreams] = all;
  if (tot[0] > 0x3fffffffLL || tot[1] > 0x3fffffffLL) return fail(c, VAMD_EINVAL, "plan too large: order[] holds 30-bit indices");
  HIP_TRY(c, hipMemcpyAsync(v_base, base, base_bytes, hipMemcpyHostToDevice, s));
  // descriptor arrays: per class lW, nW, blocktype (int32) and src (int64); then order
  void *v_desc, *v_order;
  const size_t per[2] = {(size_t)tot[0], (size_t)tot[1]};
  const size_t desc_bytes = (per[0] + per[1]) * (3 * sizeof(int) + sizeof(long long)) + 64;
  if ((r = ws_get(c, 0, vamd_ctx::WS_PLAN_DESC, desc_bytes, &v_desc))) return r;
  if ((r = ws_get(c, 0, vamd_ctx::WS_PLAN_ORDER, (size_t)(all ? all : 1) * sizeof(int), &v_order))) return r;
  PlanOut O;
  long long *p64 = (long long *)v_desc;  // the 8-byte arrays first (alignment)
  O.src[0] = p64;
  O.src[1] = p64 + per[0];
  int *p32 = (int *)(p64 + per[0] + per[1]);
  for (int W = 0; W < 2; W++) {
    O.lW[W] = p32, p32 += per[W];
    O.nW[W] = p32, p32 += per[W];
    O.bt[W] = p32, p32 += per[W];
  }
  O.order = (int *)v_order;
  hipLaunchKernelGGL(k_plan_emit, dim3((unsigned)nstreams), dim3(64), 0, s, B, nstreams, stream_stride,
                     (const PlannedBlock *)v_blocks, (const int *)v_counts, (const long long *)v_base,
                     (const long long *)v_base + 2 * nstreams, O);
  HIP_TRY(c, hipGetLastError());
  for (int W = 0; W < 2; W++) {
    plan->nblocks[W] = tot[W];
    plan->lW[W] = O.lW[W];
    plan->nW[W] = O.nW[W];
    plan->blocktype[W] = O.bt[W];
    plan->src[W] = (const int64_t *)O.src[W];
  }
  plan->order = O.order;
  plan->stream_start = (const int64_t *)((const long long *)v_base + 2 * nstreams);
  return VAMD_OK;
}

// whole != 0: the streams are complete (vamd_plan_streams_whole) -- `nsamples` counts the space in front of the first
// sample and the real samples; the buffers have room for the end-of-stream padding behind them
// frames_of (host, whole streams only): the streams' own lengths, each <= nsamples - blocksizes[1]/2
static int plan_streams(vamd_ctx *c, float *pcm, long stream_stride, long channel_stride, long nstreams, long nsamples,
                        vamd_envelope_state *states, vamd_stream_plan *plan, int whole, const int64_t *frames_of = nullptr) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!plan) return fail(c, VAMD_EINVAL, "null plan");
  memset(plan, 0, sizeof(*plan));
  if (nstreams < 0 || nsamples < 0) return fail(c, VAMD_EINVAL, "negative stream / sample count");
  if (nstreams == 0) return VAMD_OK;
  if (!pcm || !states) return fail(c, VAMD_EINVAL, "null pcm / states");
  if ((stream_stride | channel_stride) & 3) return fail(c, VAMD_EINVAL, "stream / channel strides must be multiples of 4 samples");
  if (nstreams > 0x3fffffffL || nsamples > 0x3fffffffL) return fail(c, VAMD_EINVAL, "too many streams / samples for one plan");
  const EnvP &E = c->B.env;
  const int ch = c->B.channels, head = c->B.bs[1] / 2, pad = whole ? 3 * c->B.bs[1] : 0;
  if (whole && (nsamples < head || channel_stride < nsamples + pad))
    return fail(c, VAMD_EINVAL, "whole streams: a channel needs blocksizes[1]/2 samples of room in front and 3 * blocksizes[1] behind its samples");
  BlockoutP B = blockout_params(c, nsamples, nsamples + pad);
  // the steps _ve_envelope_search takes with this much data (lib/envelope.c:223-224); a whole stream's padding adds
  // pad / searchstep more, taken in a second pass once the padding exists
  long steps1 = nsamples / E.searchstep - VAMD_VE_WIN;
  if (steps1 < 0) steps1 = 0;
  long steps_all = (nsamples + pad) / E.searchstep - VAMD_VE_WIN;
  if (steps_all < 0) steps_all = 0;
  B.nsteps = steps1;
  plan->nstreams = nstreams;
  PlanWs ws;
  int r;
  if ((r = plan_ws(c, nstreams, (size_t)nstreams * (steps_all ? steps_all : 1), B.maxblocks, &ws))) return r;
  hipStream_t s = c->stream;
  // the walk's LDS: a window of marks (MarkWindow), the whole of a stream that is shorter.  The default fits the 64 KB of
  // dynamic LDS a launch gets without an opt-in; a window from the test knob is held to what a workgroup has.
  long window = plan_window_clamp(B, c->K.plan_window > 0 ? c->K.plan_window : VAMD_PLAN_WINDOW_DEFAULT);
  if (window > 65536) window = 65536;
  if (window > steps_all + 4) window = steps_all + 4;
  const size_t plan_lds = (size_t)((window + 15) & ~15L);
  unsigned char *flags1 = (unsigned char *)ws.flags, *flags2 = flags1 + (size_t)nstreams * steps1;
  const PlanGeo *geo = nullptr;      // streams of unequal length: their own sample counts, step counts and first padding steps
  const int *count1 = nullptr, *count2 = nullptr;
  const long long *first2 = nullptr;
  long steps2 = steps_all - steps1;  // steps of the second detector pass (the launch's: the longest stream's)
  if (whole && frames_of) {
    // [geo | count1 | count2 | first2] built on the host (a few words per stream) in a pinned buffer of the context's, one upload
    const size_t o_c1 = (size_t)nstreams * sizeof(PlanGeo), o_c2 = o_c1 + (size_t)nstreams * 4, o_f2 = (o_c2 + (size_t)nstreams * 4 + 7) & ~(size_t)7,
                 total = o_f2 + (size_t)nstreams * 8;
    if ((r = pinned_get(c, c->h_geo, total, true))) return r;
    void *v_geo;
    if ((r = ws_get(c, 0, vamd_ctx::WS_PLAN_GEO, total, &v_geo))) return r;
    // (the previous plan's upload out of this buffer has long been consumed: every plan ends with a stream synchronisation)
    unsigned char *hg = (unsigned char *)c->h_geo.p;
    PlanGeo *g = (PlanGeo *)hg;
    int *c1 = (int *)(hg + o_c1), *c2 = (int *)(hg + o_c2);
    long long *f2 = (long long *)(hg + o_f2);
    steps2 = 0;
    for (long i = 0; i < nstreams; i++) {
      const long fr = (long)frames_of[i];
      if (fr < 1 || head + fr > nsamples) return fail(c, VAMD_EINVAL, "whole streams: a stream's length must be 1 .. the launch's frame count");
      long s1 = (head + fr) / E.searchstep - VAMD_VE_WIN, sa = (head + fr + pad) / E.searchstep - VAMD_VE_WIN;
      if (s1 < 0) s1 = 0;
      if (sa < s1) sa = s1;
      g[i].nsamples = head + fr + pad, g[i].eof = head + fr, g[i].nsteps = (int)sa, g[i].split = (int)s1;
      c1[i] = (int)s1, c2[i] = (int)(sa - s1), f2[i] = (long long)s1 * E.searchstep;
      if (sa - s1 > steps2) steps2 = sa - s1;
    }
    HIP_TRY(c, hipMemcpyAsync(v_geo, hg, total, hipMemcpyHostToDevice, s));
    geo = (const PlanGeo *)v_geo;
    count1 = (const int *)((unsigned char *)v_geo + o_c1), count2 = (const int *)((unsigned char *)v_geo + o_c2);
    first2 = (const long long *)((unsigned char *)v_geo + o_f2);
    // flags2's rows are steps2 long; the flag buffer was sized for steps_all per stream: steps1 + steps2 may exceed it by VE_WIN
    if ((r = ws_get(c, 0, vamd_ctx::WS_PLAN_FLAGS, (size_t)nstreams * (steps1 + steps2 + 1), &ws.flags))) return r;
    flags1 = (unsigned char *)ws.flags, flags2 = flags1 + (size_t)nstreams * steps1;
  }
  if (whole) {
    // the start of a stream as the example's 1024-sample writes make it (lib/block.c:524-528: the helper runs after the
    // first write that leaves more than blocksizes[1] samples beyond the centre, or when the stream is closed)
    const long frames = nsamples - head;
    long n_head = live_n_head(c, 1024);
    if (frames < n_head) n_head = frames;
    const size_t lds_lpc = lpc_lds(c, n_head);
    if (lds_lpc > c->lds_per_block) return fail(c, VAMD_EIMPL, "block size too large for the stream-end extrapolation");
    if ((r = lpc_opt_in(c))) return r;
    if (n_head > 32)
      hipLaunchKernelGGL(k_lpc_head, dim3((unsigned)(nstreams * ch)), dim3(64), lds_lpc, s, ch, nstreams, pcm, stream_stride,
                         channel_stride, head, (int)n_head, geo);
    if (steps1 && (r = envelope_search_batch(c, pcm, stream_stride, channel_stride, nstreams, steps1, states, flags1, c->d_bad + 1, count1)))
      return r;
    // where every stream's walk stands when the data runs out: the reference's buffer begins blocksizes[1]/2 before it
    hipLaunchKernelGGL(k_plan_streams, dim3((unsigned)nstreams), dim3(64), plan_lds, s, B, nstreams, flags1, steps1, steps1, flags2, steps2,
                       (PlannedBlock *)nullptr, (int *)nullptr, (long long *)ws.pending, geo, 0, window);
    hipLaunchKernelGGL(k_lpc_tail, dim3((unsigned)(nstreams * ch)), dim3(64), lds_lpc, s, ch, nstreams, pcm, stream_stride,
                       channel_stride, nsamples, c->B.bs[1], pad, (const long long *)ws.pending, geo);
    HIP_TRY(c, hipGetLastError());
    if (steps2 > 0 &&
        (r = envelope_search_batch(c, geo ? pcm : pcm + steps1 * E.searchstep, stream_stride, channel_stride, nstreams, steps2, states, flags2,
                                   c->d_bad + 1, count2, first2)))
      return r;
    B.eof = nsamples;
    B.nsamples = nsamples + pad;
    B.nsteps = steps_all;
  } else if (steps1 && (r = vamd_envelope_search_batch(c, pcm, stream_stride, channel_stride, nstreams, steps1, states, flags1)))
    return r;
  HIP_TRY(c, hipMemsetAsync(ws.counts, 0, (size_t)nstreams * 2 * sizeof(int), s));
  hipLaunchKernelGGL(k_plan_streams, dim3((unsigned)nstreams), dim3(64), plan_lds, s, B, nstreams, flags1, steps1, steps1, flags2, steps2,
                     (PlannedBlock *)ws.blocks, (int *)ws.counts, (long long *)nullptr, geo, 1, window);
  HIP_TRY(c, hipGetLastError());
  return plan_emit(c, B, nstreams, stream_stride, ws, plan);
}

int vamd_plan_streams(vamd_ctx *c, const float *pcm, long stream_stride, long channel_stride, long nstreams, long nsamples,
                      vamd_envelope_state *states, vamd_stream_plan *plan) {
  VAMD_NEEDS_ENCODER(c);
  return plan_streams(c, (float *)pcm, stream_stride, channel_stride, nstreams, nsamples, states, plan, 0);
}

int vamd_plan_streams_whole(vamd_ctx *c, float *pcm, long stream_stride, long channel_stride, long nstreams, long nframes,
                            vamd_envelope_state *states, vamd_stream_plan *plan) {
  VAMD_NEEDS_ENCODER(c);
  if (c && nframes < 0) return fail(c, VAMD_EINVAL, "negative frame count");
  return plan_streams(c, pcm, stream_stride, channel_stride, nstreams, c ? c->B.bs[1] / 2 + nframes : 0, states, plan, 1);
}

int vamd_plan_streams_whole_v(vamd_ctx *c, float *pcm, long stream_stride, long channel_stride, long nstreams, long max_frames,
                              const int64_t *nframes, vamd_envelope_state *states, vamd_stream_plan *plan) {
  VAMD_NEEDS_ENCODER(c);
  if (c && (max_frames < 0 || !nframes)) return fail(c, VAMD_EINVAL, "negative frame count / null lengths");
  return plan_streams(c, pcm, stream_stride, channel_stride, nstreams, c ? c->B.bs[1] / 2 + max_frames : 0, states, plan, 1, nframes);
}

// ---- the live feed's plan (vamd_live.h; vamd_feed.hip is its caller) ----
long vamd_live_retain(const vamd_ctx *c, int write_frames) {
  const long bs0 = c->B.bs[0], bs1 = c->B.bs[1], step = c->B.env.searchstep;
  long run = 3 * bs1 / 4 + bs0 / 4 + (VAMD_VE_WIN + 3) * step;  // (a): out of detector steps
  if (run < bs1) run = bs1;                                    // (b): the next window does not fit
  const long walk = run + bs1 / 2 + 2 * step, head = bs1 / 2 + live_n_head(c, write_frames);
  return walk > head ? walk : head;
}

static size_t live_lpc_lds(const vamd_ctx *c, int write_frames) { return lpc_lds(c, live_n_head(c, write_frames)); }

// (the walk's LDS: a mark and a flag byte per step of the largest buffer)
static size_t live_plan_lds(long steps) { return (size_t)(((steps + 4 + 15) & ~15L) + ((steps + 15) & ~15L)); }

const char *vamd_live_check(const vamd_ctx *c, int write_frames, long max_frames) {
  if (!c || write_frames < 1) return "bad context / write cadence";
  if (live_lpc_lds(c, write_frames) > c->lds_per_block)
    return "write_frames too large: the backward extrapolation over its first n_head frames does not fit a workgroup's LDS";
  const long cap = 2 * vamd_live_retain(c, write_frames) + max_frames + 3 * c->B.bs[1] + 256;
  if (live_plan_lds(cap / c->B.env.searchstep) > c->lds_per_block) return "max_frames too large for one piece: its detector marks must fit a workgroup's LDS";
  return nullptr;
}

int vamd_live_plan(vamd_ctx *c, float *pcm, long ss, long cs, long nstreams, const vamd_live_geo *lg, int n_head,
                   void *walk, unsigned char *rows, long row_stride, vamd_envelope_state *states, long long *shift,
                   vamd_stream_plan *plan) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!plan || !lg || !pcm || !walk || !rows || !states || !shift || nstreams < 1) return fail(c, VAMD_EINVAL, "live plan: null argument");
  memset(plan, 0, sizeof(*plan));
  plan->nstreams = nstreams;
  static_assert(sizeof(WalkState) == VAMD_LIVE_WALK_BYTES, "vamd_live.h: VAMD_LIVE_WALK_BYTES");
  const EnvP &E = c->B.env;
  const int ch = c->B.channels, head = c->B.bs[1] / 2, pad = 3 * c->B.bs[1];
  const long step = E.searchstep;
  const BlockoutP B = blockout_params(c, cs, cs);
  // per stream: k_plan_live's geometry, the two extrapolations' (eof < 0: not in this group), the detector passes' step
  // counts and first samples; one upload out of the context's pinned buffer.  (shift[]: written by the walk, fetched.)
  const size_t o_ph = (size_t)nstreams * sizeof(LiveGeo), o_pt = o_ph + (size_t)nstreams * sizeof(PlanGeo),
               o_c1 = o_pt + (size_t)nstreams * sizeof(PlanGeo), o_c2 = o_c1 + (size_t)nstreams * 4,
               o_f1 = (o_c2 + (size_t)nstreams * 4 + 7) & ~(size_t)7, o_f2 = o_f1 + (size_t)nstreams * 8, o_sh = o_f2 + (size_t)nstreams * 8,
               total = o_sh + (size_t)nstreams * 8;
  int r;
  if ((r = pinned_get(c, c->h_geo, total, true))) return r;
  void *v_geo;
  if ((r = ws_get(c, 0, vamd_ctx::WS_PLAN_GEO, total, &v_geo))) return r;
  unsigned char *hg = (unsigned char *)c->h_geo.p, *dg = (unsigned char *)v_geo;
  LiveGeo *g = (LiveGeo *)hg;
  PlanGeo *gh = (PlanGeo *)(hg + o_ph), *gt = (PlanGeo *)(hg + o_pt);
  int *c1 = (int *)(hg + o_c1), *c2 = (int *)(hg + o_c2);
  long long *f1 = (long long *)(hg + o_f1), *f2 = (long long *)(hg + o_f2);
  long n1 = 0, n2 = 0, steps_max = 0;
  bool heads = false, closes = false;
  for (long i = 0; i < nstreams; i++) {
    const vamd_live_geo &x = lg[i];
    const long steps = (long)(x.kept + x.c1 + (x.close ? x.c2 : 0));
    if (x.have < 0 || x.have + pad + 128 > cs || x.kept < 0 || x.c1 < 0 || x.c2 < 0 || steps * step > cs)
      return fail(c, VAMD_EINVAL, "live plan: a stream's geometry outside its buffer");
    g[i].have = x.have, g[i].kept = (int)x.kept, g[i].c1 = (int)x.c1, g[i].c2 = (int)x.c2, g[i].fresh = x.fresh, g[i].close = x.close;
    gh[i].nsamples = gt[i].nsamples = x.have + pad;
    gh[i].eof = x.n_head > 0 ? head + x.n_head : -1;
    gt[i].eof = x.close ? x.have : -1;
    gh[i].nsteps = gt[i].nsteps = gh[i].split = gt[i].split = 0;
    // a stream with no steps in a pass reads from its buffer's start (the launch takes the longest stream's steps for all)
    c1[i] = (int)x.c1, f1[i] = x.c1 ? x.kept * step : 0;
    c2[i] = x.close ? (int)x.c2 : 0, f2[i] = c2[i] ? (x.kept + x.c1) * step : 0;
    if (c1[i] > n1) n1 = c1[i];
    if (c2[i] > n2) n2 = c2[i];
    if (steps > steps_max) steps_max = steps;
    heads |= x.n_head > 0;
    closes |= x.close != 0;
    if (x.kept + x.c1 > row_stride) return fail(c, VAMD_EINVAL, "live plan: a stream's flags do not fit its row");
  }
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(dg, hg, o_sh, hipMemcpyHostToDevice, s));
  const LiveGeo *d_g = (const LiveGeo *)dg;
  const PlanGeo *d_gh = (const PlanGeo *)(dg + o_ph), *d_gt = (const PlanGeo *)(dg + o_pt);
  const int *d_c1 = (const int *)(dg + o_c1), *d_c2 = (const int *)(dg + o_c2);
  const long long *d_f1 = (const long long *)(dg + o_f1), *d_f2 = (const long long *)(dg + o_f2);
  long long *d_sh = (long long *)(dg + o_sh);
  PlanWs ws;
  if ((r = plan_ws(c, nstreams, (size_t)nstreams * (n1 + n2 + 1), B.maxblocks, &ws))) return r;
  unsigned char *flags1 = (unsigned char *)ws.flags, *flags2 = flags1 + (size_t)nstreams * n1;
  const size_t plan_lds = live_plan_lds(steps_max), lds_lpc = lpc_lds(c, n_head);
  if (plan_lds > c->lds_per_block) return fail(c, VAMD_EINVAL, "live plan: a piece too long for one plan (its marks must fit a workgroup's LDS)");
  if (lds_lpc > c->lds_per_block) return fail(c, VAMD_EIMPL, "live plan: write cadence too large for the stream-start extrapolation");
  HIP_TRY(c, hipFuncSetAttribute((const void *)k_plan_live, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_per_block));
  if ((r = lpc_opt_in(c))) return r;
  // the stream starts that are due: lib/block.c:417-458 over the first n_head frames
  if (heads && n_head > 32)
    hipLaunchKernelGGL(k_lpc_head, dim3((unsigned)(nstreams * ch)), dim3(64), lds_lpc, s, ch, nstreams, pcm, ss, cs, head, n_head, d_gh);
  // the detector over every stream's new steps, from its carried state
  if (n1 && (r = envelope_search_batch(c, pcm, ss, cs, nstreams, n1, states, flags1, c->d_bad + 1, d_c1, d_f1))) return r;
  WalkState *d_walk = (WalkState *)walk;
  if (closes) {
    // the closing streams' ends as vamd_plan_streams_whole makes them: where the walk stands when the data runs out, the
    // forward extrapolation from there (lib/block.c:474-512), the detector over the padding
    hipLaunchKernelGGL(k_plan_live, dim3((unsigned)nstreams), dim3(64), plan_lds, s, B, nstreams, steps_max, d_g, rows, row_stride,
                       flags1, n1, flags2, n2, pad, d_walk, (PlannedBlock *)nullptr, (int *)nullptr, (long long *)ws.pending, (long long *)nullptr);
    hipLaunchKernelGGL(k_lpc_tail, dim3((unsigned)(nstreams * ch)), dim3(64), lds_lpc, s, ch, nstreams, pcm, ss, cs, 0L, c->B.bs[1], pad,
                       (const long long *)ws.pending, d_gt);
    HIP_TRY(c, hipGetLastError());
    if (n2 && (r = envelope_search_batch(c, pcm, ss, cs, nstreams, n2, states, flags2, c->d_bad + 1, d_c2, d_f2))) return r;
  }
  HIP_TRY(c, hipMemsetAsync(ws.counts, 0, (size_t)nstreams * 2 * sizeof(int), s));
  hipLaunchKernelGGL(k_plan_live, dim3((unsigned)nstreams), dim3(64), plan_lds, s, B, nstreams, steps_max, d_g, rows, row_stride,
                     flags1, n1, flags2, n2, pad, d_walk, (PlannedBlock *)ws.blocks, (int *)ws.counts, (long long *)nullptr, d_sh);
  HIP_TRY(c, hipGetLastError());
  return plan_emit(c, B, nstreams, ss, ws, plan, shift, d_sh, (size_t)nstreams * 8);
}

int vamd_gather_blocks(vamd_ctx *c, const vamd_stream_plan *plan, int W, const float *pcm, long channel_stride,
                       float *pcm_blocks) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!plan || (W != 0 && W != 1)) return fail(c, VAMD_EINVAL, "null plan / bad size class");
  const long nb = plan->nblocks[W];
  if (nb == 0) return VAMD_OK;
  if (!pcm || !pcm_blocks) return fail(c, VAMD_EINVAL, "null pcm / pcm_blocks");
  if (channel_stride & 3) return fail(c, VAMD_EINVAL, "channel stride must be a multiple of 4 samples");
  if (((uintptr_t)pcm | (uintptr_t)pcm_blocks) & 15) return fail(c, VAMD_EINVAL, "pcm / pcm_blocks must be 16-byte aligned");
  const int ch = c->B.channels, n = c->B.bs[W];
  const long total = nb * ch * (n / 4);
  const long blocks = (total + 255) / 256;
  const long cap = (long)c->num_cus * 16;
  hipLaunchKernelGGL(k_gather_blocks, dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, c->stream, ch, n, nb,
                     (const long long *)plan->src[W], channel_stride, pcm, pcm_blocks);
  HIP_TRY(c, hipGetLastError());
  return VAMD_OK;
}

int vamd_plan_fetch(vamd_ctx *c, const vamd_stream_plan *plan, int32_t *const lW[2], int32_t *const nW[2],
                    int32_t *const blocktype[2], int64_t *const src[2], int32_t *order, int64_t *stream_start) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!plan) return fail(c, VAMD_EINVAL, "null plan");
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (int W = 0; W < 2; W++) {
    const size_t n = (size_t)plan->nblocks[W];
    if (!n) continue;
    if (lW && lW[W]) HIP_TRY(c, hipMemcpy(lW[W], plan->lW[W], n * 4, hipMemcpyDeviceToHost));
    if (nW && nW[W]) HIP_TRY(c, hipMemcpy(nW[W], plan->nW[W], n * 4, hipMemcpyDeviceToHost));
    if (blocktype && blocktype[W]) HIP_TRY(c, hipMemcpy(blocktype[W], plan->blocktype[W], n * 4, hipMemcpyDeviceToHost));
    if (src && src[W]) HIP_TRY(c, hipMemcpy(src[W], plan->src[W], n * 8, hipMemcpyDeviceToHost));
  }
  const size_t all = (size_t)(plan->nblocks[0] + plan->nblocks[1]);
  if (order && all) HIP_TRY(c, hipMemcpy(order, plan->order, all * 4, hipMemcpyDeviceToHost));
  if (stream_start && plan->nstreams) HIP_TRY(c, hipMemcpy(stream_start, plan->stream_start, (size_t)(plan->nstreams + 1) * 8, hipMemcpyDeviceToHost));
  return VAMD_OK;
}
