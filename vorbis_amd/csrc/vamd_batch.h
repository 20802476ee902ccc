// vamd_batch.h -- the batch calls of the C ABI (device pointers in, device pointers out): workspace planning, the launch
// sequence of the stages (launch_transform ... launch_floor_on) and the runs that put them in order (run_batch,
// run_streams_mixed), with their entry points.  Part of the library's single translation unit: included by vamd_hip.hip,
// once, inside its extern "C" block, after vamd_ctx.h.
#pragma once
struct WsPlan {
  float *mdct_raw, *logmdct, *logfft, *noise, *tone, *mdct, *local, *ampin, *ampglob, *seed;
  float *peaks;  // [channel-blocks][run_peaks_stride]: logfft's peak per run of bins, or null below the psy level
  unsigned short *surv;
  int32_t *nsurv;
  ilog_t *ilogmask;  // a byte per bin, workspace only (the int32 tap is widened from it: k_widen_ilog)
  int32_t *iwork, *posts, *post_valid, *nonzero;
  int32_t *wrapped;  // [channel-blocks][VAMD_POSTS_STRIDE] floor1_encode's out[], k_floor -> k_pack; null unless packets are assembled
  unsigned char *status;
};

// floats per channel-block of the run-peak hand-over (k_transform -> k_tone_seed), rows 16-byte aligned
static int run_peaks_stride(const PsyP &P) { return (P.nruns + 3) & ~3; }

// Resolve every inter-stage tensor: the caller's buffer when given, otherwise workspace.
static int plan(vamd_ctx *c, int W, long nb, const vamd_batch_io *io, int level, WsPlan *p) {
  const size_t ch = c->B.channels, n2 = c->B.bs[W] / 2;
  const size_t per = (size_t)nb * ch * n2 * 4;
  p->wrapped = nullptr;
  void *v;
#define PICK(field, user, slot, bytes)                     \
  do {                                                     \
    if (user) {                                            \
      p->field = user;                                     \
    } else {                                               \
      int r__ = ws_get(c, W, vamd_ctx::slot, (bytes), &v); \
      if (r__) return r__;                                 \
      p->field = (decltype(p->field))v;                    \
    }                                                      \
  } while (0)
  PICK(mdct_raw, io ? io->mdct_raw : nullptr, WS_MDCT_RAW, per);
  p->logmdct = io ? io->logmdct : nullptr;  // a tap only: the later stages form it from mdct_raw
  p->logfft = io ? io->logfft : nullptr;  // a tap only: the tone stage reads the run peaks
  p->peaks = nullptr;
  if (level >= VAMD_LEVEL_PSY) {
    PICK(peaks, (float *)nullptr, WS_LOGFFT, (size_t)nb * ch * run_peaks_stride(c->B.psy[2 * W]) * 4);
  }
  PICK(local, io ? io->local_ampmax : nullptr, WS_LOCAL, (size_t)nb * ch * 4);
  PICK(ampglob, io ? io->ampmax_out : nullptr, WS_AMPGLOB, (size_t)nb * 4);
  PICK(ampin, (float *)nullptr, WS_AMPIN, (size_t)nb * 4);
  PICK(status, io ? io->status : nullptr, WS_STATUS, (size_t)nb * ch);
  if (level >= VAMD_LEVEL_PSY) {
    PICK(noise, io ? io->noise : nullptr, WS_NOISE, per);
    PICK(tone, io ? io->tone : nullptr, WS_TONE, per);
    const size_t nlp = (size_t)VAMD_LINES_PAD(c->B.psy[2 * W].total_octave_lines);
    PICK(seed, (float *)nullptr, WS_SEED, (size_t)nb * ch * nlp * 4);
    PICK(surv, (unsigned short *)nullptr, WS_SURV, (size_t)nb * ch * nlp * 2);
    PICK(nsurv, (int32_t *)nullptr, WS_NSURV, (size_t)nb * ch * 4);
  }
  if (level >= VAMD_LEVEL_FULL) {
    PICK(mdct, io ? io->mdct : nullptr, WS_MDCT, per);
    PICK(ilogmask, (ilog_t *)nullptr, WS_ILOGMASK, per / 4 * sizeof(ilog_t));
    PICK(iwork, io ? io->iwork : nullptr, WS_IWORK, per);
    PICK(posts, io ? io->posts : nullptr, WS_POSTS, (size_t)nb * ch * VAMD_POSTS_STRIDE * 4);
    PICK(post_valid, io ? io->post_valid : nullptr, WS_POSTVALID, (size_t)nb * ch * 4);
    PICK(nonzero, io ? io->nonzero : nullptr, WS_NONZERO, (size_t)nb * ch * 4);
    if (io && io->packets) PICK(wrapped, (int32_t *)nullptr, WS_WRAPPED, (size_t)nb * ch * VAMD_POSTS_STRIDE * 4);
  }
#undef PICK
  return VAMD_OK;
}

int vamd_reserve(vamd_ctx *c, int W, long max_blocks) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  if (!c || (W != 0 && W != 1) || max_blocks < 1) return VAMD_EINVAL;
  WsPlan p;
  return plan(c, W, max_blocks, nullptr, VAMD_LEVEL_FULL, &p);
}

// (test aid) the seed lines, survivor lists and counts the last run of size class W left in the workspace
int vamd_debug_survivors(vamd_ctx *c, int W, long ncb, float *seed, uint16_t *surv, int32_t *nsurv, int32_t *row_lines,
                         int32_t *lines) {
  DeviceGuard dev_guard(c);
  if (!c || (W != 0 && W != 1) || ncb < 0) return VAMD_EINVAL;
  const size_t nl = (size_t)c->B.psy[2 * W].total_octave_lines, nlp = (size_t)VAMD_LINES_PAD(nl);
  if (row_lines) *row_lines = (int32_t)nlp;
  if (lines) *lines = (int32_t)nl;
  if (!seed && !surv && !nsurv) return VAMD_OK;
  const DevBuf &bs = c->ws[W][vamd_ctx::WS_SEED], &bv = c->ws[W][vamd_ctx::WS_SURV], &bn = c->ws[W][vamd_ctx::WS_NSURV];
  if (bs.bytes < (size_t)ncb * nlp * 4 || bv.bytes < (size_t)ncb * nlp * 2 || bn.bytes < (size_t)ncb * 4)
    return fail(c, VAMD_EINVAL, "no batch of that size has left survivor lists");
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if (seed) HIP_TRY(c, hipMemcpy(seed, bs.p, (size_t)ncb * nlp * 4, hipMemcpyDeviceToHost));
  if (surv) HIP_TRY(c, hipMemcpy(surv, bv.p, (size_t)ncb * nlp * 2, hipMemcpyDeviceToHost));
  if (nsurv) HIP_TRY(c, hipMemcpy(nsurv, bn.p, (size_t)ncb * 4, hipMemcpyDeviceToHost));
  return VAMD_OK;
}

// (test aid) the kernels the last batch call launched for size class W, as words in launch order
const char *vamd_launch_record(const vamd_ctx *c, int W) { return c && (W == 0 || W == 1) ? c->roads[W] : ""; }

// from a run-time size to a template argument: the call site defines VAMD_GO(arg) as its launch
#define VAMD_SWITCH_LOGN(logn)   \
  switch (logn) {                \
    case 8: VAMD_GO(8); break;   \
    case 9: VAMD_GO(9); break;   \
    case 10: VAMD_GO(10); break; \
    case 11: VAMD_GO(11); break; \
    case 12: VAMD_GO(12); break; \
    default: VAMD_GO(0);         \
  }
#define VAMD_SWITCH_BINS(n2)                                                                \
  switch (n2) {                                                                             \
    case 32: VAMD_GO(5); break;                                                             \
    case 64: VAMD_GO(6); break;                                                             \
    case 128: VAMD_GO(7); break;                                                            \
    case 256: VAMD_GO(8); break;                                                            \
    case 512: VAMD_GO(9); break;                                                            \
    case 1024: VAMD_GO(10); break;                                                          \
    default: VAMD_GO(11); break; /* 2048 bins: the largest block size the context accepts */ \
  }

int vamd_mdct_forward_batch(vamd_ctx *c, int W, const float *in, float *out, long nframes) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  if (!c || (W != 0 && W != 1) || nframes < 0) return VAMD_EINVAL;
  if (nframes == 0) return VAMD_OK;
  if (!in || !out) return fail(c, VAMD_EINVAL, "null frame buffer");
  if (nframes > 0x7fffffffL) return fail(c, VAMD_EINVAL, "too many frames for one launch");
  const XformP &P = c->B.xf[W];
  int waves = VAMD_MD_WAVES;
  while (waves > 1 && mdct_only_lds_bytes(P, waves) > c->lds_per_block) waves--;
  const long groups = (nframes + waves - 1) / waves;
  const unsigned grid = (unsigned)(groups < c->num_cus ? groups : c->num_cus);
#define VAMD_GO(LOGN)                                                                                                     \
  hipLaunchKernelGGL(k_mdct_only<LOGN>, dim3(grid), dim3(64 * waves), mdct_only_lds_bytes(P, waves), c->stream, P, W, nframes, \
                     in, out)
  VAMD_SWITCH_LOGN(fixed_logn(P))
#undef VAMD_GO
  HIP_TRY(c, hipGetLastError());
  return VAMD_OK;
}

static int check_desc(vamd_ctx *c, const vamd_batch_desc *d, const vamd_batch_io *io) {
  if (!c) return VAMD_EINVAL;
  if (!d || !io || !io->pcm) return fail(c, VAMD_EINVAL, "null descriptor / io / pcm");
  if (d->W != 0 && d->W != 1) return fail(c, VAMD_EINVAL, "W must be 0 or 1");
  if (d->nblocks < 0 || d->nblocks * (long)c->B.channels > 0x7fffffffL)
    return fail(c, VAMD_EINVAL, "nblocks out of range");
  if (!d->blocktype && (d->uniform_blocktype != 0 && d->uniform_blocktype != 1))
    return fail(c, VAMD_EINVAL, "blocktype must be 0 or 1");
  if (!d->lW && (d->uniform_lW & ~1)) return fail(c, VAMD_EINVAL, "lW must be 0 or 1");
  if (!d->nW && (d->uniform_nW & ~1)) return fail(c, VAMD_EINVAL, "nW must be 0 or 1");
  return VAMD_OK;
}

// ---- the launch sequence ---------------------------------------------------------
// the residue search's outputs: the caller's buffers, or workspace when only the packets are wanted
struct ResBufs {
  int32_t *cls;
  uint16_t *entries;
  int32_t *count;
  uint8_t *books;  // [units][res_cap] the book of every entry, k_residue -> k_pack (workspace only)
};
struct BatchRun {
  int W;
  long nb;
  WsPlan p;
  DescP d;
  const vamd_batch_io *io;
  const vamd_managed_io *M;  // bitrate-managed: fifteen candidate packets per block, their outputs here (else null)
  ilog_t *m_ilogmask;        // ... and their integer floor curves, which live in workspace only
  long units;                // (block, candidate packet) pairs of the stages behind the floor: nb, or nb * VAMD_PACKETBLOBS
  ResBufs rb;
  float *couple_state;  // [units][4][ch][n2] or null (alloc_couple_state)
  bool make_ampmax;     // the block ampmax is formed by k_tone_seed (independent blocks at the psy level or above: no k_ampmax launch)
  bool want_res;        // the residue search runs whether or not the caller takes its outputs (vamd_analyze_batch_synth)
};

// what a mode's setup may leave uncovered (vamd_bind.h)
static int res_covered(vamd_ctx *c, int W) {
  if ((W != 0 && W != 1) || !c->B.res_cap[W])
    return fail(c, VAMD_EIMPL, "this mode's residue back-end is not covered on the GPU (residue types 1 and 2 are)");
  return VAMD_OK;
}
static int packets_assembled(vamd_ctx *c, int W) {
  if ((W != 0 && W != 1) || c->B.pack[W].capacity == 0)
    return fail(c, VAMD_EIMPL, "this mode's packets are not assembled on the GPU (its residue back-end is not covered)");
  return VAMD_OK;
}

static int check_packets(vamd_ctx *c, int W, int level, const void *packets, const void *bits, int64_t stride) {
  if (!(packets && bits)) return fail(c, VAMD_EINVAL, "packets / packet_bits go together");
  if (level < VAMD_LEVEL_FULL) return fail(c, VAMD_EINVAL, "packet outputs need level FULL");
  if (stride < 4 || (stride & 3) || stride > 0x7fffffffL) return fail(c, VAMD_EINVAL, "packet_stride must be a positive multiple of 4");
  return packets_assembled(c, W);
}

static int res_bufs(vamd_ctx *c, int W, long units, int32_t *cls, uint16_t *entries, int32_t *count, ResBufs *o) {
  o->cls = cls, o->entries = entries, o->count = count;
  void *v;
  int r;
  if ((r = ws_get(c, W, vamd_ctx::WS_RES_BOOKS, (size_t)units * c->B.res_cap[W], &v))) return r;
  o->books = (uint8_t *)v;
  if (entries) return VAMD_OK;
  if ((r = ws_get(c, W, vamd_ctx::WS_RES_CLASS, (size_t)units * c->B.chmap[W].submaps * VAMD_RES_CLASS_STRIDE * 4, &v))) return r;
  o->cls = (int32_t *)v;
  if ((r = ws_get(c, W, vamd_ctx::WS_RES_ENTRIES, (size_t)units * c->B.res_cap[W] * 2, &v))) return r;
  o->entries = (uint16_t *)v;
  if ((r = ws_get(c, W, vamd_ctx::WS_RES_COUNT, (size_t)units * c->B.chmap[W].submaps * 8, &v))) return r;
  o->count = (int32_t *)v;
  return VAMD_OK;
}

// layouts beyond stereo keep the channels' running state of the coupling stage in HBM (k_couple.h)
static bool needs_general_couple(const vamd_ctx *c, int W) {
  return c->B.channels > 2 || c->B.couple[W].coupling_steps > 1;
}
static int alloc_couple_state(vamd_ctx *c, BatchRun *R) {
  R->couple_state = nullptr;
  if (R->nb == 0 || !needs_general_couple(c, R->W)) return VAMD_OK;
  void *v;
  int r = ws_get(c, R->W, vamd_ctx::WS_COUPLE_STATE, (size_t)R->units * 4 * c->B.channels * (c->B.bs[R->W] / 2) * 4, &v);
  if (r) return r;
  R->couple_state = (float *)v;
  return VAMD_OK;
}

// M: the run is bitrate-managed (the caller has checked it: check_managed), `io` then holds the shared tensors only
static int prepare_run(vamd_ctx *c, const vamd_batch_desc *desc, const vamd_batch_io *io, int level, BatchRun *R,
                       const vamd_managed_io *M = nullptr, bool want_res = false) {
  memset(R, 0, sizeof(*R));
  c->synth_src[desc->W].nb = -1;  // (the run's tensors replace the last run's)
  R->want_res = want_res;
  int r;
  if (io && (io->res_class || io->res_entries || io->res_count)) {
    if (!(io->res_class && io->res_entries && io->res_count)) return fail(c, VAMD_EINVAL, "res_class / res_entries / res_count go together");
    if (level < VAMD_LEVEL_FULL) return fail(c, VAMD_EINVAL, "residue outputs need level FULL");
    if ((r = res_covered(c, desc->W))) return r;
  }
  if (io && (io->packets || io->packet_bits) &&
      (r = check_packets(c, desc->W, level, io->packets, io->packet_bits, io->packet_stride)))
    return r;
  R->W = desc->W;
  R->nb = desc->nblocks;
  R->io = io;
  R->M = M;
  R->units = M ? R->nb * VAMD_PACKETBLOBS : R->nb;
  if (R->nb == 0) return VAMD_OK;
  if ((r = plan(c, R->W, R->nb, io, level, &R->p))) return r;
  if (io && level >= VAMD_LEVEL_FULL && (io->res_entries || io->packets || want_res) &&
      (r = res_bufs(c, R->W, R->units, io->res_class, io->res_entries, io->res_count, &R->rb)))
    return r;
  if (M) {  // the fifteen integer floor curves live in workspace only
    void *v;
    if ((r = ws_get(c, R->W, vamd_ctx::WS_M_ILOGMASK, (size_t)R->units * c->B.channels * (c->B.bs[R->W] / 2) * sizeof(ilog_t), &v)))
      return r;
    R->m_ilogmask = (ilog_t *)v;
    if ((M->res_entries || M->packets) && (r = res_bufs(c, R->W, R->units, M->res_class, M->res_entries, M->res_count, &R->rb)))
      return r;
  }
  if (level >= VAMD_LEVEL_FULL && (r = alloc_couple_state(c, R))) return r;
  DescP &d = R->d;
  d.lW = desc->lW;
  d.nW = desc->nW;
  d.blocktype = desc->blocktype;
  d.ampmax_in = desc->ampmax_in;
  d.u_lW = desc->uniform_lW;
  d.u_nW = desc->uniform_nW;
  d.u_blocktype = desc->uniform_blocktype;
  d.u_ampmax_in = desc->uniform_ampmax_in;
  d.dbg = c->d_dbg;
  d.clk = c->d_clk;
  d.status = R->p.status;
  d.bad = c->d_bad;
  d.src = nullptr;
  d.cstride = 0;
  if (io && io->pcm_src) {
    if ((io->pcm_channel_stride & 3) || ((uintptr_t)io->pcm & 15)) return fail(c, VAMD_EINVAL, "pcm_src: pcm 16-byte aligned, pcm_channel_stride a multiple of 4");
    d.src = (const long long *)io->pcm_src;
    d.cstride = (long)io->pcm_channel_stride;
  }
  return VAMD_OK;
}

// stage 1 (window, MDCT, FFT, logs, local ampmax)
static void launch_transform(vamd_ctx *c, BatchRun *R) {
  if (R->nb == 0) return;
  const int ch = c->B.channels;
  const XformP &X = c->B.xf[R->W];
  const unsigned gcb = (unsigned)(R->nb * ch);
  const int waves = xf_waves(c, X);
  const long groups = ((long)gcb + waves - 1) / waves;
  const unsigned grid = (unsigned)(groups < c->num_cus ? groups : c->num_cus);
  const PsyP &PS = c->B.psy[2 * R->W];  // (the runs are the size class's: vamd_bind checks both block types share them)
  prof_mark(c, VAMD_ST_BEGIN);
#define VAMD_GO(LOGN)                                                                                                      \
  hipLaunchKernelGGL(k_transform<LOGN>, dim3(grid), dim3(64 * waves), transform_lds_bytes(X, waves), c->stream, X, R->W, R->d, \
                     ch, (long)gcb, R->io->pcm, R->p.mdct_raw, R->p.logmdct, R->p.logfft, R->p.local, PS.run_of_bin, PS.nruns,    \
                     run_peaks_stride(PS), R->p.peaks)
  VAMD_SWITCH_LOGN(fixed_logn(X))
#undef VAMD_GO
  prof_mark(c, VAMD_ST_TRANSFORM);
}

// the grid of a persistent kernel: as many workgroups as are resident at once, or the `want` that the work gives
static unsigned persistent_grid(vamd_ctx *c, const void *kernel, int threads, size_t lds, long want) {
  int resident = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&resident, kernel, threads, lds) != hipSuccess || resident < 1) {
    (void)hipGetLastError();
    resident = 1;
  }
  const long fill = (long)c->num_cus * resident;
  return (unsigned)(want < fill ? want : fill);
}

// stage 6 for every submap of the mode, then (optionally) stage 7; a unit is a (block, candidate packet)
static void launch_residue_pack(vamd_ctx *c, BatchRun *R, hipStream_t s, int nblobs, const int *posts,
                                const int *wrapped /* k_floor's out[] per post, or null */, const int *post_valid, const int *iwork, const int *nonzero, const ResBufs &rb,
                                void *packets, int64_t packet_stride, int32_t *packet_bits) {
  const int W = R->W, ch = c->B.channels, n2 = c->B.xf[W].n / 2;
  const ChMap &cm = c->B.chmap[W];
  const long res_team_max = c->K.res_team_max, units = R->units;
  for (int sm = 0; sm < cm.submaps; sm++) {
    const ResP &Rs = c->B.res[W][sm];
    // round 6: a stereo type-2 residue whose vectors tile runs of eight values is searched out of registers, a lane per
    // run, a wave per block (k_residue_chunks: persistent waves)
    const int chunks = Rs.chunked && !c->K.res_in_lds && ((uintptr_t)iwork & 15) == 0 && (n2 & 3) == 0
                           ? Rs.partvals * (Rs.tab_grouping >> 3) : 0;
    if (chunks > 0 && units <= res_team_max && chunks <= 64 * VAMD_RES_WAVES) {
      // a handful of units: a workgroup a unit, a thread a run (residue_team_chunks) -- a lone block's search in half the time
      road(c, W, "k_residue:team", (chunks + 63) & ~63);
      hipLaunchKernelGGL(k_residue, dim3((unsigned)units), dim3((chunks + 63) & ~63),
                         (size_t)(Rs.lds_ints - Rs.bundle * n2 + Rs.fast_ints) * 4, s, Rs, cm, sm,
                         c->B.res_cap[W], nblobs, R->d, ch, n2, iwork, nonzero, rb.cls, rb.entries, rb.count, packets ? rb.books : nullptr, 1);
      continue;
    }
    if (chunks > 0 && units > res_team_max) {
      const size_t per_wave = (size_t)((Rs.partvals + Rs.nstages * Rs.partvals + 1 + 3) & ~3);
      const size_t lds = ((size_t)Rs.fast_ints + VAMD_RESC_WAVES * per_wave) * 4;
      const unsigned grid = persistent_grid(c, (const void *)k_residue_chunks, 64 * VAMD_RESC_WAVES, lds, (units + VAMD_RESC_WAVES - 1) / VAMD_RESC_WAVES);
      road(c, W, "k_residue_chunks");
      hipLaunchKernelGGL(k_residue_chunks, dim3(grid), dim3(64 * VAMD_RESC_WAVES), lds, s, Rs, cm, sm, c->B.res_cap[W], nblobs, R->d, ch,
                         n2, units, iwork, nonzero, rb.cls, rb.entries, rb.count, packets ? rb.books : nullptr);
      continue;
    }
    // a stereo bundle's search keeps two waves busy, the five-channel bundle of the 5.1 layout four; a handful of units
    // takes four either way (nothing else wants the CU, and a lone unit's latency is the caller's)
    const int res_threads = 64 * (c->B.res[W][sm].bundle * n2 > 4096 || units <= res_team_max ? VAMD_RES_WAVES : 2);
    road(c, W, "k_residue", res_threads);
    hipLaunchKernelGGL(k_residue, dim3((unsigned)units), dim3(res_threads),
                       (size_t)c->B.res[W][sm].lds_ints * 4, s, c->B.res[W][sm], cm, sm,
                       c->B.res_cap[W], nblobs, R->d, ch, n2, iwork, nonzero, rb.cls, rb.entries, rb.count, packets ? rb.books : nullptr, 0);
  }
  prof_mark(c, VAMD_ST_RESIDUE);
  if (packets) {
    const size_t lds = ((size_t)VAMD_PK_RING + VAMD_POSTS_STRIDE + VAMD_RES_CLASS_STRIDE + 2 * (size_t)c->B.res_off_ints[W] +
                        VAMD_PK_FTAB_INTS + 3 * (size_t)c->B.pack[W].nbooks) * 4;
    const long pair_max = c->K.pack_pair_max;
    // a handful of packets: two waves each -- where the rows hold any packet (the residue part is assembled past the
    // longest possible head and then moved down: in a shorter row the end of a cut-off packet would be lost on the way)
    if (units <= pair_max && packet_stride >= c->B.pack[W].capacity) {
      road(c, W, "k_pack_pair");
      hipLaunchKernelGGL(k_pack_pair, dim3((unsigned)units), dim3(128), lds + ((size_t)VAMD_PK_RING + 4 + c->B.res[W][0].fast_ints) * 4, s, c->B.pack[W],
                         c->B.floor[W][0], c->B.floor[W][1], c->B.res[W][0], c->B.res[W][1], cm, c->B.res_cap[W], c->B.res_off_ints[W],
                         R->d, ch, W, nblobs, posts, wrapped, post_valid, rb.cls, rb.entries, rb.books, rb.count, (unsigned *)packets,
                         (int)(packet_stride / 4), packet_bits);
    } else if (cm.submaps == 1 && units >= 4 * (long)c->num_cus && !c->K.pack_per_packet) {
      // a batch of a one-submap mode: persistent waves over the packets, the tables staged once per workgroup (k_pack_waves)
      const ResP &R0 = c->B.res[W][0];
      const int per_wave_ints = (R0.slots + 2 * R0.nstages * R0.slots + 1 + 3) & ~3;
      const size_t ldsw = ((size_t)((VAMD_PK_FTAB_INTS + 3 * c->B.pack[W].nbooks + 3) & ~3) + (size_t)R0.fast_ints +
                           (size_t)VAMD_PKW_WAVES * ((size_t)VAMD_PK_RING + VAMD_POSTS_STRIDE + per_wave_ints)) * 4;
      // (persistent -- registers, not LDS, set how many workgroups are resident here)
      const unsigned grid = persistent_grid(c, (const void *)k_pack_waves, 64 * VAMD_PKW_WAVES, ldsw, (units + VAMD_PKW_WAVES - 1) / VAMD_PKW_WAVES);
      road(c, W, "k_pack_waves");
      hipLaunchKernelGGL(k_pack_waves, dim3(grid), dim3(64 * VAMD_PKW_WAVES), ldsw, s, c->B.pack[W],
                         c->B.floor[W][0], R0, cm, c->B.res_cap[W], per_wave_ints, R->d, ch, W, nblobs, units, posts, wrapped, post_valid,
                         rb.cls, rb.entries, rb.books, rb.count, (unsigned *)packets, (int)(packet_stride / 4), packet_bits);
    } else {
      road(c, W, "k_pack");
      hipLaunchKernelGGL(k_pack, dim3((unsigned)units), dim3(64), lds, s, c->B.pack[W], c->B.floor[W][0], c->B.floor[W][1],
                         c->B.res[W][0], c->B.res[W][1], cm, c->B.res_cap[W], c->B.res_off_ints[W], R->d, ch, W, nblobs, posts,
                         wrapped, post_valid, rb.cls, rb.entries, rb.books, rb.count, (unsigned *)packets, (int)(packet_stride / 4), packet_bits);
    }
    prof_mark(c, VAMD_ST_PACK);
  }
}

// couple / quantise / normalise for the run's (block, candidate) pairs
static void launch_couple(vamd_ctx *c, BatchRun *R, hipStream_t s, int blob_base, int nblobs, const float *mdct,
                          const ilog_t *ilogmask, int *iwork, int *nonzero) {
  const int W = R->W, ch = c->B.channels;
  const PsyP &P0 = c->B.psy[2 * W], &P1 = c->B.psy[2 * W + 1];
  const int n2 = c->B.xf[W].n / 2;
  const long units = R->units;
  if (needs_general_couple(c, W)) {
    road(c, W, "k_couple_general");
    hipLaunchKernelGGL(k_couple_general, dim3((unsigned)units), dim3(64), (size_t)n2 * 12 + 1024, s, P0, P1, c->B.couple_all[W],
                       blob_base, nblobs, R->d, mdct, ilogmask, iwork, nonzero, R->couple_state);
    return;
  }
  // the LDS arrays serve noise normalisation's sort only (lib/psy.c:941-1010); without it the
  // stage is register-only and the CU holds twice as many of its waves
  const bool norm0 = P0.normal_p && P0.normal_start < n2, norm1 = P1.normal_p && P1.normal_start < n2;
  if (norm0 || norm1) {
    road(c, W, "k_couple_norm");
    hipLaunchKernelGGL(k_couple_norm, dim3((unsigned)units), dim3(64), (size_t)n2 * 12 + 1024, s, P0, P1, c->B.couple_all[W], blob_base,
                       nblobs, R->d, mdct, ilogmask, iwork, nonzero, c->couple_band);
  } else {  // (a handful of blocks: four waves each)
    const int couple_threads = units <= 2048 && n2 >= 512 ? 256 : 64;
    road(c, W, "k_couple", couple_threads);
    hipLaunchKernelGGL(k_couple, dim3((unsigned)units), dim3(couple_threads), 0, s, P0, P1, c->B.couple_all[W],
                       blob_base, nblobs, R->d, mdct, ilogmask, iwork, nonzero, c->couple_band);
  }
}

// ---- stages 2..5 (masking, floor, couple) and what follows them, in two steps; R->d.ampmax_in / p.ampglob must be final.
// A mixed run issues both size classes' masks before either's floor, so that the short blocks' tone chain -- as long as
// the long blocks', beside a noise mask a fifth as long -- has the long blocks' noise mask and floor fits to run beside
// (C5: visible tone tail 1.08 -> see DESIGN section 6).

// the tone chain on the side stream, beside the noise mask
// (a handful of blocks: the fork / join through events costs more than running the tone chain beside the noise mask
// saves -- one stereo block 192 us with it, 181 without)
static bool masks_overlap(const vamd_ctx *c, const BatchRun *R) { return c->overlap && (unsigned)(R->nb * c->B.channels) > 64; }
static hipEvent_t join_event(const vamd_ctx *c, const BatchRun *R) { return R->W ? c->ev_join : c->ev_join2; }
// the fold's LDS: the seed lines, then a float per group and one for the tail bins' group (k_tone_fold.inc); whole 16
// bytes, so that the second half of a paired wave (k_floor_pair) starts aligned as well
static size_t fold_lds_bytes(int nlp, const PsyP &P0, const PsyP &P1) {
  return ((size_t)(nlp + (P0.ngroups > P1.ngroups ? P0.ngroups : P1.ngroups) + 1) * 4 + 15) & ~(size_t)15;
}
// the VBR path's floor stage takes the tone chain's last step with it (k_floor)
static bool fold_in_floor(const vamd_ctx *c, const BatchRun *R, int level) {
  const bool fold_env = !c->K.fold_separate;
  return fold_env && level >= VAMD_LEVEL_FULL && !R->M && c->B.xf[R->W].n / 2 <= 64 * 4 * VAMD_QPL;
}

// noise teams per CU (k_noise: persistent; `lds` bytes and nw waves a team)
//   alone: no other size class's masks and floors in this run for the tone chain to run beside
static long noise_teams_per_cu(const vamd_ctx *c, int n2, size_t lds, bool overlap, bool alone, bool fold_later) {
  // persistent teams.  A CU's LDS and 32 wave slots hold 8 of them at 1024 bins (both exactly full) -- but then the
  // tone chain on the side stream finds no room until they retire and runs behind them.  Six teams (three quarters of
  // the wave slots) keep the vector units as busy -- the stage is issue-bound -- and leave eight slots and 40 KB in
  // which the tone kernels, which wait on LDS atomics and memory, run BESIDE them.  (The figures behind every number
  // here, round by round: DESIGN.md, "Decided variants".)
  const int nw = n2 >= 256 ? 4 : (n2 >= 64 ? n2 / 64 : 1);
  long per_cu = (long)(c->lds_per_block / lds);
  if (per_cu > 32 / nw) per_cu = 32 / nw;
  const int noise_cap = c->K.noise_teams;  // (measurement aid)
  if (noise_cap > 0) {
    if (per_cu > noise_cap) per_cu = noise_cap;
  } else if (overlap) {
    // ... and where the tone chain carries its own last step (the fold as a launch of its own: the masks-only level,
    // bitrate-managed blocks) it needs half the CU to finish beside the noise mask: four teams (16 waves).  Otherwise
    // six teams (24 waves): the walk (k_tone.h: tone_chase_regs) takes no LDS and 62 VGPRs, two waves a SIMD in the 128
    // that six teams leave, and beside six the chain ends before the noise mask does; the seventh team is kept out by
    // k_tone_seed, which alone takes longer than the noise mask in the 4 wave slots seven leave.  A run of smaller
    // blocks alone keeps the five teams (20 waves) it was measured with.
    const int beside = c->K.noise_waves > 0 ? c->K.noise_waves : (alone && n2 < 1024 ? 20 : 24);
    const long cap = (fold_later ? beside : 16) / nw;
    if (per_cu > cap) per_cu = cap > 0 ? cap : 1;
  }
  return per_cu < 1 ? 1 : per_cu;
}

// the masks: noise on the main stream, the tone chain beside it, their join left open (launch_floor_on)
//   forked: the side stream already waits for everything the tone chain needs (run_streams_mixed's ampmax chain)
//   alone: no other size class's masks and floors in this run for the tone chain to run beside
static void launch_masks(vamd_ctx *c, BatchRun *R, int level, bool forked, bool alone) {
  if (R->nb == 0 || level < VAMD_LEVEL_PSY) return;
  const int W = R->W, ch = c->B.channels;
  const WsPlan &p = R->p;
  const DescP &d = R->d;
  const PsyP &P0 = c->B.psy[2 * W], &P1 = c->B.psy[2 * W + 1];
  const int n2 = c->B.xf[W].n / 2, nl = P0.total_octave_lines;
  const unsigned gcb = (unsigned)(R->nb * ch);
  hipStream_t s = c->stream;
  const bool overlap = masks_overlap(c, R);
  const bool fold_later = fold_in_floor(c, R, level);
  if (overlap && !forked) {  // fork: the tone chain needs only what is already queued on `stream`
    (void)hipEventRecord(c->ev_fork, c->stream);
    (void)hipStreamWaitEvent(c->side, c->ev_fork, 0);
  }
  const int nlp = VAMD_LINES_PAD(nl);
  const size_t seed_lds = (size_t)(seed_pad_lo(P0.eighth_octave_lines) + nlp + seed_pad_hi(P0.eighth_octave_lines)) * 4;
  // a lane per block for batches, a wave per block (the walk in 64 chunks) where that would leave the GPU to a
  // handful of lanes walking ~800 lines each: the per-block entry points, the batcher's small batches
  const long wave_max_cb = c->K.chase_wave_max;
  const bool by_wave = (long)gcb <= wave_max_cb && P0.eighth_octave_lines <= 16 && nl <= 2048;
  const bool lp8 = P0.eighth_octave_lines == 8 && P1.eighth_octave_lines == 8;
  // the stack walk's ring: VAMD_CHASE_RING slots where no window is longer than 8 lines, 16 otherwise (k_tone.h)
  const bool ring8 = P0.eighth_octave_lines <= 8 && P1.eighth_octave_lines <= 8;
  const size_t ring_slots = ring8 ? VAMD_CHASE_RING : VAMD_RING;
  // a handful of blocks, no second stream: both masks in one launch, side by side (k_noise_tone)
  const bool merge_env = !c->K.masks_separate;
  const bool merged = merge_env && !overlap && by_wave && lp8;
  if (merged) {
    const size_t nlds = (size_t)5 * VAMD_NZ_STRIDE(n2) * 4, tlds = seed_lds + (size_t)chase_ring_slots(8) * 8;
    road(c, W, "k_noise_tone");
#define VAMD_GO(L)                                                                                                          \
  hipLaunchKernelGGL((k_noise_tone<L, 8>), dim3(2 * gcb), dim3(64 * NoiseGeom<L>::NW), nlds > tlds ? nlds : tlds, s, P0, P1, d, ch, \
                     (long)gcb, p.mdct_raw, p.noise, nlp, run_peaks_stride(P0), p.peaks, p.local, p.ampglob,                  \
                     R->make_ampmax ? p.ampglob : nullptr, p.seed, p.surv, p.nsurv)
    VAMD_SWITCH_BINS(n2)
#undef VAMD_GO
    prof_mark(c, VAMD_ST_NOISE);
  } else {
    const size_t lds = (size_t)5 * VAMD_NZ_STRIDE(n2) * 4;
    const long per_cu = noise_teams_per_cu(c, n2, lds, overlap, alone, fold_later);
    const unsigned grid = (unsigned)((long)gcb < per_cu * c->num_cus ? (long)gcb : per_cu * c->num_cus);
    road(c, W, "k_noise");
#define VAMD_GO(L)                                                                                                    \
  hipLaunchKernelGGL(k_noise<L>, dim3(grid), dim3(64 * NoiseGeom<L>::NW), lds, s, P0, P1, d, ch, (long)gcb, p.mdct_raw, \
                     p.noise)
    VAMD_SWITCH_BINS(n2)
#undef VAMD_GO
    prof_mark(c, VAMD_ST_NOISE);
  }
  if (overlap) s = c->side;
  {
    if (merged) {
      // (launched with the noise stage)
    } else if (by_wave && lp8) {  // ... and seed + chase in one launch (k_tone_seed_chase)
      road(c, W, "k_tone_seed_chase");
      hipLaunchKernelGGL(k_tone_seed_chase<8>, dim3(gcb), dim3(64), seed_lds + (size_t)chase_ring_slots(8) * 8, s, P0, P1, d, ch, nlp,
                         run_peaks_stride(P0), p.peaks, p.local, p.ampglob, R->make_ampmax ? p.ampglob : nullptr, p.seed, p.surv,
                         p.nsurv);
    } else {
      road(c, W, lp8 ? "k_tone_seed" : "k_tone_seed<0>");
      if (lp8)
        hipLaunchKernelGGL(k_tone_seed<8>, dim3(gcb), dim3(64), seed_lds, s, P0, P1, d, ch, nlp, run_peaks_stride(P0), p.peaks, p.local,
                           p.ampglob, R->make_ampmax ? p.ampglob : nullptr, p.seed);
      else
        hipLaunchKernelGGL(k_tone_seed<0>, dim3(gcb), dim3(64), seed_lds, s, P0, P1, d, ch, nlp, run_peaks_stride(P0), p.peaks, p.local,
                           p.ampglob, R->make_ampmax ? p.ampglob : nullptr, p.seed);
      const size_t chase_pad = (size_t)c->K.chase_lds_pad;  // (experiment: the walk's waves per CU beside the noise mask)
#define VAMD_GO(RING)                                                                                                          \
  if (by_wave)                                                                                                                 \
    hipLaunchKernelGGL(k_tone_chase_wave<RING>, dim3(gcb), dim3(64), (size_t)nlp * 4 + (size_t)RING * 64 * 8, s,               \
                       P0.eighth_octave_lines, nl, nlp, d, p.seed, p.surv, p.nsurv);                                           \
  else                                                                                                                         \
    hipLaunchKernelGGL(k_tone_chase<RING>, dim3((gcb + VAMD_CHASE_LANES - 1) / VAMD_CHASE_LANES), dim3(VAMD_CHASE_LANES),      \
                       (size_t)RING * VAMD_CHASE_LANES * 8 + chase_pad, s, P0.eighth_octave_lines, nl, nlp, (long)gcb, d, p.seed, \
                       p.surv, p.nsurv)
      if (!by_wave && chase_walk_regs(P0, P1)) {  // the window in registers, no ring (k_tone.h: tone_chase_regs)
        road(c, W, "k_tone_chase_regs");
        hipLaunchKernelGGL(k_tone_chase_regs<8>, dim3((gcb + VAMD_CHASE_LANES - 1) / VAMD_CHASE_LANES), dim3(VAMD_CHASE_LANES), chase_pad, s,
                           nl, nlp, (long)gcb, d, p.seed, p.surv, p.nsurv);
      } else if (ring_slots == VAMD_RING) {
        road(c, W, by_wave ? "k_tone_chase_wave" : "k_tone_chase", (int)VAMD_RING);  // (the number: the ring's slots)
        VAMD_GO(VAMD_RING);
      } else {
        road(c, W, by_wave ? "k_tone_chase_wave" : "k_tone_chase", (int)VAMD_CHASE_RING);
        VAMD_GO(VAMD_CHASE_RING);
      }
#undef VAMD_GO
    }
    if (!fold_later) {
      road(c, W, "k_tone_fold");
      hipLaunchKernelGGL(k_tone_fold, dim3(gcb), dim3(64), fold_lds_bytes(nlp, P0, P1), s, P0, P1, d, ch, nlp, p.seed, p.surv,
                         p.nsurv, p.local, p.tone);
    }
  }
  if (overlap) (void)hipEventRecord(join_event(c, R), c->side);
}

// the rest: the masks' join, floor, tap, couple, residue + pack
static void launch_floor_on(vamd_ctx *c, BatchRun *R, int level) {
  if (R->nb == 0) return;
  const ResBufs &rb = R->rb;
  const int W = R->W, ch = c->B.channels;
  const WsPlan &p = R->p;
  const DescP &d = R->d;
  const vamd_managed_io *M = R->M;
  const PsyP &P0 = c->B.psy[2 * W], &P1 = c->B.psy[2 * W + 1];
  const int n2 = c->B.xf[W].n / 2, nlp_all = VAMD_LINES_PAD(P0.total_octave_lines);
  const unsigned gcb = (unsigned)(R->nb * ch), gb = (unsigned)R->nb;
  hipStream_t s = c->stream;
  const bool fold_here = fold_in_floor(c, R, level);
  const size_t fold_lds = fold_lds_bytes(nlp_all, P0, P1);
  if (level >= VAMD_LEVEL_PSY) {
    if (masks_overlap(c, R)) (void)hipStreamWaitEvent(s, join_event(c, R), 0);  // join
    prof_mark(c, VAMD_ST_TONE);
  }
  if (level >= VAMD_LEVEL_FULL && M) {
    // bitrate-managed: fifteen candidate packets per block
    const size_t flds = (size_t)((n2 + 15) & ~15) * 2 + sizeof(FloorScratch);
    road(c, W, "k_floor_managed");
    hipLaunchKernelGGL(k_floor_managed, dim3(gcb), dim3(64), flds, s, P0, P1, c->B.floor[W][0], c->B.floor[W][1], c->B.chmap[W], d, ch, p.noise, p.tone,
                       p.mdct_raw, p.mdct, R->io->logmask, M->posts, M->post_valid, R->m_ilogmask, M->nonzero);
    prof_mark(c, VAMD_ST_FLOOR);
    launch_couple(c, R, s, 0, VAMD_PACKETBLOBS, p.mdct, R->m_ilogmask, M->iwork, M->nonzero);
    prof_mark(c, VAMD_ST_COUPLE);
    if (M->res_entries || M->packets)
      launch_residue_pack(c, R, s, VAMD_PACKETBLOBS, M->posts, nullptr, M->post_valid, M->iwork, M->nonzero, rb,
                          M->packets, M->packet_stride, M->packet_bits);
  } else if (level >= VAMD_LEVEL_FULL) {
    const size_t floor_pad = (size_t)c->K.floor_lds_pad;  // (experiment: occupancy)
    size_t floor_lds = (size_t)((n2 + 15) & ~15) * 2 + sizeof(FloorScratch) + floor_pad;
    if (fold_here && fold_lds > floor_lds) floor_lds = fold_lds;
    // two channels per wave (k_floor_pair) for stereo setups whose channels share a floor of at most 32 posts, from
    // `floor_pair_min` channel-blocks up (a test knob; the default is set by what was measured: DESIGN section 6)
    const FloorP &F0 = c->B.floor[W][c->B.chmap[W].sub[0]];
    const long pair_min = c->K.floor_pair_min >= 0 ? c->K.floor_pair_min : (W ? VAMD_FLOOR_PAIR_MIN_LONG : VAMD_FLOOR_PAIR_MIN_SHORT);
    const bool paired = ch == 2 && c->B.chmap[W].sub[0] == c->B.chmap[W].sub[1] && F0.posts <= 32 && (long)gcb >= pair_min && pair_min >= 0 &&
                        ((c->K.floor_pair_w >> W) & 1) &&
                        n2 <= 32 * 4 * 8 && 2 * floor_lds <= c->lds_per_block;
    road(c, W, paired ? "k_floor_pair" : "k_floor");
    if (paired)
      hipLaunchKernelGGL(k_floor_pair, dim3(gb), dim3(64), 2 * floor_lds, s,
                         (const Bound *)c->d_bound, W, d, (int)floor_lds, p.noise, fold_here ? R->io->tone : p.tone, fold_here ? p.seed : nullptr, p.surv, p.nsurv, p.local,
                         nlp_all, p.mdct_raw, p.mdct,
                         R->io->logmask, p.posts, p.post_valid, p.ilogmask, p.nonzero, p.wrapped);
    else
    hipLaunchKernelGGL(k_floor, dim3(gcb), dim3(64), floor_lds, s,
                       (const Bound *)c->d_bound, W, d, ch, p.noise, fold_here ? R->io->tone : p.tone, fold_here ? p.seed : nullptr, p.surv, p.nsurv, p.local,
                       nlp_all, p.mdct_raw, p.mdct,
                       R->io->logmask, p.posts, p.post_valid, p.ilogmask, p.nonzero, p.wrapped);
    if (R->io->ilogmask) {  // (a tap: tests and callers with their own quantiser)
      road(c, W, "k_widen_ilog");
      hipLaunchKernelGGL(k_widen_ilog, dim3(1024), dim3(256), 0, s, (long)gcb * n2, (const ilog_t *)p.ilogmask, R->io->ilogmask);
    }
    prof_mark(c, VAMD_ST_FLOOR);
    launch_couple(c, R, s, VAMD_PACKETBLOBS / 2, 1, p.mdct, p.ilogmask, p.iwork, p.nonzero);
    prof_mark(c, VAMD_ST_COUPLE);
    if (R->io && (R->io->res_entries || R->io->packets || R->want_res)) {
      launch_residue_pack(c, R, s, 1, p.posts, p.wrapped, p.post_valid, p.iwork, p.nonzero, rb, R->io->packets, R->io->packet_stride,
                          R->io->packet_bits);
      vamd_ctx::SynthSrc &y = c->synth_src[W];
      y.nb = R->nb, y.post_valid = p.post_valid, y.ilogmask = p.ilogmask;
      y.res_class = rb.cls, y.res_entries = rb.entries, y.res_count = rb.count;
    }
  }
}

static int launch_synth(vamd_ctx *c, int W, const vamd_ctx::SynthSrc &y, float *synth, bool bounded = false);

static int run_batch(vamd_ctx *c, const vamd_batch_desc *desc, const vamd_batch_io *io, int level, bool stream_mode,
                     float *ampmax_state, const vamd_managed_io *M = nullptr, float *synth = nullptr) {
  BatchRun R;
  c->roads[0][0] = c->roads[1][0] = 0;  // (the record of what this call launches: vamd_launch_record)
  int r = prepare_run(c, desc, io, level, &R, M, synth != nullptr);
  if (r) return r;
  if (R.nb == 0) return VAMD_OK;
  const int ch = c->B.channels;
  hipStream_t s = c->stream;
  launch_transform(c, &R);
  if (stream_mode) {
    const float secs = (float)(c->B.xf[R.W].n / 2) / (float)c->B.rate;  // lib/psy.c:842-843
    hipLaunchKernelGGL(k_ampmax_stream, dim3(1), dim3(64), 0, s, ch, R.nb, secs, c->B.ampmax_att_per_sec, *ampmax_state,
                       R.p.local, R.p.ampin, R.p.ampglob);
    R.d.ampmax_in = R.p.ampin;
  } else if (level >= VAMD_LEVEL_PSY) {
    R.make_ampmax = true;  // (one launch less: 4 us of a single block's 180)
  } else {
    hipLaunchKernelGGL(k_ampmax, dim3((unsigned)((R.nb + 255) / 256)), dim3(256), 0, s, R.d, ch, R.nb, R.p.local,
                       R.p.ampglob);
  }
  prof_mark(c, VAMD_ST_AMPMAX);
  launch_masks(c, &R, level, false, true);
  launch_floor_on(c, &R, level);
  if (c->profile) c->prof_runs++;
  HIP_TRY(c, hipGetLastError());
  if (synth && (r = launch_synth(c, R.W, c->synth_src[R.W], synth))) return r;
  if (stream_mode) {
    // new state = ampmax_out of the last block
    HIP_TRY(c, hipMemcpyAsync(ampmax_state, R.p.ampglob + (R.nb - 1), sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  return VAMD_OK;
}

int vamd_analyze_batch(vamd_ctx *c, const vamd_batch_desc *desc, const vamd_batch_io *io, int level) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  int r = check_desc(c, desc, io);
  if (r) return r;
  if (level < VAMD_LEVEL_TRANSFORM || level > VAMD_LEVEL_FULL) return fail(c, VAMD_EINVAL, "bad level");
  return run_batch(c, desc, io, level, false, nullptr);
}

// ---- the decoder's back half (k_synth.h): vb->pcm per block, the streams' decoded samples ----
static size_t synth_lds_bytes(const vamd_ctx *c, int W) {
  return synth_lds_words(c->B.channels, c->B.bs[W] / 2, c->B.channels, c->B.res_off_ints[W]) * 4;
}
// what k_synth needs of a size class's setup beyond the residue back-end: floors it can draw the decoder's way, and a
// workgroup's LDS for the block's spectrum and a butterfly vector per channel
static int synth_covered(vamd_ctx *c, int W, SynthFloorP *S) {
  int r = res_covered(c, W);
  if (r) return r;
  const int ch = c->B.channels, n2 = c->B.bs[W] / 2;
  if (!synth_floor_ranges(c->B.floor[W][0], c->B.floor[W][1], c->B.chmap[W].submaps, n2, S))
    return fail(c, VAMD_EIMPL, "synthesis: a floor of more than two posts whose range is no power of two (a decoder rebuilds the range from its bit count, lib/floor1.c:160)");
  if (synth_lds_bytes(c, W) > c->lds_per_block)
    return fail(c, VAMD_EIMPL, "synthesis: a block's spectrum and butterfly vectors do not fit a workgroup's LDS");
  return VAMD_OK;
}
// k_synth over y's blocks of size class W -- what the last run left (vamd_ctx::synth_src), or the rows k_unpack wrote
// (vamd_decode.h) -- on the context's stream.  bounded: the rows are k_unpack_partial's (res_count[1] = the entries read)
static int launch_synth(vamd_ctx *c, int W, const vamd_ctx::SynthSrc &y, float *synth, bool bounded) {
  SynthFloorP S;
  int r = synth_covered(c, W, &S);
  if (r) return r;
  if (y.nb < 1) return VAMD_OK;
  const int ch = c->B.channels, n2 = c->B.bs[W] / 2;
  if (bounded && c->V.values)
    hipLaunchKernelGGL(k_synth_values_bounded, dim3((unsigned)y.nb), dim3(64 * ch), synth_lds_bytes(c, W), c->stream,
                       c->B.xf[W], c->B.res[W][0], c->B.res[W][1], c->B.chmap[W], c->B.couple[W], S, ch, c->B.res_cap[W], c->B.res_off_ints[W],
                       c->d_dbg ? c->d_dbg + 8 : nullptr, y.post_valid, y.ilogmask, y.res_class, y.res_entries, y.res_count, synth, c->V);
  else if (bounded)
    hipLaunchKernelGGL(k_synth_bounded, dim3((unsigned)y.nb), dim3(64 * ch), synth_lds_bytes(c, W), c->stream,
                       c->B.xf[W], c->B.res[W][0], c->B.res[W][1], c->B.chmap[W], c->B.couple[W], S, ch, c->B.res_cap[W], c->B.res_off_ints[W],
                       c->d_dbg ? c->d_dbg + 8 : nullptr, y.post_valid, y.ilogmask, y.res_class, y.res_entries, y.res_count, synth);
  else if (c->V.values)  // (a header-made setup with a residue book that is no lattice book: vamd_ctx::V)
    hipLaunchKernelGGL(k_synth_values, dim3((unsigned)y.nb), dim3(64 * ch), synth_lds_bytes(c, W), c->stream,
                       c->B.xf[W], c->B.res[W][0], c->B.res[W][1], c->B.chmap[W], c->B.couple[W], S, ch, c->B.res_cap[W], c->B.res_off_ints[W],
                       c->d_dbg ? c->d_dbg + 8 : nullptr, y.post_valid, y.ilogmask, y.res_class, y.res_entries, y.res_count, synth, c->V);
  else
    hipLaunchKernelGGL(k_synth, dim3((unsigned)y.nb), dim3(64 * ch), synth_lds_bytes(c, W), c->stream,
                       c->B.xf[W], c->B.res[W][0], c->B.res[W][1], c->B.chmap[W], c->B.couple[W], S, ch, c->B.res_cap[W], c->B.res_off_ints[W],
                       c->d_dbg ? c->d_dbg + 8 : nullptr, y.post_valid, y.ilogmask, y.res_class, y.res_entries, y.res_count, synth);
  HIP_TRY(c, hipGetLastError());
  return VAMD_OK;
}

int vamd_synth_check(vamd_ctx *c, int W) {
  if (!c || (W != 0 && W != 1)) return VAMD_EINVAL;
  SynthFloorP S;
  return synth_covered(c, W, &S);
}

int vamd_analyze_batch_synth(vamd_ctx *c, const vamd_batch_desc *desc, const vamd_batch_io *io, float *synth) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  int r = check_desc(c, desc, io);
  if (r) return r;
  SynthFloorP S;
  if ((r = synth_covered(c, desc->W, &S))) return r;
  if (!synth && desc->nblocks) return fail(c, VAMD_EINVAL, "null synth buffer");
  if (!desc->nblocks) return run_batch(c, desc, io, VAMD_LEVEL_FULL, false, nullptr);
  return run_batch(c, desc, io, VAMD_LEVEL_FULL, false, nullptr, nullptr, synth);
}

int vamd_synth_streams(vamd_ctx *c, const vamd_stream_plan *plan, long nstreams, long max_frames, const int64_t *frames,
                       const int64_t *offset, float *scratch_short, float *scratch_long, float *pcm) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!plan || nstreams < 1 || plan->nstreams != nstreams || max_frames < 1 || !frames || !offset || !pcm)
    return fail(c, VAMD_EINVAL, "plan / max_frames / frames / offset / pcm");
  float *scratch[2] = {scratch_short, scratch_long};
  for (int W = 0; W < 2; W++) {
    if (!plan->nblocks[W]) continue;
    if (!scratch[W]) return fail(c, VAMD_EINVAL, "null scratch for a size class with blocks");
    if (c->synth_src[W].nb != (long)plan->nblocks[W])
      return fail(c, VAMD_EINVAL, "vamd_synth_streams: the context's last analysis is not the plan's (a VBR vamd_analyze_streams_mixed with packets or residue outputs)");
    int r = launch_synth(c, W, c->synth_src[W], scratch[W]);
    if (r) return r;
  }
  LapP L;
  L.ch = c->B.channels, L.bs0 = c->B.bs[0], L.bs1 = c->B.bs[1];
  L.win0 = c->B.xf[0].win_short, L.win1 = c->B.xf[0].win_long;
  L.order = plan->order, L.stream_start = (const long long *)plan->stream_start;
  L.src0 = (const long long *)plan->src[0], L.src1 = (const long long *)plan->src[1];
  L.synth0 = scratch_short, L.synth1 = scratch_long;
  const long per_stream = (max_frames + 1023) / 1024;  // workgroups a stream: four frames a thread, at most 1024 of them (the kernel strides)
  hipLaunchKernelGGL(k_lap, dim3((unsigned)(per_stream < 1024 ? per_stream : 1024), (unsigned)(nstreams < 1024 ? nstreams : 1024)), dim3(256), 0, c->stream, L, nstreams,
                     (const long long *)frames, (const long long *)offset, pcm);
  HIP_TRY(c, hipGetLastError());
  return VAMD_OK;
}

// a bitrate-managed call's outputs, of size class W
static int check_managed(vamd_ctx *c, int W, const vamd_managed_io *m) {
  if (!m || !m->posts || !m->post_valid || !m->iwork || !m->nonzero)
    return fail(c, VAMD_EINVAL, "managed outputs posts / post_valid / iwork / nonzero are required");
  if (m->res_class || m->res_entries || m->res_count) {
    if (!(m->res_class && m->res_entries && m->res_count))
      return fail(c, VAMD_EINVAL, "res_class / res_entries / res_count go together");
    int r = res_covered(c, W);
    if (r) return r;
  }
  if (m->packets || m->packet_bits) return check_packets(c, W, VAMD_LEVEL_FULL, m->packets, m->packet_bits, m->packet_stride);
  return VAMD_OK;
}
// ... and what its VBR io keeps: the per-candidate fields do not apply
static vamd_batch_io shared_io(const vamd_batch_io &io) {
  vamd_batch_io shared = io;
  shared.packets = nullptr;
  shared.packet_bits = nullptr;
  shared.posts = shared.post_valid = shared.ilogmask = shared.iwork = shared.nonzero = nullptr;
  shared.res_class = nullptr;
  shared.res_entries = nullptr;
  shared.res_count = nullptr;
  return shared;
}

int vamd_analyze_batch_managed(vamd_ctx *c, const vamd_batch_desc *desc, const vamd_batch_io *io,
                               const vamd_managed_io *m) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  int r = check_desc(c, desc, io);
  if (r) return r;
  if ((r = check_managed(c, desc->W, m))) return r;
  const vamd_batch_io shared = shared_io(*io);
  return run_batch(c, desc, &shared, VAMD_LEVEL_FULL, false, nullptr, m);
}

int vamd_analyze_stream(vamd_ctx *c, const vamd_batch_desc *desc, const vamd_batch_io *io, float *ampmax_state) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  int r = check_desc(c, desc, io);
  if (r) return r;
  if (!ampmax_state) return fail(c, VAMD_EINVAL, "null ampmax_state");
  return run_batch(c, desc, io, VAMD_LEVEL_FULL, true, ampmax_state);
}

// the two-size-class stream run; nstreams == 0: one stream whose state is the host float *ampmax_state,
// otherwise `stream_start` [nstreams+1] and `states` [nstreams] are device arrays
static int run_streams_mixed(vamd_ctx *c, const vamd_batch_desc *desc_short, const vamd_batch_io *io_short,
                             const vamd_batch_desc *desc_long, const vamd_batch_io *io_long, const int32_t *order,
                             long nblocks_total, float *ampmax_state, const int64_t *stream_start, long nstreams,
                             float *states, bool first_given = false, const vamd_managed_io *M0 = nullptr,
                             const vamd_managed_io *M1 = nullptr) {
  if (desc_short->W != 0 || desc_long->W != 1) return fail(c, VAMD_EINVAL, "desc_short->W must be 0, desc_long->W 1");
  if (nblocks_total != desc_short->nblocks + desc_long->nblocks || (nblocks_total && !order))
    return fail(c, VAMD_EINVAL, "order[] must name every block of both batches exactly once");
  int r;
  if (desc_short->nblocks && (r = check_desc(c, desc_short, io_short))) return r;
  if (desc_long->nblocks && (r = check_desc(c, desc_long, io_long))) return r;
  if (nblocks_total == 0) return VAMD_OK;
  c->roads[0][0] = c->roads[1][0] = 0;  // (the record of what this call launches: vamd_launch_record)
  BatchRun R[2];
  if ((r = prepare_run(c, desc_short, io_short, VAMD_LEVEL_FULL, &R[0], M0))) return r;
  if ((r = prepare_run(c, desc_long, io_long, VAMD_LEVEL_FULL, &R[1], M1))) return r;
  // scratch for the chained state; an empty size class still needs valid (unused) pointers
  void *misc = nullptr;
  if ((r = ws_get(c, 0, vamd_ctx::WS_MISC, 256, &misc))) return r;
  float *d_state = (float *)misc;
  for (int W = 0; W < 2; W++)
    if (R[W].nb == 0) R[W].p.ampin = R[W].p.ampglob = R[W].p.local = (float *)misc + 16;
  hipStream_t s = c->stream;
  launch_transform(c, &R[0]);
  launch_transform(c, &R[1]);
  const float secs0 = (float)(c->B.bs[0] / 2) / (float)c->B.rate, secs1 = (float)(c->B.bs[1] / 2) / (float)c->B.rate;
  // The chains' walk (a wave per stream) feeds the tone
  // seeds and nothing else of the masking stage, so where the tone chain runs on the side stream the walk goes there
  // too, ahead of it, and the noise masks start at once on the main stream.
  const bool chain_on_side = nstreams && c->overlap && (R[0].nb == 0 || R[0].nb * c->B.channels > 64) &&
                             (R[1].nb == 0 || R[1].nb * c->B.channels > 64);
  if (chain_on_side) {
    (void)hipEventRecord(c->ev_fork, c->stream);
    (void)hipStreamWaitEvent(c->side, c->ev_fork, 0);
    s = c->side;
  }
  if (nstreams)
    hipLaunchKernelGGL(k_ampmax_streams_mixed, dim3((unsigned)nstreams), dim3(64), 0, s, c->B.channels, nstreams,
                       (const long long *)stream_start, (const int *)order, secs0, secs1, c->B.ampmax_att_per_sec, states,
                       R[0].p.local, R[1].p.local, R[0].p.ampin, R[1].p.ampin, R[0].p.ampglob, R[1].p.ampglob);
  else
    hipLaunchKernelGGL(k_ampmax_stream_mixed, dim3(1), dim3(64), 0, s, c->B.channels, nblocks_total, (const int *)order, secs0,
                       secs1, c->B.ampmax_att_per_sec, *ampmax_state, R[0].p.local, R[1].p.local, R[0].p.ampin,
                       R[1].p.ampin, R[0].p.ampglob, R[1].p.ampglob, d_state, first_given ? 1 : 0);
  s = c->stream;
  prof_mark(c, VAMD_ST_AMPMAX);
  R[0].d.ampmax_in = R[0].p.ampin;
  R[1].d.ampmax_in = R[1].p.ampin;
  if (chain_on_side) {  // both classes' masks first, the long blocks' leading
    launch_masks(c, &R[1], VAMD_LEVEL_FULL, true, R[0].nb == 0);
    launch_masks(c, &R[0], VAMD_LEVEL_FULL, true, R[1].nb == 0);
    launch_floor_on(c, &R[1], VAMD_LEVEL_FULL);
    launch_floor_on(c, &R[0], VAMD_LEVEL_FULL);
  } else {
    launch_masks(c, &R[0], VAMD_LEVEL_FULL, false, R[1].nb == 0);
    launch_floor_on(c, &R[0], VAMD_LEVEL_FULL);
    launch_masks(c, &R[1], VAMD_LEVEL_FULL, false, R[0].nb == 0);
    launch_floor_on(c, &R[1], VAMD_LEVEL_FULL);
  }
  if (chain_on_side && R[0].nb == 0 && R[1].nb == 0) {  // (cannot happen -- nblocks_total > 0 -- but nothing may be left unjoined)
    (void)hipEventRecord(c->ev_join, c->side);
    (void)hipStreamWaitEvent(c->stream, c->ev_join, 0);
  }
  if (c->profile) c->prof_runs++;
  HIP_TRY(c, hipGetLastError());
  if (!nstreams) {
    HIP_TRY(c, hipMemcpyAsync(ampmax_state, d_state, sizeof(float), hipMemcpyDeviceToHost, s));
    HIP_TRY(c, hipStreamSynchronize(s));
  }
  return VAMD_OK;
}

int vamd_analyze_stream_mixed(vamd_ctx *c, const vamd_batch_desc *desc_short, const vamd_batch_io *io_short,
                              const vamd_batch_desc *desc_long, const vamd_batch_io *io_long, const int32_t *order,
                              long nblocks_total, float *ampmax_state) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!desc_short || !desc_long || !ampmax_state) return fail(c, VAMD_EINVAL, "null argument");
  return run_streams_mixed(c, desc_short, io_short, desc_long, io_long, order, nblocks_total, ampmax_state, nullptr, 0, nullptr);
}

int vamd_analyze_streams_mixed(vamd_ctx *c, const vamd_batch_desc *desc_short, const vamd_batch_io *io_short,
                               const vamd_batch_desc *desc_long, const vamd_batch_io *io_long, const int32_t *order,
                               const int64_t *stream_start, long nstreams, long nblocks_total, float *ampmax_states) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!desc_short || !desc_long) return fail(c, VAMD_EINVAL, "null argument");
  if (nstreams < 1 || !stream_start || !ampmax_states) return fail(c, VAMD_EINVAL, "stream_start / ampmax_states / nstreams");
  return run_streams_mixed(c, desc_short, io_short, desc_long, io_long, order, nblocks_total, nullptr, stream_start, nstreams,
                           ampmax_states);
}

int vamd_analyze_streams_mixed_managed(vamd_ctx *c, const vamd_batch_desc *desc_short, const vamd_batch_io *io_short,
                                       const vamd_managed_io *m_short, const vamd_batch_desc *desc_long,
                                       const vamd_batch_io *io_long, const vamd_managed_io *m_long, const int32_t *order,
                                       const int64_t *stream_start, long nstreams, long nblocks_total, float *ampmax_states) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!desc_short || !desc_long) return fail(c, VAMD_EINVAL, "null argument");
  if (nstreams < 1 || !stream_start || !ampmax_states) return fail(c, VAMD_EINVAL, "stream_start / ampmax_states / nstreams");
  const vamd_managed_io *m[2] = {m_short, m_long};
  const vamd_batch_desc *d[2] = {desc_short, desc_long};
  vamd_batch_io shared[2];
  const vamd_batch_io *io[2] = {io_short, io_long};
  for (int W = 0; W < 2; W++) {
    memset(&shared[W], 0, sizeof(shared[W]));
    if (!d[W]->nblocks) continue;
    if (!io[W]) return fail(c, VAMD_EINVAL, "null io of a size class with blocks");
    int r = check_managed(c, W, m[W]);
    if (r) return r;
    shared[W] = shared_io(*io[W]);
  }
  return run_streams_mixed(c, desc_short, &shared[0], desc_long, &shared[1], order, nblocks_total, nullptr, stream_start, nstreams,
                           ampmax_states, false, desc_short->nblocks ? m_short : nullptr, desc_long->nblocks ? m_long : nullptr);
}

int vamd_bitrate_init_states(vamd_ctx *c, vamd_bitrate_state *states, long nstreams) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!c->B.has_bitrate) return fail(c, VAMD_EIMPL, "the setup blob carries no bitrate manager (a VBR setup, or one packed without the section)");
  if (nstreams < 1 || !states) return fail(c, VAMD_EINVAL, "states / nstreams");
  hipLaunchKernelGGL(k_bitrate_init, dim3((unsigned)((nstreams + 255) / 256)), dim3(256), 0, c->stream, c->B.bitrate, nstreams, states);
  HIP_TRY(c, hipGetLastError());
  return VAMD_OK;
}

int vamd_bitrate_walk(vamd_ctx *c, const int32_t *order, const int64_t *stream_start, long nstreams,
                      const int32_t *const packet_bits[2], const uint8_t *const status[2], vamd_bitrate_state *states,
                      int32_t *const choice[2], int32_t *const final_bits[2]) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!c->B.has_bitrate) return fail(c, VAMD_EIMPL, "the setup blob carries no bitrate manager (a VBR setup, or one packed without the section)");
  if (nstreams < 1 || !order || !stream_start || !states || !packet_bits || !choice || !final_bits)
    return fail(c, VAMD_EINVAL, "order / stream_start / states / packet_bits / choice / final_bits / nstreams");
  // (a size class without blocks may pass NULL arrays: order[] never names one of its blocks)
  hipLaunchKernelGGL(k_bitrate_walk, dim3((unsigned)((nstreams + 63) / 64)), dim3(64), 0, c->stream, c->B.bitrate, c->B.bs[0] >> 1,
                     c->B.bs[1] >> 1, c->B.channels, nstreams, (const long long *)stream_start, (const int *)order,
                     (const int *)packet_bits[0], (const int *)packet_bits[1], status ? status[0] : nullptr,
                     status ? status[1] : nullptr, states, (int *)choice[0], (int *)choice[1], (int *)final_bits[0],
                     (int *)final_bits[1]);
  HIP_TRY(c, hipGetLastError());
  return VAMD_OK;
}

#undef VAMD_SWITCH_LOGN
#undef VAMD_SWITCH_BINS
