// vamd_block.h -- the host-pointer calls of the C ABI, a block (or a look-ahead's few) at a time: the caller's samples go
// through a pinned arena of the context's to the batch calls of vamd_batch.h, the results come back the same way.  Part of
// the library's single translation unit: included by vamd_hip.hip, once, after vamd_plan.h.
#pragma once
// one block with uniform lW / nW / blocktype / ampmax_in
static vamd_batch_desc one_block_desc(int W, int lW, int nW, int blocktype, float ampmax_in) {
  vamd_batch_desc d;
  memset(&d, 0, sizeof(d));
  d.W = W;
  d.nblocks = 1;
  d.uniform_lW = lW;
  d.uniform_nW = nW;
  d.uniform_blocktype = blocktype;
  d.uniform_ampmax_in = ampmax_in;
  return d;
}

// the caller's channel pointers: none may be null; `bytes` of each into the arena, one behind the other
static int channels_given(vamd_ctx *c, const float *const *pcm, size_t ch) {
  for (size_t i = 0; i < ch; i++)
    if (!pcm[i]) return fail(c, VAMD_EINVAL, "null channel pointer");
  return VAMD_OK;
}
static int stage_channels(vamd_ctx *c, unsigned char *dst, const float *const *pcm, size_t ch, size_t bytes) {
  int r = channels_given(c, pcm, ch);
  for (size_t i = 0; !r && i < ch; i++) memcpy(dst + i * bytes, pcm[i], bytes);
  return r;
}

// (test knob: a GPU failure under a call, for the binding's error path -- from the `after`-th call on, by the call
// site's own count)
static int injected_failure(vamd_ctx *c, long after, std::atomic<long> &calls, const char *knob) {
  if (after < 0 || calls.fetch_add(1) < after) return VAMD_OK;
  return fail(c, VAMD_EFAULT, (std::string("injected failure (") + knob + ")").c_str());
}

// device row length of a packet: the caller's stride, or the longest packet where that is shorter
static size_t packet_row(const vamd_ctx *c, int W, long packet_stride) {
  const size_t cap = (size_t)c->B.pack[W].capacity;
  return cap < (size_t)packet_stride ? cap : ((size_t)packet_stride & ~(size_t)3);
}
// K packets out of the arena (`bits`, rows of `row` bytes) into the caller's arrays; bytes_too: and their bytes
static void copy_out_packets(const int32_t *bits, const unsigned char *rows, size_t row, size_t K, int32_t *packet_bits,
                             uint8_t *packets, size_t packet_stride, bool bytes_too) {
  for (size_t k = 0; k < K; k++) {
    packet_bits[k] = bits[k];
    size_t bytes = ((size_t)(bits[k] > 0 ? bits[k] : 0) + 7) / 8;
    if (bytes > row) bytes = row;  // (cut off: packet_bits says so)
    if (bytes_too) memcpy(packets + k * packet_stride, rows + k * row, bytes);
  }
}

int vamd_analyze_block_managed(vamd_ctx *c, const float *const *pcm, int lW, int W, int nW, int blocktype,
                               float ampmax_in, float *mdct, float *ampmax_out, int32_t *posts,
                               int32_t *post_valid, int32_t *iwork, int32_t *nonzero, int32_t *res_class,
                               uint16_t *res_entries, int32_t *res_count) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!pcm || (W != 0 && W != 1)) return fail(c, VAMD_EINVAL, "bad pcm / W");
  const bool want_res = res_class || res_entries || res_count;
  int r;
  if (want_res && (r = res_covered(c, W))) return r;
  const size_t rcap = want_res ? (size_t)c->B.res_cap[W] : 0;
  const size_t S = (size_t)c->B.chmap[W].submaps;
  const size_t ch = c->B.channels, n = c->B.bs[W], n2 = n / 2, K = VAMD_PACKETBLOBS;
  Arena A;
  const size_t o_pcm = A.take(ch * n * 4), o_mdct = A.take(ch * n2 * 4), o_amp = A.take(16),
               o_posts = A.take(K * ch * VAMD_POSTS_STRIDE * 4), o_valid = A.take(K * ch * 4), o_nz = A.take(K * ch * 4),
               o_iwork = A.take(K * ch * n2 * 4), o_rcls = A.take(want_res ? K * S * VAMD_RES_CLASS_STRIDE * 4 : 0),
               o_rcnt = A.take(want_res ? K * S * 2 * 4 : 0), o_rent = A.take(K * rcap * 2), total = A.at;
  if ((r = pinned_get(c, c->h_stage, total, false))) return r;
  void *dv;
  if ((r = ws_get(c, W, vamd_ctx::WS_M_STAGE, total, &dv))) return r;
  unsigned char *hs = (unsigned char *)c->h_stage.p, *ds = (unsigned char *)dv;
  if ((r = stage_channels(c, hs + o_pcm, pcm, ch, n * 4))) return r;
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(ds + o_pcm, hs + o_pcm, ch * n * 4, hipMemcpyHostToDevice, s));
  const vamd_batch_desc d = one_block_desc(W, lW, nW, blocktype, ampmax_in);
  vamd_batch_io io;
  memset(&io, 0, sizeof(io));
  io.pcm = (const float *)(ds + o_pcm);
  io.mdct = (float *)(ds + o_mdct);
  io.ampmax_out = (float *)(ds + o_amp);
  io.status = ds + o_amp + 4;
  vamd_managed_io m;
  memset(&m, 0, sizeof(m));
  m.posts = (int32_t *)(ds + o_posts);
  m.post_valid = (int32_t *)(ds + o_valid);
  m.nonzero = (int32_t *)(ds + o_nz);
  m.iwork = (int32_t *)(ds + o_iwork);
  if (want_res) {
    m.res_class = (int32_t *)(ds + o_rcls);
    m.res_count = (int32_t *)(ds + o_rcnt);
    m.res_entries = (uint16_t *)(ds + o_rent);
  }
  r = vamd_analyze_batch_managed(c, &d, &io, &m);
  if (r) return r;
  HIP_TRY(c, hipMemcpyAsync(hs + o_mdct, ds + o_mdct, total - o_mdct, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (ampmax_out) memcpy(ampmax_out, hs + o_amp, 4);  // (the block's ampmax comes out of its FFT: delivered with a domain error too)
  if ((r = status_verdict(c, hs + o_amp + 4, ch))) return r;
  if (mdct) memcpy(mdct, hs + o_mdct, ch * n2 * 4);
  if (posts) memcpy(posts, hs + o_posts, K * ch * VAMD_POSTS_STRIDE * 4);
  if (post_valid) memcpy(post_valid, hs + o_valid, K * ch * 4);
  if (nonzero) memcpy(nonzero, hs + o_nz, K * ch * 4);
  if (iwork) memcpy(iwork, hs + o_iwork, K * ch * n2 * 4);
  if (want_res) {
    if (res_class) memcpy(res_class, hs + o_rcls, K * S * VAMD_RES_CLASS_STRIDE * 4);
    if (res_count) memcpy(res_count, hs + o_rcnt, K * S * 2 * 4);
    if (res_entries) memcpy(res_entries, hs + o_rent, K * rcap * 2);
  }
  return VAMD_OK;
}

int vamd_analyze_block(vamd_ctx *c, const float *const *pcm, int lW, int W, int nW, int blocktype, float ampmax_in,
                       float *mdct, float *logmask, int32_t *posts, int32_t *post_valid, int32_t *iwork,
                       int32_t *nonzero, float *ampmax_out) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  return vamd_analyze_block_res(c, pcm, lW, W, nW, blocktype, ampmax_in, mdct, logmask, posts, post_valid, iwork,
                                nonzero, ampmax_out, nullptr, nullptr, nullptr);
}

int vamd_analyze_block_res(vamd_ctx *c, const float *const *pcm, int lW, int W, int nW, int blocktype,
                           float ampmax_in, float *mdct, float *logmask, int32_t *posts, int32_t *post_valid,
                           int32_t *iwork, int32_t *nonzero, float *ampmax_out, int32_t *res_class,
                           uint16_t *res_entries, int32_t *res_count) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!pcm || (W != 0 && W != 1)) return fail(c, VAMD_EINVAL, "bad pcm / W");
  const bool want_res = res_class || res_entries || res_count;
  int r;
  if (want_res && (r = res_covered(c, W))) return r;
  const size_t rcap = want_res ? (size_t)c->B.res_cap[W] : 0;
  const size_t S = (size_t)c->B.chmap[W].submaps;
  const int ch = c->B.channels, n = c->B.bs[W], n2 = n / 2;
  // one pinned + one device arena: [pcm | mdct | logmask | iwork | posts | post_valid | nonzero | ampmax]
  Arena A;
  const size_t o_pcm = A.take((size_t)ch * n * 4), o_mdct = A.take((size_t)ch * n2 * 4), o_mask = A.take((size_t)ch * n2 * 4),
               o_iwork = A.take((size_t)ch * n2 * 4), o_posts = A.take((size_t)ch * VAMD_POSTS_STRIDE * 4),
               o_valid = A.take((size_t)ch * 4), o_nz = A.take((size_t)ch * 4), o_amp = A.take(16),
               o_rcls = A.take(S * VAMD_RES_CLASS_STRIDE * 4), o_rcnt = A.take(S * 8), o_rent = A.take(rcap * 2), total = A.at;
  if ((r = pinned_get(c, c->h_stage, total, false))) return r;
  void *dv;
  if ((r = ws_get(c, W, vamd_ctx::WS_PCM, total, &dv))) return r;
  unsigned char *hs = (unsigned char *)c->h_stage.p, *ds = (unsigned char *)dv;
  if ((r = stage_channels(c, hs + o_pcm, pcm, (size_t)ch, (size_t)n * 4))) return r;
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(ds + o_pcm, hs + o_pcm, (size_t)ch * n * 4, hipMemcpyHostToDevice, s));
  const vamd_batch_desc d = one_block_desc(W, lW, nW, blocktype, ampmax_in);
  vamd_batch_io io;
  memset(&io, 0, sizeof(io));
  io.pcm = (const float *)(ds + o_pcm);
  io.mdct = (float *)(ds + o_mdct);
  io.logmask = (float *)(ds + o_mask);
  io.iwork = (int32_t *)(ds + o_iwork);
  io.posts = (int32_t *)(ds + o_posts);
  io.post_valid = (int32_t *)(ds + o_valid);
  io.nonzero = (int32_t *)(ds + o_nz);
  io.ampmax_out = (float *)(ds + o_amp);
  io.status = ds + o_amp + 4;  // ch <= 8 bytes behind the float, inside its 16-byte slot
  if (want_res) {
    io.res_class = (int32_t *)(ds + o_rcls);
    io.res_count = (int32_t *)(ds + o_rcnt);
    io.res_entries = (uint16_t *)(ds + o_rent);
  }
  r = vamd_analyze_batch(c, &d, &io, VAMD_LEVEL_FULL);
  if (r) return r;
  HIP_TRY(c, hipMemcpyAsync(hs + o_mdct, ds + o_mdct, total - o_mdct, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (ampmax_out) memcpy(ampmax_out, hs + o_amp, 4);  // (the block's ampmax comes out of its FFT: delivered with a domain error too)
  if ((r = status_verdict(c, hs + o_amp + 4, (size_t)ch))) return r;
  if (mdct) memcpy(mdct, hs + o_mdct, (size_t)ch * n2 * 4);
  if (logmask) memcpy(logmask, hs + o_mask, (size_t)ch * n2 * 4);
  if (iwork) memcpy(iwork, hs + o_iwork, (size_t)ch * n2 * 4);
  if (posts) memcpy(posts, hs + o_posts, (size_t)ch * VAMD_POSTS_STRIDE * 4);
  if (post_valid) memcpy(post_valid, hs + o_valid, (size_t)ch * 4);
  if (nonzero) memcpy(nonzero, hs + o_nz, (size_t)ch * 4);
  if (want_res) {
    if (res_count) memcpy(res_count, hs + o_rcnt, S * 8);
    if (res_class) memcpy(res_class, hs + o_rcls, S * VAMD_RES_CLASS_STRIDE * 4);
    if (res_entries) memcpy(res_entries, hs + o_rent, rcap * 2);
  }
  return VAMD_OK;
}

int vamd_encode_block(vamd_ctx *c, const float *const *pcm, int lW, int W, int nW, int blocktype, float ampmax_in,
                      int managed, float *ampmax_out, uint8_t *packets, long packet_stride, int32_t *packet_bits) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!pcm || (W != 0 && W != 1)) return fail(c, VAMD_EINVAL, "bad pcm / W");
  if (!packets || !packet_bits) return fail(c, VAMD_EINVAL, "null packets / packet_bits");
  int r;
  if ((r = packets_assembled(c, W))) return r;
  if (packet_stride < 4) return fail(c, VAMD_EINVAL, "packet_stride too small");
  static std::atomic<long> calls{0};
  if ((r = injected_failure(c, c->K.fail_encode_after, calls, "VAMD_FAIL_ENCODE_AFTER"))) return r;
  const size_t ch = c->B.channels, n = c->B.bs[W], n2 = n / 2, K = managed ? VAMD_PACKETBLOBS : 1;
  const size_t row = packet_row(c, W, packet_stride);
  // one pinned + one device arena: [pcm | ampmax | bits | packets || the managed candidates' intermediates]
  Arena A;
  const size_t o_pcm = A.take(ch * n * 4), o_amp = A.take(16), o_bits = A.take(K * 4), o_pk = A.take(K * row), o_back = A.at,
               o_posts = A.take(K * ch * VAMD_POSTS_STRIDE * 4), o_valid = A.take(K * ch * 4), o_nz = A.take(K * ch * 4),
               o_iwork = A.take(K * ch * n2 * 4), total = managed ? A.at : o_back;
  if ((r = pinned_get(c, c->h_stage, o_back, false))) return r;
  void *dv;
  if ((r = ws_get(c, W, managed ? vamd_ctx::WS_M_STAGE : vamd_ctx::WS_PCM, total, &dv))) return r;
  unsigned char *hs = (unsigned char *)c->h_stage.p, *ds = (unsigned char *)dv;
  if ((r = stage_channels(c, hs + o_pcm, pcm, ch, n * 4))) return r;
  hipStream_t s = c->stream;
  // The kernels read the samples out of, and write the packet into, the pinned arena itself (it is mapped into the
  // device's address space): 16 KB in and a few hundred bytes out per block cross the link inside the first and the
  // last kernel instead of as two copy commands either side of them.  VAMD_STAGE_COPIES=1 brings the copies back
  // (measurement aid).
  const bool staged_copies = c->K.stage_copies;
  unsigned char *io_base = ds;
  if (!staged_copies) {
    void *mapped = nullptr;
    HIP_TRY(c, hipHostGetDevicePointer(&mapped, hs, 0));
    io_base = (unsigned char *)mapped;
  } else {
    HIP_TRY(c, hipMemcpyAsync(ds + o_pcm, hs + o_pcm, ch * n * 4, hipMemcpyHostToDevice, s));
  }
  const vamd_batch_desc d = one_block_desc(W, lW, nW, blocktype, ampmax_in);
  vamd_batch_io io;
  memset(&io, 0, sizeof(io));
  io.pcm = (const float *)(io_base + o_pcm);
  io.ampmax_out = (float *)(io_base + o_amp);
  io.status = io_base + o_amp + 4;  // ch <= 8 bytes behind the float, inside its 16-byte slot
  if (managed) {
    vamd_managed_io m;
    memset(&m, 0, sizeof(m));
    m.posts = (int32_t *)(ds + o_posts);
    m.post_valid = (int32_t *)(ds + o_valid);
    m.nonzero = (int32_t *)(ds + o_nz);
    m.iwork = (int32_t *)(ds + o_iwork);
    m.packets = io_base + o_pk;
    m.packet_bits = (int32_t *)(io_base + o_bits);
    m.packet_stride = (int64_t)row;
    r = vamd_analyze_batch_managed(c, &d, &io, &m);
  } else {
    io.packets = io_base + o_pk;
    io.packet_bits = (int32_t *)(io_base + o_bits);
    io.packet_stride = (int64_t)row;
    r = vamd_analyze_batch(c, &d, &io, VAMD_LEVEL_FULL);
  }
  if (r) return r;
  if (staged_copies) HIP_TRY(c, hipMemcpyAsync(hs + o_amp, ds + o_amp, o_back - o_amp, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (ampmax_out) memcpy(ampmax_out, hs + o_amp, 4);  // (the block's ampmax comes out of its FFT: delivered with a domain error too)
  if ((r = status_verdict(c, hs + o_amp + 4, ch))) return r;
  copy_out_packets((const int32_t *)(hs + o_bits), hs + o_pk, row, K, packet_bits, packets, (size_t)packet_stride, true);
  return VAMD_OK;
}

// N consecutive blocks of ONE stream from host memory to their packets in one launch sequence (the binding's look-ahead,
// integration/mapping0_vamd.c): what vamd_encode_block does for one block, with the ampmax chain between them on the device.
int vamd_encode_blocks(vamd_ctx *c, long nblocks, const float *const *pcm, const int32_t *lW, const int32_t *W,
                       const int32_t *nW, const int32_t *blocktype, float ampmax_in_first, int managed, float *ampmax_in,
                       float *ampmax_out, uint8_t *packets, long packet_stride, int32_t *packet_bits, int32_t *verdict) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (nblocks < 0 || nblocks > 0x3fffffffL) return fail(c, VAMD_EINVAL, "nblocks out of range");
  if (nblocks == 0) return VAMD_OK;
  if (!pcm || !lW || !W || !nW || !blocktype || !packets || !packet_bits || !verdict) return fail(c, VAMD_EINVAL, "null argument");
  if (packet_stride < 4) return fail(c, VAMD_EINVAL, "packet_stride too small");
  const size_t ch = c->B.channels;
  int r;
  if ((r = packets_assembled(c, 0)) || (r = packets_assembled(c, 1))) return r;
  static std::atomic<long> calls{0};  // (this call's own count, not vamd_encode_block's)
  if ((r = injected_failure(c, c->K.fail_encode_after, calls, "VAMD_FAIL_ENCODE_AFTER"))) return r;
  long nb[2] = {0, 0};
  for (long b = 0; b < nblocks; b++) {
    if (W[b] != 0 && W[b] != 1) return fail(c, VAMD_EINVAL, "W must be 0 or 1");
    if ((lW[b] & ~1) || (nW[b] & ~1) || (blocktype[b] & ~1)) return fail(c, VAMD_EINVAL, "lW / nW / blocktype must be 0 or 1");
    if ((r = channels_given(c, pcm + b * ch, ch))) return r;
    nb[W[b]]++;
  }
  const size_t K = managed ? VAMD_PACKETBLOBS : 1;  // packets per block: one, or a bitrate-managed block's fifteen candidates
  // one pinned arena, read and written in place by the kernels (mapped): per size class [pcm | lW | nW | blocktype |
  // ampmax_out | bits | status | packets], then the stream order
  size_t o_pcm[2], o_lW[2], o_nW[2], o_bt[2], o_amp[2], o_bits[2], o_st[2], o_pk[2], row[2];
  Arena A;
  for (int w = 0; w < 2; w++) {
    const size_t n = c->B.bs[w];
    row[w] = packet_row(c, w, packet_stride);
    o_pcm[w] = A.take((size_t)nb[w] * ch * n * 4);
    o_lW[w] = A.take((size_t)nb[w] * 4);
    o_nW[w] = A.take((size_t)nb[w] * 4);
    o_bt[w] = A.take((size_t)nb[w] * 4);
    o_amp[w] = A.take((size_t)nb[w] * 4);
    o_bits[w] = A.take((size_t)nb[w] * K * 4);
    o_st[w] = A.take((size_t)nb[w] * ch);
    o_pk[w] = A.take((size_t)nb[w] * K * row[w]);
  }
  const size_t o_order = A.take((size_t)nblocks * 4), total = A.at;
  if ((r = pinned_get(c, c->h_stage, total, true))) return r;
  unsigned char *hs = (unsigned char *)c->h_stage.p;
  void *mapped = nullptr;
  HIP_TRY(c, hipHostGetDevicePointer(&mapped, hs, 0));
  unsigned char *ds = (unsigned char *)mapped;
  std::vector<long> slot((size_t)nblocks);  // block b's index inside its size class
  long seen[2] = {0, 0};
  for (long b = 0; b < nblocks; b++) {
    const int w = W[b];
    const long i = seen[w]++;
    const size_t n = c->B.bs[w];
    slot[(size_t)b] = i;
    for (size_t k = 0; k < ch; k++) memcpy(hs + o_pcm[w] + ((size_t)i * ch + k) * n * 4, pcm[b * ch + k], n * 4);
    ((int32_t *)(hs + o_lW[w]))[i] = lW[b];
    ((int32_t *)(hs + o_nW[w]))[i] = nW[b];
    ((int32_t *)(hs + o_bt[w]))[i] = blocktype[b];
    ((int32_t *)(hs + o_order))[b] = (int32_t)((w << 30) | (int)i);
  }
  vamd_batch_desc d[2];
  vamd_batch_io io[2];
  vamd_managed_io m[2];
  memset(d, 0, sizeof(d));
  memset(io, 0, sizeof(io));
  memset(m, 0, sizeof(m));
  for (int w = 0; w < 2; w++) {
    d[w].W = w;
    d[w].nblocks = nb[w];
    d[w].lW = (const int32_t *)(ds + o_lW[w]);
    d[w].nW = (const int32_t *)(ds + o_nW[w]);
    d[w].blocktype = (const int32_t *)(ds + o_bt[w]);
    io[w].pcm = (const float *)(ds + o_pcm[w]);
    io[w].ampmax_out = (float *)(ds + o_amp[w]);
    io[w].status = ds + o_st[w];
    if (!managed) {
      io[w].packets = ds + o_pk[w];
      io[w].packet_bits = (int32_t *)(ds + o_bits[w]);
      io[w].packet_stride = (int64_t)row[w];
    } else if (nb[w]) {
      // the candidates' intermediates stay on the device (workspace); their packets go to the arena
      const size_t n2 = (size_t)c->B.bs[w] / 2, units = (size_t)nb[w] * K;
      Arena Q;
      const size_t q_posts = Q.take(units * ch * VAMD_POSTS_STRIDE * 4), q_valid = Q.take(units * ch * 4), q_nz = Q.take(units * ch * 4),
                   q_iwork = Q.take(units * ch * n2 * 4), q_total = Q.at;
      void *dv;
      if ((r = ws_get(c, w, vamd_ctx::WS_M_STAGE, q_total, &dv))) return r;
      unsigned char *dm = (unsigned char *)dv;
      m[w].posts = (int32_t *)(dm + q_posts);
      m[w].post_valid = (int32_t *)(dm + q_valid);
      m[w].nonzero = (int32_t *)(dm + q_nz);
      m[w].iwork = (int32_t *)(dm + q_iwork);
      m[w].packets = ds + o_pk[w];
      m[w].packet_bits = (int32_t *)(ds + o_bits[w]);
      m[w].packet_stride = (int64_t)row[w];
    }
  }
  float state = ampmax_in_first;
  r = run_streams_mixed(c, &d[0], &io[0], &d[1], &io[1], (const int32_t *)(ds + o_order), nblocks, &state, nullptr, 0, nullptr,
                        true, managed && nb[0] ? &m[0] : nullptr, managed && nb[1] ? &m[1] : nullptr);  // (synchronises: the chain's final state comes back)
  if (r) return r;
  const float att = c->B.ampmax_att_per_sec;
  float prev_out = 0.f;
  for (long b = 0; b < nblocks; b++) {
    const int w = W[b];
    const long i = slot[(size_t)b];
    const float out = ((const float *)(hs + o_amp[w]))[i];
    if (ampmax_in) {  // what the block received: the caller's figure, then _vp_ampmax_decay of its predecessor's (lib/psy.c:837-848)
      float a = ampmax_in_first;
      if (b > 0) {
        a = prev_out + ((float)(c->B.bs[w] / 2) / (float)c->B.rate) * att;
        if (a < -9999) a = -9999;
      }
      ampmax_in[b] = a;
    }
    prev_out = out;
    if (ampmax_out) ampmax_out[b] = out;
    unsigned any = 0;
    for (size_t k = 0; k < ch; k++) any |= hs[o_st[w] + (size_t)i * ch + k];
    verdict[b] = (any & VAMD_STATUS_NONFINITE) ? VAMD_ENONFINITE : ((any & VAMD_STATUS_RANGE) ? VAMD_EDOMAIN : VAMD_OK);
    copy_out_packets((const int32_t *)(hs + o_bits[w]) + (size_t)i * K, hs + o_pk[w] + (size_t)i * K * row[w], row[w], K,
                     packet_bits + (size_t)b * K, packets + (size_t)b * K * (size_t)packet_stride, (size_t)packet_stride, verdict[b] == VAMD_OK);
  }
  return VAMD_OK;
}

int vamd_envelope_search(vamd_ctx *c, const float *const *pcm, long nsteps, vamd_envelope_state *state,
                         unsigned char *ret) {
  VAMD_NEEDS_ENCODER(c);
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (nsteps < 0) return fail(c, VAMD_EINVAL, "negative step count");
  if (nsteps == 0) return VAMD_OK;
  if (!pcm || !state || !ret) return fail(c, VAMD_EINVAL, "null pcm / state / ret");
  int r;
  static std::atomic<long> calls{0};
  if ((r = injected_failure(c, c->K.fail_envelope_after, calls, "VAMD_FAIL_ENVELOPE_AFTER"))) return r;
  const int ch = c->B.channels, n = c->B.env.mdct.n, step = c->B.env.searchstep;
  const long len = (nsteps - 1) * step + n;  // samples per channel the steps read
  // [pcm | state | bad (one word, zero on the way up) | ret]
  Arena A;
  const size_t o_pcm = A.take((size_t)ch * len * 4), o_state = A.take(sizeof(vamd_envelope_state)), o_bad = A.take(16),
               o_ret = A.take((size_t)nsteps), total = A.at;
  if ((r = pinned_get(c, c->h_stage, total, false))) return r;
  void *dv;
  if ((r = ws_get(c, 0, vamd_ctx::WS_ENV_STAGE, total, &dv))) return r;
  unsigned char *hs = (unsigned char *)c->h_stage.p, *ds = (unsigned char *)dv;
  if ((r = stage_channels(c, hs + o_pcm, pcm, (size_t)ch, (size_t)len * 4))) return r;
  memcpy(hs + o_state, state, sizeof(*state));
  memset(hs + o_bad, 0, 16);
  hipStream_t s = c->stream;
  HIP_TRY(c, hipMemcpyAsync(ds, hs, o_ret, hipMemcpyHostToDevice, s));
  r = envelope_search_batch(c, (const float *)(ds + o_pcm), (long)ch * len, len, 1, nsteps,
                            (vamd_envelope_state *)(ds + o_state), ds + o_ret, (unsigned int *)(ds + o_bad));
  if (r) return r;
  HIP_TRY(c, hipMemcpyAsync(hs + o_state, ds + o_state, total - o_state, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  if (*(const unsigned int *)(hs + o_bad))  // (the state is left as it was: the stream is over for this caller)
    return fail(c, VAMD_ENONFINITE, "input outside the domain: a non-finite sample (include/vorbis_amd.h, Input domain)");
  memcpy(state, hs + o_state, sizeof(*state));
  memcpy(ret, hs + o_ret, (size_t)nsteps);
  return VAMD_OK;
}
