// vamd_hip.hip -- libvorbis_amd.so: the C ABI of include/vorbis_amd.h over the gfx950 kernels (vamd_kernels.h: thin
// __global__ shells around the wave-level bodies in k_*.h).  One translation unit, seven files: this root with the context's
// life cycle and the small getters, the context (vamd_ctx.h), and the host side in three parts by topic -- the batch calls
// and their launch sequence (vamd_batch.h), stream planning (vamd_plan.h), the host-pointer per-block calls (vamd_block.h) --
// and the packet decoder (vamd_decode.h); a decode-only context is made from a stream's headers by vamd_headers.h (plain C++).
// (Round 5 took the kernels and the context out of one file of 2 700 lines; round 10 the three parts out of 2 000.)
//
// Launch geometry: one 64-lane wavefront per workgroup, one workgroup per
// channel-block (per block for the coupling stage).  A 65 536-block stereo batch
// is 131 072 workgroups per stage -- ~500 per CU -- so the chip is filled many
// times over and the per-wave latency of the ordered sections (running sums,
// seed_chase, the greedy floor split) is hidden by the other resident waves.
// Intermediates between stages live in an HBM workspace owned by the context;
// a tensor the caller asked for is written straight to the caller's buffer.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (mandatory: the
// reference's results depend on separately rounded mul/add).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <atomic>
#include <new>
#include <string>
#include <vector>

#include "vorbis_amd.h"
#include "vamd_bind.h"
#include "vamd_knobs.h"
#include "vamd_live.h"
#include "k_transform.h"
#include "k_noise.h"
#include "k_tone.h"
#include "k_floor.h"
#include "vamd_wave_pair.h"
#include "k_couple.h"
#include "k_envelope.h"
#include "k_residue.h"
#include "k_pack.h"
#include "k_blockout.h"
#include "k_lpc.h"
#include "k_bitrate.h"
#include "k_synth.h"
#include "k_unpack.h"
#include "vamd_decode_plan.h"
#include "vamd_decode_live_plan.h"
#define VAMD_OGG_NO_FEED_KERNELS  // (k_ogg.h: k_ogg_plan / _pages / _carry are vamd_feed.hip's)
#include "vamd_demux.h"
#include "vamd_demux_live.h"
#include "vamd_decode_layout.h"  // (namespace vamd, so here and not from vamd_decode.h, which is included inside extern "C")
#include "vamd_headers.h"

using namespace vamd;

#include "vamd_kernels.h"  // every __global__ shell
#include "vamd_ctx.h"      // struct vamd_ctx and the helpers of the entry points

// ---------------------------------------------------------------------------
// the C ABI (include/vorbis_amd.h): the context's life cycle and the small getters
// ---------------------------------------------------------------------------
extern "C" {

const char *vamd_config_string(const vamd_ctx *c) { return c ? c->config : ""; }

// vamd_create_abi's way out once HIP has failed: vamd_destroy skips what was never made (every handle is null until its
// creation succeeded; d_bad points into d_bound; where c->device was never read nothing exists that belongs to a device)
static int create_failed(vamd_ctx *c, int caller_device) {
  vamd_destroy(c);
  if (caller_device >= 0) (void)hipSetDevice(caller_device);
  return VAMD_EFAULT;
}

// the part of a context's creation that both kinds share, from the image on: the device, its streams and events, the
// image and the parameter block in HBM.  c: a new context with its knobs read; on failure it is destroyed.
static int create_on_device(vamd_ctx *c, const std::vector<unsigned char> &image, const std::vector<uint32_t> &doff,
                            const std::vector<PsyDerived> &derived, int device, vamd_ctx **out) {
  hipError_t e = hipSuccess;
  int caller_device = -1;
  (void)hipGetDevice(&caller_device);  // put back before returning: creating a context must not move the caller
  if (device >= 0) e = hipSetDevice(device);
  if (e == hipSuccess) e = hipGetDevice(&c->device);
  if (e == hipSuccess) {
    hipDeviceProp_t prop;
    e = hipGetDeviceProperties(&prop, c->device);
    if (e == hipSuccess) {
      c->num_cus = prop.multiProcessorCount;
      c->lds_per_block = prop.sharedMemPerBlock;
      // opt in to the full LDS for the persistent transform kernels (a no-op where the
      // runtime does not require it)
#define VAMD_OPT_IN(LOGN)                                                                                      \
  (void)hipFuncSetAttribute((const void *)k_transform<LOGN>, hipFuncAttributeMaxDynamicSharedMemorySize,       \
                            (int)c->lds_per_block);                                                            \
  (void)hipFuncSetAttribute((const void *)k_mdct_only<LOGN>, hipFuncAttributeMaxDynamicSharedMemorySize,       \
                            (int)c->lds_per_block);
      VAMD_OPT_IN(0) VAMD_OPT_IN(8) VAMD_OPT_IN(9) VAMD_OPT_IN(10) VAMD_OPT_IN(11) VAMD_OPT_IN(12)
#undef VAMD_OPT_IN
      (void)hipFuncSetAttribute((const void *)k_synth, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_per_block);
      if (c->decode_only) (void)hipFuncSetAttribute((const void *)k_synth_values, hipFuncAttributeMaxDynamicSharedMemorySize, (int)c->lds_per_block);
      (void)hipGetLastError();
      if (c->K.verbose)
        fprintf(stderr, "vamd_create: %d CUs, %zu B LDS per workgroup\n", c->num_cus, c->lds_per_block);
    }
  }
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->side, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_join2, hipEventDisableTiming);
  c->overlap = !c->K.no_overlap;
  // (test aid: k_couple's estimate-then-verify margin as a power of two; 1 sends every quad through the exact path)
  c->couple_band = c->K.couple_band_set ? ldexpf(1.f, c->K.couple_band_log2) : VAMD_COUPLE_BAND;
  if (e == hipSuccess) e = hipMalloc((void **)&c->d_image, image.size());
  if (e == hipSuccess) e = hipMemcpy(c->d_image, image.data(), image.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    fprintf(stderr, "vamd_create: HIP failure: %s\n", hipGetErrorString(e));
    return create_failed(c, caller_device);
  }
  c->image_bytes = image.size();
  bind_params(image, doff, derived, c->d_image, &c->B);
  if (!c->decode_only) {  // ... and which stack walk a large batch of either size class takes (not a knob: the build and the setup decide)
    const size_t n = strlen(c->config);
    snprintf(c->config + n, sizeof(c->config) - n, " chase_walk=%s,%s", chase_walk_regs(c->B.psy[0], c->B.psy[1]) ? "regs" : "ring",
             chase_walk_regs(c->B.psy[2], c->B.psy[3]) ? "regs" : "ring");
  }
  const size_t bound_bytes = (sizeof(Bound) + 15) & ~(size_t)15;
  if (hipMalloc((void **)&c->d_bound, bound_bytes + 16) != hipSuccess ||
      hipMemset(c->d_bound, 0, bound_bytes + 16) != hipSuccess ||
      hipMemcpy(c->d_bound, &c->B, sizeof(Bound), hipMemcpyHostToDevice) != hipSuccess) {
    fprintf(stderr, "vamd_create: HIP failure uploading the parameter block\n");
    return create_failed(c, caller_device);
  }
  c->d_bad = (unsigned int *)((unsigned char *)c->d_bound + bound_bytes);
  if (caller_device >= 0 && caller_device != c->device) (void)hipSetDevice(caller_device);
  *out = c;
  return VAMD_OK;
}

int vamd_create_abi(vamd_ctx **out, const void *setup_blob, size_t blob_bytes, int device, int caller_abi_version) {
  if (!out) return VAMD_EINVAL;
  *out = nullptr;
  if (caller_abi_version != VAMD_ABI_VERSION) {
    fprintf(stderr, "vamd_create: the caller was built against ABI %d of include/vorbis_amd.h, this library is ABI %d\n",
            caller_abi_version, VAMD_ABI_VERSION);
    return VAMD_EVERSION;
  }
  vamd_ctx *c = new (std::nothrow) vamd_ctx;
  if (!c) return VAMD_EFAULT;
  c->K = read_knobs();
  knobs_string(c->K, c->config, sizeof(c->config));
  std::vector<unsigned char> image;
  std::vector<uint32_t> doff;
  std::vector<PsyDerived> derived;
  int r = build_image(setup_blob, blob_bytes, &image, &doff, &derived, &c->err);
  if (r != VAMD_OK) {
    fprintf(stderr, "vamd_create: %s\n", c->err.c_str());
    delete c;
    return r;
  }
  return create_on_device(c, image, doff, derived, device, out);
}

// A decode-only context out of a stream's identification and setup header packets (vamd_headers.h).  A refusal's text
// has no context to live in: it is kept here per thread, and vamd_last_error(NULL) hands it out.
static thread_local std::string g_decoder_err;

static int synth_covered(vamd_ctx *c, int W, SynthFloorP *S);  // vamd_batch.h

int vamd_create_decoder(vamd_ctx **out, const void *id_header, size_t id_bytes, const void *setup_header, size_t setup_bytes, int device) {
  if (!out) return VAMD_EINVAL;
  *out = nullptr;
  g_decoder_err.clear();
  HeaderImage H;
  int r = headers_to_image(id_header, id_bytes, setup_header, setup_bytes, &H, &g_decoder_err);
  if (r != VAMD_OK) return r;
  vamd_ctx *c = new (std::nothrow) vamd_ctx;
  if (!c) return VAMD_EFAULT;
  c->K = read_knobs();
  knobs_string(c->K, c->config, sizeof(c->config));
  c->decode_only = true;
  c->setup_packet.assign((const uint8_t *)setup_header, (const uint8_t *)setup_header + setup_bytes);
  vamd_ctx *made = nullptr;
  if ((r = create_on_device(c, H.image, H.derived_off, H.derived, device, &made)) != VAMD_OK) {  // (c is gone)
    g_decoder_err = "vamd_create_decoder: the device part failed (the device ordinal, an allocation or a copy: HIP's reason is on stderr)";
    return r;
  }
  DeviceGuard dev_guard(c);
  vamd_setup_header made_h;
  memcpy(&made_h, H.image.data(), sizeof(made_h));
  for (int W = 0; W < made_h.modes && r == VAMD_OK; W++) {  // (a workgroup's LDS is the device's to say)
    SynthFloorP S;
    r = synth_covered(c, W, &S);
  }
  if (r == VAMD_OK && H.table_books) {  // the value lists, behind their offsets
    const size_t head = ((size_t)H.value_off.size() * 4 + 15) & ~(size_t)15, bytes = head + 4 * H.values.size();
    if (hipMalloc((void **)&c->d_values, bytes) != hipSuccess ||
        hipMemcpy(c->d_values, H.value_off.data(), 4 * H.value_off.size(), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(c->d_values + head, H.values.data(), 4 * H.values.size(), hipMemcpyHostToDevice) != hipSuccess) {
      g_decoder_err = "vamd_create_decoder: HIP failure uploading the residue books' values";
      r = VAMD_EFAULT;
    } else {
      c->V.book_off = (const int *)c->d_values, c->V.values = (const float *)(c->d_values + head);
    }
  }
  if (r != VAMD_OK) {
    if (g_decoder_err.empty()) g_decoder_err = c->err;
    vamd_destroy(c);
    return r;
  }
  {
    const size_t n = strlen(c->config);
    snprintf(c->config + n, sizeof(c->config) - n, " decode_only=1 value_books=%d lattice_books=%d", H.table_books, H.lattice_books);
  }
  *out = c;
  return VAMD_OK;
}

static void decode_release(vamd_ctx *c);  // vamd_decode.h

void vamd_destroy(vamd_ctx *c) {
  DeviceGuard dev_guard(c);
  if (!c) return;
  decode_release(c);
  for (int W = 0; W < 2; W++)
    for (int i = 0; i < vamd_ctx::WS_COUNT; i++)
      if (c->ws[W][i].p) (void)hipFree(c->ws[W][i].p);
  if (c->h_stage.p) (void)hipHostFree(c->h_stage.p);
  if (c->h_plan.p) (void)hipHostFree(c->h_plan.p);
  if (c->h_geo.p) (void)hipHostFree(c->h_geo.p);
  if (c->d_dbg) (void)hipFree(c->d_dbg);
  for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  if (c->ev_join2) (void)hipEventDestroy(c->ev_join2);
  if (c->side) (void)hipStreamDestroy(c->side);
  if (c->d_image) (void)hipFree(c->d_image);
  if (c->d_bound) (void)hipFree(c->d_bound);
  if (c->d_values) (void)hipFree(c->d_values);
  delete c;
}

int vamd_abi_version(void) { return VAMD_ABI_VERSION; }

int vamd_device_count(void) {
  int n = 0;
  return hipGetDeviceCount(&n) == hipSuccess ? n : VAMD_EFAULT;
}

const char *vamd_last_error(const vamd_ctx *c) { return c ? c->err.c_str() : (g_decoder_err.empty() ? "null context" : g_decoder_err.c_str()); }

int vamd_set_stream(vamd_ctx *c, void *s) {
  if (!c) return VAMD_EINVAL;
  c->stream = (hipStream_t)s;
  return VAMD_OK;
}

// Did any block (or detector step) issued on this context since the last call fall outside the input domain?
int vamd_input_status(vamd_ctx *c, long *bad_channel_blocks, long *bad_detector_steps) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  unsigned int h[3] = {0, 0, 0};
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(h, c->d_bad, sizeof(h), hipMemcpyDeviceToHost));
  if (h[0] | h[1] | h[2]) HIP_TRY(c, hipMemset(c->d_bad, 0, sizeof(h)));
  if (bad_channel_blocks) *bad_channel_blocks = (long)h[0];
  if (bad_detector_steps) *bad_detector_steps = (long)h[1];
  if (h[1] | h[2]) return fail(c, VAMD_ENONFINITE, "input outside the domain: NaN / Inf samples");
  if (h[0]) return fail(c, VAMD_EDOMAIN, "input outside the domain: quantised values beyond the bound up to which the reference's integer arithmetic is defined (vamd_quant_limit)");
  return VAMD_OK;
}

int vamd_quant_limit(const vamd_ctx *c, int W, int channel, int *first_bin, int *end_bin, int *square_bin) {
  if (!c || (W != 0 && W != 1) || channel < 0 || channel >= c->B.channels) return VAMD_EINVAL;
  if (first_bin) *first_bin = c->B.qlimit[W].lo[channel];
  if (end_bin) *end_bin = c->B.qlimit[W].hi[channel];
  if (square_bin) *square_bin = c->B.qlimit[W].sq;
  return c->B.qlimit[W].q[channel];
}

int vamd_profile(vamd_ctx *c, int enable) {
  if (!c) return VAMD_EINVAL;
  c->profile = enable != 0;
  c->ev_used = 0;
  c->prof_runs = 0;
  return VAMD_OK;
}

int vamd_stage_ms(vamd_ctx *c, float *ms, int nstages, int *runs) {
  DeviceGuard dev_guard(c);
  if (!c || !ms || nstages < 1) return VAMD_EINVAL;
  for (int i = 0; i < nstages; i++) ms[i] = 0.f;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for (size_t i = 1; i < c->ev_used; i++) {
    const int st = c->ev_stage[i];
    if (st < 0 || st >= nstages) continue;
    float t = 0.f;
    HIP_TRY(c, hipEventElapsedTime(&t, c->ev_pool[i - 1], c->ev_pool[i]));
    ms[st] += t;
  }
  if (runs) *runs = c->prof_runs;
  c->ev_used = 0;
  c->prof_runs = 0;
  return VAMD_OK;
}

int vamd_calib_copy(vamd_ctx *c, void *dst, const void *src, size_t bytes) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (!dst || !src || (bytes & 15) || (((uintptr_t)dst | (uintptr_t)src) & 15)) return fail(c, VAMD_EINVAL, "calibration copy: 16-byte aligned buffers and size");
  if (bytes == 0) return VAMD_OK;
  hipLaunchKernelGGL(k_calib_copy, dim3((unsigned)(c->num_cus * 16)), dim3(256), 0, c->stream, (const F4 *)src, (F4 *)dst, (long)(bytes / 16));
  HIP_TRY(c, hipGetLastError());
  return VAMD_OK;
}

int vamd_clock_probe(vamd_ctx *c, unsigned long long *acc3) {
  if (!c) return VAMD_EINVAL;
  c->d_clk = acc3;
  return VAMD_OK;
}

int vamd_debug_cycles(vamd_ctx *c, int enable, unsigned long long *out80) {
  DeviceGuard dev_guard(c);
  if (!c) return VAMD_EINVAL;
  if (out80 && c->d_dbg) {
    std::vector<unsigned long long> all(64 * 80);
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    HIP_TRY(c, hipMemcpy(all.data(), c->d_dbg, all.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    for (int k = 0; k < 80; k++) {
      out80[k] = 0;
      for (int r = 0; r < 64; r++) out80[k] += all[(size_t)r * 80 + k];
    }
  }
  if (enable) {
    if (!c->d_dbg) HIP_TRY(c, hipMalloc((void **)&c->d_dbg, 64 * 80 * sizeof(unsigned long long)));
    HIP_TRY(c, hipMemset(c->d_dbg, 0, 64 * 80 * sizeof(unsigned long long)));
  } else if (c->d_dbg) {
    HIP_TRY(c, hipFree(c->d_dbg));
    c->d_dbg = nullptr;
  }
  return VAMD_OK;
}

int vamd_channels(const vamd_ctx *c) { return c ? c->B.channels : VAMD_EINVAL; }
int vamd_blocksize(const vamd_ctx *c, int W) { return (c && (W == 0 || W == 1)) ? c->B.bs[W] : VAMD_EINVAL; }
int vamd_posts(const vamd_ctx *c, int W) { return (c && (W == 0 || W == 1)) ? c->B.floor[W][0].posts : VAMD_EINVAL; }

int vamd_packet_capacity(const vamd_ctx *c, int W) {
  if (!c || (W != 0 && W != 1)) return 0;
  return c->B.pack[W].capacity;
}

int vamd_residue_capacity(const vamd_ctx *c, int W) {
  if (!c || (W != 0 && W != 1)) return 0;
  return c->B.res_cap[W];
}

int vamd_submaps(const vamd_ctx *c, int W) { return (c && (W == 0 || W == 1)) ? c->B.chmap[W].submaps : VAMD_EINVAL; }

int vamd_residue_offset(const vamd_ctx *c, int W, int submap) {
  if (!c || (W != 0 && W != 1) || submap < 0 || submap >= c->B.chmap[W].submaps) return VAMD_EINVAL;
  return c->B.res[W][submap].ent_base;
}

int vamd_envelope_geometry(const vamd_ctx *c, int *winlength, int *searchstep) {
  if (!c) return VAMD_EINVAL;
  if (winlength) *winlength = c->B.env.mdct.n;
  if (searchstep) *searchstep = c->B.env.searchstep;
  return VAMD_OK;
}

#include "vamd_batch.h"  // workspace planning, the launch sequence, the batch entry points
#include "vamd_decode.h" // the packet decoder: plan on the host, k_unpack ahead of k_synth and k_lap
#include "vamd_decode_window.h"  // ... windows of streams and of files: a seek index, k_lap_window
#include "vamd_decode_live.h"  // ... and continuing streams in pieces: the lap carried between calls
#include "vamd_decode_ogg_live.h"  // ... and their Ogg bytes in pieces, cut anywhere: open packets carried too
#include "vamd_plan.h"   // the detector over streams, the walk, the plans
#include "vamd_block.h"  // the host-pointer calls: a block, a look-ahead's blocks, a detector call

}  // extern "C"
