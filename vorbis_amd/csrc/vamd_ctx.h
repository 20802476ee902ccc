// vamd_ctx.h -- the context behind a vamd_ctx handle: the parameter structs bound to the HBM image, streams and events,
// the workspace, staging, the profiling hooks, the environment knobs -- and the small helpers every entry point uses
// (fail / HIP_TRY, DeviceGuard, ws_get, pinned_get, Arena).  Part of the library's single translation unit: included by
// vamd_hip.hip, once, after vamd_kernels.h and before the three parts of the host side (vamd_batch.h, vamd_block.h,
// vamd_plan.h).
#pragma once
#include "vamd_arena.h"
// ---------------------------------------------------------------------------
// context
// ---------------------------------------------------------------------------
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
};
struct HostBuf : DevBuf {};  // pinned host memory, grown on demand (pinned_get)

struct vamd_ctx {
  int device = 0;
  int num_cus = 256;
  size_t lds_per_block = 160 * 1024;
  hipStream_t stream = nullptr;
  // noise masking and tone masking read different inputs and write different outputs; the tone
  // kernels run on this library-owned side stream, forked from / joined back into `stream`
  hipStream_t side = nullptr;
  unsigned long long *d_clk = nullptr;  // vamd_clock_probe's accumulator (the caller's, device memory), or null
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_join2 = nullptr;  // (ev_join2: the short size class of a mixed run)
  bool overlap = true;
  float couple_band = VAMD_COUPLE_BAND;  // k_couple.h, chan_bin_sure
  Bound B;                 // parameter structs bound to the HBM image
  unsigned char *d_image = nullptr;
  Bound *d_bound = nullptr;  // c->B in HBM: kernels that would otherwise carry several parameter structs in SGPRs read it
  unsigned int *d_bad = nullptr;  // [0] channel-blocks, [1] detector steps outside the input domain since vamd_input_status(), [2] the non-finite ones among [0] (behind d_bound)
  size_t image_bytes = 0;
  std::string err;
  Knobs K;           // the environment knobs, read once at vamd_create (vamd_knobs.h)
  char config[1024]; // ... and as text (vamd_config_string)
  // (test aid) the kernels the last batch call launched for each size class, as words in launch order: the name, and the
  // workgroup's threads where the launch code chooses them ("k_couple/64"); vamd_launch_record
  char roads[2][320] = {{0}, {0}};
  // workspace, grown on demand (vamd_reserve to pre-size)
  enum { WS_MDCT_RAW, WS_LOGMDCT, WS_LOGFFT, WS_NOISE, WS_TONE, WS_MDCT, WS_ILOGMASK, WS_IWORK, WS_POSTS, WS_POSTVALID,
         WS_NONZERO, WS_LOCAL, WS_AMPIN, WS_AMPGLOB, WS_PCM, WS_SEED, WS_SURV, WS_NSURV, WS_MISC,
         WS_ENV_NEAR, WS_ENV_RAW, WS_ENV_AMP, WS_ENV_BITS, WS_ENV_STAGE, WS_M_ILOGMASK, WS_M_STAGE,
         WS_RES_CLASS, WS_RES_ENTRIES, WS_RES_COUNT, WS_COUPLE_STATE,
         WS_PLAN_FLAGS, WS_PLAN_BLOCKS, WS_PLAN_COUNTS, WS_PLAN_BASE, WS_PLAN_DESC, WS_PLAN_ORDER, WS_STATUS, WS_WRAPPED, WS_RES_BOOKS, WS_PLAN_PENDING, WS_PLAN_GEO, WS_COUNT };
  DevBuf ws[2][WS_COUNT];  // per size class (a mixed stream keeps both batches in flight)
  // pinned staging for the per-block host API
  HostBuf h_stage;
  HostBuf h_plan;  // a stream plan's per-stream bases on their way up (vamd_plan_streams)
  HostBuf h_geo;   // per-stream geometry of whole streams of unequal length (vamd_plan_streams_whole_v), of a live group
  // optional per-stage timing (vamd_profile): one event before each stage + one after the last
  unsigned long long *d_dbg = nullptr;  // 80 phase-stopwatch slots when armed
  bool profile = false;
  std::vector<hipEvent_t> ev_pool;
  size_t ev_used = 0;
  std::vector<int> ev_stage;  // per recorded event: the stage whose interval it closes (VAMD_ST_BEGIN = none)
  int prof_runs = 0;          // batches recorded since the last vamd_stage_ms()
  // what the last VBR run of each size class left for k_synth (vamd_synth_streams): its blocks (-1: none) and where their
  // floor flags, integer curves and residue rows are -- the caller's buffers or workspace, as the run had them
  struct SynthSrc {
    long nb = -1;
    const int32_t *post_valid = nullptr;
    const ilog_t *ilogmask = nullptr;
    const int32_t *res_class = nullptr;
    const uint16_t *res_entries = nullptr;
    const int32_t *res_count = nullptr;
  } synth_src[2];
  // the packet decoder (vamd_decode.h): the codebooks' decode tables, built at first use, and its workspace, grown on
  // demand -- the packets and the plan as they go up, per size class the rows k_unpack writes and k_synth's output; the
  // Ogg entry's files as they go up (k_ogg_depage fills `bytes` from them)
  struct Decode {
    bool ready = false;
    int lanes = VAMD_UNPACK_LANES;  // packets a wave of k_unpack
    bool partial = false;           // vamd_decode_partial: k_unpack_partial and the bounded k_synth forms in place of k_unpack / k_synth
    bool follow = false;            // vamd_decode_follow: vamd_decode_ogg* walk links and foreign pages and cut by the page granules
    int pcm_dtype = 0;              // vamd_decode_output: the element type (VAMD_PCM_*) and the layout every decode entry writes;
    bool pcm_interleaved = false;   //   F32 planar takes k_lap / k_lap_window / k_lap_segments, the others their _as forms
    unsigned char *d_tab = nullptr;
    UnpackP U = {};
    DevBuf bytes, plan, status, files;
    DevBuf post_valid[2], ilogmask[2], res_class[2], res_entries[2], res_count[2], synth[2];
    HostBuf h_plan;
    HostBuf h_stage;  // a window call's bytes on their way up: the windows' packets, or their pages (vamd_decode_window.h)
  } dec;
  // a context made from a stream's headers (vamd_create_decoder, vamd_headers.h): no encode-side tables, so every encode
  // entry refuses it; the setup header packet it was made from, which every Ogg entry holds a file's third packet to;
  // and, where a residue book is no lattice book, the value lists in device memory ([nbooks] offsets, then the floats) --
  // launch_synth then takes k_synth_values
  bool decode_only = false;
  std::vector<uint8_t> setup_packet;
  unsigned char *d_values = nullptr;
  ValueP V = {nullptr, nullptr};
};

// what an encode entry answers a decode-only context, before it looks at anything else
#define VAMD_NEEDS_ENCODER(c) \
  if ((c) && (c)->decode_only) return fail((c), VAMD_EIMPL, "decode-only context: made from a stream's headers, it holds no encoder tables")

// stage ids of vamd_stage_ms(); a mark closes the interval of the stage it names (VAMD_ST_BEGIN: opens one)
enum { VAMD_ST_BEGIN = -1, VAMD_ST_TRANSFORM = 0, VAMD_ST_AMPMAX, VAMD_ST_NOISE, VAMD_ST_TONE, VAMD_ST_FLOOR, VAMD_ST_COUPLE,
       VAMD_ST_RESIDUE, VAMD_ST_PACK, VAMD_ST_COUNT };
static void prof_mark(vamd_ctx *c, int stage) {
  if (!c->profile) return;
  if (c->ev_used == c->ev_pool.size()) {
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return;
    c->ev_pool.push_back(e);
  }
  (void)hipEventRecord(c->ev_pool[c->ev_used], c->stream);
  if (c->ev_stage.size() <= c->ev_used) c->ev_stage.resize(c->ev_used + 1);
  c->ev_stage[c->ev_used++] = stage;
}

// a launch of the batch sequence joins its size class's record (vamd_ctx::roads); a word that does not fit whole is
// left out: the record never ends inside a kernel's name
static void road(vamd_ctx *c, int W, const char *kernel, int threads = 0) {
  char word[64];
  const int len = threads ? snprintf(word, sizeof(word), " %s/%d", kernel, threads) : snprintf(word, sizeof(word), " %s", kernel);
  if (len < 0 || len >= (int)sizeof(word)) return;
  char *t = c->roads[W];
  const size_t at = strlen(t);
  const char *w = at ? word : word + 1;  // (no blank in front of the first word)
  if (at + strlen(w) < sizeof(c->roads[W])) memcpy(t + at, w, strlen(w) + 1);
}

// waves per persistent transform workgroup: as many as fit beside the staged tables
static int xf_waves(const vamd_ctx *c, const XformP &P) {
  const int cap = c->K.xf_waves_cap;  // (measurement aid, a test knob: vamd_knobs.h)
  int w = cap > 0 && cap < VAMD_XF_WAVES ? cap : VAMD_XF_WAVES;
  while (w > 1 && transform_lds_bytes(P, w) > c->lds_per_block) w--;
  return w;
}

static int fail(vamd_ctx *c, int code, const char *what, hipError_t e = hipSuccess) {
  if (c) {
    c->err = what;
    if (e != hipSuccess) {
      c->err += ": ";
      c->err += hipGetErrorString(e);
    }
  }
  return code;
}

// what a host-pointer call makes of its block's status bytes (include/vorbis_amd.h, "Input domain")
static int status_verdict(vamd_ctx *c, const unsigned char *st, size_t ch) {
  unsigned any = 0;
  for (size_t i = 0; i < ch; i++) any |= st[i];
  if (any & VAMD_STATUS_NONFINITE)
    return fail(c, VAMD_ENONFINITE, "input outside the domain: a NaN / Inf sample (or finite ones beyond ~3e16 x full scale, where the fp32 spectrum overflows)");
  if (any & VAMD_STATUS_RANGE)
    return fail(c, VAMD_EDOMAIN, "input outside the domain: a quantised value beyond the bound up to which the reference's integer arithmetic is defined (vamd_quant_limit)");
  return VAMD_OK;
}

#define HIP_TRY(c, expr)                                              \
  do {                                                                \
    hipError_t e__ = (expr);                                          \
    if (e__ != hipSuccess) return fail((c), VAMD_EFAULT, #expr, e__); \
  } while (0)


// A context is bound to ONE device (vamd_create).  Every public entry point runs with that device current --
// workspace allocations, pinned staging, launches and the side stream all belong to it -- and puts the caller's
// device back on the way out, so a context on GPU 1 works while the caller (or torch) sits on GPU 0.
struct DeviceGuard {
  int prev = -1;
  bool switched = false;
  explicit DeviceGuard(const vamd_ctx *c) {
    if (!c) return;
    if (hipGetDevice(&prev) == hipSuccess && prev != c->device) switched = hipSetDevice(c->device) == hipSuccess;
  }
  ~DeviceGuard() {
    if (switched) (void)hipSetDevice(prev);
  }
};

static int ws_get(vamd_ctx *c, int W, int which, size_t bytes, void **out) {
  DevBuf &b = c->ws[W][which];
  if (b.bytes < bytes) {
    c->synth_src[W].nb = -1;  // (what the last run left for k_synth may have lived here)
    if (b.p) HIP_TRY(c, hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    HIP_TRY(c, hipMalloc(&b.p, bytes));
    b.bytes = bytes;
  }
  *out = b.p;
  return VAMD_OK;
}

// a pinned buffer of the context's of at least `bytes`; `slack`: half as much again when it has to grow (buffers whose
// size follows the call -- the look-ahead's arena, the plans' geometry -- would otherwise be reallocated at every new maximum)
static int pinned_get(vamd_ctx *c, HostBuf &b, size_t bytes, bool slack) {
  if (b.bytes < bytes) {
    if (b.p) HIP_TRY(c, hipHostFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    const size_t want = slack ? bytes + bytes / 2 : bytes;
    HIP_TRY(c, hipHostMalloc(&b.p, want, hipHostMallocDefault));
    b.bytes = want;
  }
  return VAMD_OK;
}
