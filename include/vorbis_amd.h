/* vorbis_amd.h -- C ABI of libvorbis_amd.so, the MI355X (gfx950) implementation of
 * libvorbis' per-block encode analysis.
 *
 * Drop-in boundary: libvorbis reaches the analysis
 * through vorbis_analysis() (reference lib/analysis.c:29-63) ->
 * _mapping_P[0]->forward == mapping0_forward() (lib/mapping0.c:230-696).  The
 * entry points below replace mapping0_forward -- the numeric section
 * (lib/mapping0.c:254-576, :613-646), the residue back-end's classification and
 * VQ search and the bit-writing of the packet (:596-687) -- and the step loop of
 * the block-switching detector (lib/envelope.c:217-262); the host keeps blockout,
 * bitrate management and Ogg framing.  INTEGRATION.md shows the patch a libvorbis
 * maintainer applies.  Covered: 1 to 8 channels (mono, stereo, the 5.1 layout with
 * its two submaps and four coupling steps, and libvorbisenc's uncoupled template
 * for the rest), VBR and bitrate-managed encoders, block sizes up to 4096.
 *
 * Conventions follow libvorbis: plain C types, caller-allocated outputs, int
 * return codes with the OV_* values of include/vorbis/codec.h:221-235, no
 * callbacks, no exceptions.  A vamd_ctx, like a vorbis_dsp_state, must not be
 * used from two threads at once; distinct contexts are independent.
 */
#ifndef VORBIS_AMD_H
#define VORBIS_AMD_H

#include <stddef.h>
#include <stdint.h>
#include "vamd_setup.h"

#ifdef __cplusplus
extern "C" {
#endif

/* return codes == libvorbis OV_* (include/vorbis/codec.h:221-235) */
#define VAMD_OK        0
#define VAMD_EFAULT   (-129) /* OV_EFAULT: HIP runtime failure; see vamd_last_error() */
#define VAMD_EIMPL    (-130) /* OV_EIMPL: setup/feature outside the covered path */
#define VAMD_EINVAL   (-131) /* OV_EINVAL: bad argument */
#define VAMD_ENOTVORBIS (-132) /* OV_ENOTVORBIS: vamd_create_decoder: a packet is no Vorbis header */
#define VAMD_EBADHEADER (-133) /* OV_EBADHEADER: vamd_create_decoder: a header vorbis_synthesis_headerin refuses */
#define VAMD_EVERSION (-134) /* OV_EVERSION: setup blob version mismatch; an identification header of another Vorbis version */
/* NOT libvorbis codes: the input (not the call) was outside the domain the reference's own arithmetic is defined on ("Input
 * domain" below).  Kept apart from VAMD_EINVAL so that a binding can tell such a block -- which it reports as OV_EINVAL out
 * of vorbis_analysis() -- from a programming error in its own arguments, which it should not swallow.
 *   VAMD_EDOMAIN     finite samples, but a quantised value beyond the bound up to which the reference's integer arithmetic
 *                    is defined by C (vamd_quant_limit()): THIS block has no defined result; the stream goes on
 *   VAMD_ENONFINITE  a NaN / Inf sample: the reference's own state (ampmax chain, detector history) is not a number from
 *                    here on, and the stream is over */
#define VAMD_EDOMAIN    (-140)
#define VAMD_ENONFINITE (-141)

/* lib/codec_internal.h:23-26 */
#define VAMD_BLOCKTYPE_IMPULSE    0
#define VAMD_BLOCKTYPE_PADDING    1
#define VAMD_BLOCKTYPE_TRANSITION 0
#define VAMD_BLOCKTYPE_LONG       1

#define VAMD_POSTS_STRIDE 32   /* ints per channel in the posts[] output (>= 29 posts at 44.1 kHz) */
#define VAMD_AMPMAX_FLOOR (-9999.f) /* a fresh vorbis_block's ampmax, lib/block.c:86 */

typedef struct vamd_ctx vamd_ctx;

/* Replaces the table-building half of vorbis_analysis_init() for the GPU side
 * (lib/block.c:296-311 -> _vds_shared_init :170-293): validates the setup blob
 * produced by vamd_pack_setup() (integration/vamd_pack_setup.c), copies it to
 * HBM on `device` and derives the static index tables the kernels use.
 * `device` < 0 keeps the calling thread's current HIP device. */
int vamd_create_abi(vamd_ctx **ctx, const void *setup_blob, size_t blob_bytes, int device, int caller_abi_version);
/* The entry point is vamd_create(); it hands the library the VAMD_ABI_VERSION of the header the CALLER was compiled
 * against, and the library refuses any other than its own (VAMD_EVERSION): the descriptor structs below grow between
 * releases, and a caller built against a shorter one would have the library read past the end of what it wrote.  (There
 * is deliberately no plain `vamd_create` symbol: a binary built before this rule fails to link instead of to behave.) */
#define vamd_create(ctx, setup_blob, blob_bytes, device) \
  vamd_create_abi((ctx), (setup_blob), (blob_bytes), (device), VAMD_ABI_VERSION)

/* Counterpart of vorbis_dsp_clear() (lib/block.c:340-388) for the GPU state. */
void vamd_destroy(vamd_ctx *ctx);

/* Text of the last failure on this context ("" if none). */
const char *vamd_last_error(const vamd_ctx *ctx);

/* All launches of this context go to `hip_stream` (a hipStream_t; NULL = the
 * null stream).  The caller owns the stream. */
int vamd_set_stream(vamd_ctx *ctx, void *hip_stream);

/* Pre-size the internal HBM workspace for batches of up to `max_blocks` blocks
 * of size class W so that no allocation happens inside a timed region. */
int vamd_reserve(vamd_ctx *ctx, int W, long max_blocks);

/* Measurement hook (no libvorbis counterpart): when enabled, a HIP event is
 * recorded on the context's stream before the first stage kernel of a batch and
 * after every stage.  vamd_stage_ms() synchronises the stream and returns, per
 * stage, the summed elapsed milliseconds of all batches issued since the last
 * call -- eight stages: 0 transform, 1 ampmax, 2 noisemask, 3 tonemask, 4 floor,
 * 5 couple, 6 residue search, 7 packet assembly (stages a batch did not run stay
 * 0; with nstages < 8 the later ones are dropped) -- and the number of batches in
 * *runs (a mixed-size call counts once; both size classes add to the same stage). */
int vamd_profile(vamd_ctx *ctx, int enable);
int vamd_stage_ms(vamd_ctx *ctx, float *ms, int nstages, int *runs);

/* Finer measurement hook: arm (enable=1) / disarm (0) an in-kernel stopwatch; while armed lane 0
 * of every wave adds the shader-clock ticks each phase took to one of 80 slots (16 per stage:
 * transform 0.., noisemask 16.., tonemask 32.., floor 48.., couple 64..).  If out80 is non-NULL
 * the slots accumulated so far are copied out first. */
int vamd_debug_cycles(vamd_ctx *ctx, int enable, unsigned long long *out80);

/* Test aid (no libvorbis counterpart): what the last batch of size class W at the masking level or above left of the tone
 * chain's first two steps, copied to host memory after the stream has drained -- for each of the first `channel_blocks`
 * channel-blocks the seed lines seed_chase walks (`seed`, rows of *row_lines floats of which *lines are lines), the lines
 * that survive the walk (`surv`, rows of *row_lines, ascending) and their number (`nsurv`).  Any of the three may be NULL;
 * with all three NULL only the two sizes are returned.  OV_EINVAL if no such batch has run or it was smaller. */
int vamd_debug_survivors(vamd_ctx *ctx, int W, long channel_blocks, float *seed, uint16_t *surv, int32_t *nsurv,
                         int32_t *row_lines, int32_t *lines);

/* Test aid (no libvorbis counterpart): which kernels the context's last batch call (vamd_analyze_batch and its stream,
 * mixed-stream, synthesis and bitrate-managed forms) launched for size class W, as words in launch order, one per launch
 * of the stages behind the transform: the kernel's name, and "/threads" where the launch code chooses the workgroup's size
 * ("k_noise k_tone_seed k_tone_chase_regs k_floor k_couple/64 k_residue_chunks k_pack_waves"; "k_residue:team/N" is
 * k_residue searching runs of eight values a thread, "k_tone_chase/N" the walk on a ring of N slots).  The launch code
 * picks kernels by batch size, so a test of a batch kernel asks here whether its batch took it.  The string belongs to
 * the context and is rewritten by its next batch call; "" before the first, and for a size class the call had no blocks
 * of. */
const char *vamd_launch_record(const vamd_ctx *ctx, int W);

/* Measurement aid (no libvorbis counterpart): the shader clock while the chip is busy.  While `acc3` (device memory,
 * three 64-bit words zeroed by the caller) is set, every batch of more than a few thousand blocks at the masking level
 * or above has the first wave of its tone stack walk -- which runs beside the noise mask, the path's longest stage --
 * add the shader ticks of its own life (s_memtime) to acc3[0], the ticks of the chip-wide 100 MHz clock (s_memrealtime)
 * to acc3[1] and 1 to acc3[2].  acc3[0] / acc3[1] x 100 MHz is the clock the vector units ran at -- what bench.py prices
 * roofline.valu with instead of a nominal figure.  NULL switches it off.  No launch, no stream of its own. */
int vamd_clock_probe(vamd_ctx *ctx, unsigned long long *acc3);

/* Calibration aid for counter passes (no libvorbis counterpart): copy `bytes` (a multiple of 16) from `src` to `dst`
 * (device pointers) with the library's own kernel k_calib_copy, 16 bytes per lane -- exactly `bytes` read and
 * `bytes` written under a name a profile can find, so that FETCH_SIZE / WRITE_SIZE are scaled by a measured factor
 * (tools/prof_run.py, tools/make_profiles.py) instead of an assumed one. */
int vamd_calib_copy(vamd_ctx *ctx, void *dst, const void *src, size_t bytes);

int vamd_channels(const vamd_ctx *ctx);
int vamd_blocksize(const vamd_ctx *ctx, int W);
int vamd_posts(const vamd_ctx *ctx, int W);

/* ---- batched device API (all pointers are DEVICE pointers) ------------------
 *
 * One batch = `nblocks` blocks of the same size class W, block-major:
 * pcm[nblocks][ch][n], every per-bin output [nblocks][ch][n/2].
 */

/* mdct_forward(lookup,in,out), reference lib/mdct.c:492-562, for `nframes`
 * independent n-sample frames (no window applied; BASELINE config 2).
 * in[nframes][n] -> out[nframes][n/2]. */
int vamd_mdct_forward_batch(vamd_ctx *ctx, int W, const float *in, float *out, long nframes);

/* Per-block descriptors.  The arrays (device, length nblocks) may be NULL, in
 * which case the uniform_* value applies to every block. */
typedef struct vamd_batch_desc {
  int         W;                 /* size class of every block in the batch (vb->W) */
  long        nblocks;
  const int32_t *lW, *nW;        /* vb->lW, vb->nW (lib/block.c:593-595) */
  const int32_t *blocktype;      /* vbi->blocktype (lib/block.c:597-615) */
  const float   *ampmax_in;      /* vbi->ampmax on entry (lib/mapping0.c:244) */
  int         uniform_lW, uniform_nW, uniform_blocktype;
  float       uniform_ampmax_in;
} vamd_batch_desc;

/* Outputs; any pointer may be NULL (that tensor is then kept internal or not
 * produced).  Names follow mapping0_forward's variables / its #if 0
 * _analysis_output taps (lib/mapping0.c:279-657). */
typedef struct vamd_batch_io {
  const float *pcm;       /* in  [nb][ch][n]   vb->pcm, un-windowed; not modified */
  float   *mdct_raw;      /* out [nb][ch][n/2] mdct_forward output (tap "mdct", pre-M1) */
  float   *logfft;        /* out [nb][ch][n/2] (tap "fft") */
  float   *logmdct;       /* out [nb][ch][n/2] (tap "mdct" in dB) */
  float   *noise;         /* out [nb][ch][n/2] _vp_noisemask (tap "noise") */
  float   *tone;          /* out [nb][ch][n/2] _vp_tonemask (tap "tone") */
  float   *logmask;       /* out [nb][ch][n/2] _vp_offset_and_mix select 1 (tap "mask1") */
  float   *mdct;          /* out [nb][ch][n/2] gmdct after AoTuV-M1: the spectrum that is quantised */
  int32_t *posts;         /* out [nb][ch][VAMD_POSTS_STRIDE] floor1_fit result, bit 15 = unused flag */
  int32_t *post_valid;    /* out [nb][ch] 0 where floor1_fit returns NULL (all-zero floor) */
  int32_t *ilogmask;      /* out [nb][ch][n/2] integer floor curve of floor1_encode (tap "maskI") */
  int32_t *iwork;         /* out [nb][ch][n/2] quantised, coupled residue (tap "res") */
  int32_t *nonzero;       /* out [nb][ch] after _vp_couple_quantize_normalize's fix-up */
  float   *local_ampmax;  /* out [nb][ch] */
  float   *ampmax_out;    /* out [nb] vbi->ampmax on exit (lib/mapping0.c:576) */
  /* residue back-end, level FULL only, all three or none: what res2_class
   * decides and, in the order res2_forward emits them, the codebook entries its lattice search
   * picks (lib/res0.c:479-532,783-809,534-640,322-410).  Available when vamd_residue_capacity() > 0. */
  int32_t  *res_class;    /* out [nb][S][VAMD_RES_CLASS_STRIDE] class of each partition (S = vamd_submaps(ctx, W);
                             type 1 over several channels: index = partition * coded channels + channel) */
  uint16_t *res_entries;  /* out [nb][vamd_residue_capacity(ctx, W)] entry numbers in emission order, (stage,
                             partition, channel, vector); a second submap's start at vamd_residue_offset(ctx, W, 1) */
  int32_t  *res_count;    /* out [nb][S][2] {classes (0 = nothing to code), entries} of each submap */
  /* packet assembly, level FULL only, both or none: the block's finished audio
   * packet -- header bits, floor1_encode's writes, the residue's phrase words and codewords, packed
   * LSb first exactly as oggpack_write would (lib/mapping0.c:598-606, lib/floor1.c:833-921,
   * lib/res0.c:534-640).  Available when vamd_packet_capacity() > 0. */
  uint8_t  *packets;      /* out [nb][packet_stride] bytes; the packet is the first (bits+7)/8 of a row */
  int32_t  *packet_bits;  /* out [nb] oggpack_bits(); > 8*packet_stride: the row was too short, packet cut off */
  int64_t   packet_stride;/* row length in bytes, a multiple of 4 (vamd_packet_capacity() always suffices) */
  uint8_t  *status;       /* out [nb][ch] 0, or a set of VAMD_STATUS_* bits where the channel-block was outside the input
                             domain (below) */
  /* blocks read in place (ABI 7).  With pcm_src non-NULL the batch is NOT a packed [nb][ch][n] array: block b, channel c
   * starts at pcm + pcm_src[b] + c * pcm_channel_stride (floats; both multiples of 4, pcm 16-byte aligned) -- e.g. a
   * vamd_stream_plan's src[W] over the stream buffers themselves, which spares vamd_gather_blocks and its copy of every
   * sample.  Blocks may overlap (consecutive blocks of a stream share half their samples). */
  const int64_t *pcm_src;       /* in  device [nb], or NULL: packed */
  int64_t   pcm_channel_stride; /* in  floats between a block's channels (only with pcm_src) */
} vamd_batch_io;
/* vamd_batch_desc / vamd_batch_io / vamd_managed_io MUST be zero-initialised by the caller (memset, = {0}) before the
 * fields it uses are set: members are appended at the END between releases (`status` came in with ABI 6, `pcm_src` with
 * 7), and a member the caller does not set is then a null pointer, which every entry point reads as "not wanted".  A
 * caller built against another header than the library it loads is refused by vamd_create() (VAMD_EVERSION) and can ask
 * beforehand with vamd_abi_version() != VAMD_ABI_VERSION. */
#define VAMD_ABI_VERSION 9
int vamd_abi_version(void);
/* GPUs the HIP runtime shows this process (hipGetDeviceCount; < 0: an OV_*-valued error) -- for plain-C hosts that spread
 * a vamd_feed / vamd_batcher over all of them without linking the runtime themselves. */
int vamd_device_count(void);
/* The environment knobs in force for a context, as "NAME=value" words (read once, at vamd_create; vorbis_amd/csrc/vamd_knobs.h).  The
 * operating knobs (VAMD_VERBOSE, VAMD_BATCH_LANES / _EAGER / _JOIN / _SPIN_BELOW) are always honoured; the test knobs --
 * kernel choices turned the other way, widened margins, occupancy caps, injected failures -- only beside
 * VAMD_TEST_KNOBS=1, so that an inherited environment cannot change what a drop-in library does.  The last word is not a
 * knob: chase_walk=<short>,<long> names the stack walk a large batch of either size class takes ("regs" or "ring"), which
 * the build and the setup decide. */
const char *vamd_config_string(const vamd_ctx *ctx);

/* ---- Input domain ---------------------------------------------------------------------------------
 * libvorbis does not validate PCM: whatever floats arrive go through mapping0_forward.  Inside the domain below this
 * library reproduces the reference bit for bit -- denormals, signed zeros and signals thousands of times over full
 * scale included (tests/soak_lib.py kinds 8-13).  Outside it the reference's own result is not defined by C, there is
 * nothing to be identical to, and the library REPORTS such input instead of inventing an answer.  The domain has two
 * edges, and they are the reference's own:
 *
 *   (1) finite arithmetic.  A NaN or +-Inf sample inside a block's windowed span (a sample the window zeroes --
 *       lib/window.c:2117-2118 -- never enters the arithmetic, in the reference or here) reaches the reference's
 *       float -> int conversions (lib/psy.c:958-962) and stays in its ampmax chain and detector history for the rest
 *       of the stream.  Finite samples do the same only beyond ~3e16 x full scale, where the reference's own fp32
 *       power spectrum overflows to Inf (lib/mapping0.c:323-343).  Test: the block's spectral peak on the reference's
 *       logfft scale (0 dB = a full-scale sine, before the clamp of :345) above +330 dB -- any NaN / Inf puts it
 *       there, todB() reads a float's bits -- one compare per channel-block.  VAMD_STATUS_NONFINITE.
 *   (2) the reference's integers.  Its quantised values are float -> int conversions (lib/psy.c:958-962): defined by C
 *       below 2^31 (VAMD_QUANT_LIMIT_INT).  Where noise normalisation is at work (q < 0.4 at 44.1 kHz; bins from
 *       normal_start on) it squares them in an `int` (:985): defined up to VAMD_QUANT_LIMIT_SQUARE = 46 340.  Its
 *       residue search sums up to eight squared differences in an `int` (lib/res0.c:361-364): defined while every
 *       value AT A POSITION THE RESIDUE CODES stays within a bound Q that depends only on the setup's codebooks --
 *       floor(sqrt(INT_MAX / dim)) less the lattice reach of the last residue class's cascade:
 *       vorbis_amd/csrc/vamd_bind.h, derive_quant_limit(), holds the proof, and vamd_quant_limit() returns Q with the
 *       bins it holds at (13 000 - 32 000 for the libvorbisenc setups: spectra ~ +85 ... +90 dB over full scale;
 *       un-normalised int16-scale floats are beyond it).  Tests: the coupling stage holds every value it writes
 *       against the first two bounds (level FULL; the levels below it form no integers); the residue search holds
 *       every value it loads from a coded position against the third (wherever it runs: res_* or packets asked for --
 *       a caller that takes `iwork` to a residue coder of its own makes that test itself, as the binding does).
 *       VAMD_STATUS_RANGE.  Up to the bounds everything is exact -- the "+60 dB" line of ABI 7 was a sufficient
 *       margin, not the edge; the edge is now the arithmetic's own.  (Ordinary input gets nowhere near Q where a
 *       codebook is searched; elsewhere it does: the reference's own test signal, a full-scale sine, quantises to
 *       ~66 000 at q 0.85 in a 5.1 stream's LFE channel, whose floor and residue end at bin 12 -- coded by nobody, squared
 *       by nobody, and the reference's defined result: tests/test_reference_matrix.py.)
 *
 *   - the host-pointer calls (vamd_analyze_block*, vamd_encode_block, vamd_batcher_encode_block) return
 *     VAMD_ENONFINITE for (1), VAMD_EDOMAIN for (2) (their argument errors stay VAMD_EINVAL); *ampmax_out is
 *     delivered either way (it comes out of the block's FFT).  vamd_envelope_search knows (1) only: a finite stream is
 *     cut into the reference's blocks whatever its level.  Through the binding (integration/mapping0_vamd.c)
 *     vorbis_analysis() returns OV_EINVAL for a block outside the domain.  For (2) that is THIS block only: the
 *     ampmax chain is carried over it and every later block of the stream is again the reference's, bit for bit.  For
 *     (1) it is this block and every later one -- the deviation from upstream that remains deliberate: libvorbis goes
 *     on encoding with NaN in its state; this back-end ends the stream;
 *   - the device-pointer calls are asynchronous: they fill `status` (when given) and count; vamd_input_status()
 *     synchronises the context's stream, returns VAMD_ENONFINITE / VAMD_EDOMAIN if anything issued since the previous
 *     call was outside the domain (how many channel-blocks of either kind / detector steps: the two optional outputs;
 *     the fifteen candidate packets of a bitrate-managed block may count one channel-block up to fifteen times) and
 *     resets the counts.  Outputs of such blocks are deterministic but unspecified; every other block of the batch is
 *     unaffected. */
#define VAMD_STATUS_RANGE     1 /* bits of status[] */
#define VAMD_STATUS_NONFINITE 2
/* the bounds of (2) for size class W and channel `channel` (any pointer may be NULL): the return value Q holds at the
 * bins [*first_bin, *end_bin) of the channel that its residue codes; VAMD_QUANT_LIMIT_SQUARE at the bins from
 * *square_bin on (n/2: nowhere -- noise normalisation is off for this size class); VAMD_QUANT_LIMIT_INT everywhere. */
#define VAMD_QUANT_LIMIT_SQUARE 46340
#define VAMD_QUANT_LIMIT_INT 0x7fffff80
int vamd_quant_limit(const vamd_ctx *ctx, int W, int channel, int *first_bin, int *end_bin, int *square_bin);
int vamd_input_status(vamd_ctx *ctx, long *bad_channel_blocks, long *bad_detector_steps);

#define VAMD_RES_CLASS_STRIDE 512 /* ints per block and submap in res_class[] (>= classified partitions) */

/* Entries one block of size class W can emit at most (the row length of res_entries), or 0 when the
 * mode's residue is not covered on the GPU (residue types 1 and 2 with vectors of <= 8 dimensions are). */
int vamd_residue_capacity(const vamd_ctx *ctx, int W);
/* Submaps of the mode (1; 2 for the 5.1 layout: the full-range channels, then the LFE), and where in a
 * block's res_entries row submap `sm`'s entries start. */
int vamd_submaps(const vamd_ctx *ctx, int W);
int vamd_residue_offset(const vamd_ctx *ctx, int W, int submap);

/* Bytes the longest possible packet of size class W takes (a multiple of 4; worst case over every
 * field's longest codeword), or 0 when packets of this mode are not assembled on the GPU (they are
 * wherever vamd_residue_capacity() > 0). */
int vamd_packet_capacity(const vamd_ctx *ctx, int W);

/* how far down mapping0_forward the batch runs */
#define VAMD_LEVEL_TRANSFORM 1 /* window, MDCT, FFT, logfft/logmdct, local ampmax (lib/mapping0.c:254-360,384) */
#define VAMD_LEVEL_PSY       2 /* + _vp_noisemask, _vp_tonemask (:417-440)           [BASELINE config 3] */
#define VAMD_LEVEL_FULL      3 /* + offset_and_mix, floor1_fit, floor render, couple/quantise (:463-646) [config 4] */

int vamd_analyze_batch(vamd_ctx *ctx, const vamd_batch_desc *desc, const vamd_batch_io *io, int level);

/* A real stream: blocks in stream order whose ampmax chains from block to block
 * (lib/block.c:626-628, lib/psy.c:837-848, lib/mapping0.c:244,346,576).  Same
 * as vamd_analyze_batch(level FULL) except desc->ampmax_in is ignored: block 0
 * starts from `ampmax_state` (host float, in/out: vorbis_look_psy_global.ampmax
 * semantics) and block k+1 receives decay(ampmax_out[k]).  W of block k is
 * desc->W (one size class per call); mixed streams are issued as consecutive
 * calls per run of equal W. */
int vamd_analyze_stream(vamd_ctx *ctx, const vamd_batch_desc *desc, const vamd_batch_io *io,
                        float *ampmax_state);

/* A real stream that mixes both block sizes (BASELINE config 5): the host's
 * vorbis_analysis_blockout() decides (lW, W, nW, blocktype) per block as before; the blocks are
 * handed over bucketed by size class, and `order[k]` (device, length nblocks_total) names the k-th
 * block of the stream: bit 30 = its size class W, bits 0..29 = its index inside that class's
 * batch.  The ampmax chain runs through the blocks in stream order with each block's own decay
 * (lib/psy.c:842: secs = blocksize[W]/2/rate).  Either batch may be empty. */
int vamd_analyze_stream_mixed(vamd_ctx *ctx, const vamd_batch_desc *desc_short, const vamd_batch_io *io_short,
                              const vamd_batch_desc *desc_long, const vamd_batch_io *io_long, const int32_t *order,
                              long nblocks_total, float *ampmax_state);

/* The same for MANY streams in one call (an encoder farm's batch): the blocks of all streams are bucketed
 * by size class as above; order[] lists them stream after stream, each stream's in its own stream order,
 * and stream s owns order[stream_start[s] .. stream_start[s+1]) (device int64 [nstreams+1], stream_start[0]
 * = 0, stream_start[nstreams] = nblocks_total).  ampmax_states (device float [nstreams]) holds every
 * stream's vorbis_look_psy_global.ampmax on entry and is updated in place; the chains run one thread per
 * stream.  Asynchronous on the context's stream like vamd_analyze_batch. */
int vamd_analyze_streams_mixed(vamd_ctx *ctx, const vamd_batch_desc *desc_short, const vamd_batch_io *io_short,
                               const vamd_batch_desc *desc_long, const vamd_batch_io *io_long, const int32_t *order,
                               const int64_t *stream_start, long nstreams, long nblocks_total, float *ampmax_states);


/* ---- per-block host API: the compatibility path behind vorbis_analysis() -----
 * Host pointers.  pcm[ch] -> n samples each (vb->pcm); outputs sized as above for
 * nblocks == 1.  Latency-bound by design (one launch sequence + two PCIe
 * copies per block); throughput users batch. */
int vamd_analyze_block(vamd_ctx *ctx, const float *const *pcm, int lW, int W, int nW, int blocktype,
                       float ampmax_in, float *mdct /*[ch][n/2]*/, float *logmask /*[ch][n/2] or NULL*/,
                       int32_t *posts /*[ch][VAMD_POSTS_STRIDE]*/, int32_t *post_valid /*[ch]*/,
                       int32_t *iwork /*[ch][n/2]*/, int32_t *nonzero /*[ch]*/, float *ampmax_out);

/* ---- the block-switching detector --------------------------------
 * Replaces the step loop of _ve_envelope_search() (lib/envelope.c:217-262) with its _ve_amp()
 * calls (:89-215): one detector step per `searchstep` (64) samples, each reading `winlength`
 * (128) samples of every channel.  Per step the reference ORs three flags: 1|4 = pre-echo
 * trigger, 2 = post-echo trigger; the caller applies them to ve->mark[] exactly as
 * lib/envelope.c:241-258 does (INTEGRATION.md shows the binding) -- cursor/testW logic, which
 * decides block sizes from the marks, stays host code.
 *
 * vamd_envelope_state carries what the reference keeps in envelope_filter_state + ve->stretch
 * (lib/envelope.h:34-45,66), as plain histories: all-zero == a fresh stream (the reference
 * calloc's its state).  A stream may be fed in calls of any length. */
#define VAMD_VE_NEAR_HIST 30  /* near-DC terms a step can reach back to (two refresh periods of 15) */
#define VAMD_VE_AMP_HIST  16  /* band amplitudes a step can reach back to (13), padded */
typedef struct vamd_envelope_state {
  int64_t steps;    /* detector steps consumed so far (nearptr == steps % 15) */
  int32_t stretch;  /* ve->stretch */
  int32_t pad;
  float near_hist[VAMD_MAX_CH][VAMD_VE_NEAR_HIST];   /* oldest first */
  float amp_hist[VAMD_MAX_CH][VAMD_VE_AMP_HIST][8];  /* oldest first; 7 bands + 1 pad */
} vamd_envelope_state;

/* Batch form, everything device-resident.  Stream s, channel c, step j reads
 * pcm[s*stream_stride + c*channel_stride + j*searchstep .. + winlength).  `states` [nstreams]
 * is read and updated in place; ret[s*nsteps + j] receives the step's flags (0..7). */
int vamd_envelope_search_batch(vamd_ctx *ctx, const float *pcm, long stream_stride, long channel_stride,
                               long nstreams, long nsteps, vamd_envelope_state *states, unsigned char *ret);

/* One stream from host memory (the per-call compatibility form used by the libvorbis binding):
 * pcm[c] points at the first sample of the first step; state and ret are host memory. */
int vamd_envelope_search(vamd_ctx *ctx, const float *const *pcm, long nsteps, vamd_envelope_state *state,
                         unsigned char *ret);

/* ---- bitrate-managed blocks ----------------------------------------------
 * With a bitrate manager (vorbis_encode_init; vorbis_bitrate_managed()) mapping0_forward prepares
 * PACKETBLOBS = 15 candidate packets per block and lets vorbis_bitrate_addblock() pick one: two more
 * floor fits on the lower / higher noise curves (offset_select 0 / 2), twelve interpolated floors
 * (floor1_interpolate_fit), and for every candidate its own floor curve, couple/quantise with that
 * candidate's coupling parameters, and residue (lib/mapping0.c:507-573,596-687).  The spectrum, the
 * select-1 mask and ampmax are shared.  Outputs are laid out [block][candidate][channel][...]. */
typedef struct vamd_managed_io {
  int32_t  *posts;       /* out [nb][15][ch][VAMD_POSTS_STRIDE] floor_posts[i][k]                (required) */
  int32_t  *post_valid;  /* out [nb][15][ch] 0 where floor_posts[i][k] is NULL                   (required) */
  int32_t  *iwork;       /* out [nb][15][ch][n/2] quantised, coupled residue of candidate k      (required) */
  int32_t  *nonzero;     /* out [nb][15][ch]                                                     (required) */
  int32_t  *res_class;   /* out [nb][15][S][VAMD_RES_CLASS_STRIDE]   optional, all three or none */
  uint16_t *res_entries; /* out [nb][15][vamd_residue_capacity(ctx, W)] */
  int32_t  *res_count;   /* out [nb][15][S][2] */
  uint8_t  *packets;     /* out [nb][15][packet_stride]           optional, with packet_bits (as vamd_batch_io) */
  int32_t  *packet_bits; /* out [nb][15] */
  int64_t   packet_stride;
} vamd_managed_io;

/* vamd_analyze_batch(level FULL) for bitrate-managed blocks: `io` carries pcm and the shared outputs
 * (mdct, logmask, ampmax_out, the psy taps; its per-candidate fields posts/post_valid/ilogmask/iwork/
 * nonzero/res_* are ignored), `m` the per-candidate ones.  Works on any setup blob: the fifteen
 * candidates' parameters are part of every libvorbisenc setup. */
int vamd_analyze_batch_managed(vamd_ctx *ctx, const vamd_batch_desc *desc, const vamd_batch_io *io,
                               const vamd_managed_io *m);

/* One managed block from host memory (the binding's call): mdct [ch][n/2] and ampmax_out are shared,
 * posts [15][ch][VAMD_POSTS_STRIDE], post_valid / nonzero [15][ch], iwork [15][ch][n/2]; the res_*
 * arrays ([15][...] as above) may be NULL. */
int vamd_analyze_block_managed(vamd_ctx *ctx, const float *const *pcm, int lW, int W, int nW, int blocktype,
                               float ampmax_in, float *mdct, float *ampmax_out, int32_t *posts,
                               int32_t *post_valid, int32_t *iwork, int32_t *nonzero, int32_t *res_class,
                               uint16_t *res_entries, int32_t *res_count);

/* vamd_analyze_block() plus the residue back-end's decisions for the block (host pointers; any may be
 * NULL).  res_entries must hold vamd_residue_capacity(ctx, W) entries, res_class S * VAMD_RES_CLASS_STRIDE
 * ints, res_count S * 2 ints (S = vamd_submaps(ctx, W)).  Fails with VAMD_EIMPL when res_* are asked for a mode that is not covered. */
int vamd_analyze_block_res(vamd_ctx *ctx, const float *const *pcm, int lW, int W, int nW, int blocktype,
                           float ampmax_in, float *mdct, float *logmask, int32_t *posts, int32_t *post_valid,
                           int32_t *iwork, int32_t *nonzero, float *ampmax_out, int32_t *res_class,
                           uint16_t *res_entries, int32_t *res_count);

/* The bitrate manager of a whole stream (vorbis_bitrate_addblock, lib/bitrate.c:73-227) on the device.  It does not
 * feed back into the analysis: per stream it is a serial walk over the blocks' fifteen candidate sizes, which picks one
 * candidate per block and cuts it (oggpack_writetrunc) or pads it with zero bytes where the reference does.  Needs a
 * setup blob with the manager's section (vamd_setup_header.off_bitrate, written by vamd_pack_setup for every managed
 * encoder); on any other context the three calls below return VAMD_EIMPL.  Device pointers, asynchronous on the
 * context's stream.
 *
 * vamd_bitrate_state: bitrate_manager_state's evolving part, per stream.  vamd_bitrate_init_states() sets `nstreams` of
 * them to a stream's start (what vorbis_bitrate_init leaves); a walk reads and updates them, so a stream may be walked
 * in pieces, in order. */
typedef struct vamd_bitrate_state {
  double  avgfloat;          /* bm->avgfloat */
  int64_t minmax_reservoir;  /* bm->minmax_reservoir */
  int64_t avg_reservoir;     /* bm->avg_reservoir */
  int64_t pad;
} vamd_bitrate_state;
int vamd_bitrate_init_states(vamd_ctx *ctx, vamd_bitrate_state *states, long nstreams);
/* order / stream_start / nstreams as vamd_analyze_streams_mixed (order[] bit 30 = W, bits 0..29 = the block's index in
 * its size class); per size class W: packet_bits[W] [nb_W][15] the candidates' oggpack_bits() (vamd_managed_io), status[W]
 * [nb_W][ch] (or NULL: every block has its packets); out choice[W] [nb_W] the chosen candidate (0..14) and final_bits[W]
 * [nb_W] oggpack_bits() of the packet the manager hands out ((final_bits + 7) / 8 bytes: the first bytes of the chosen
 * candidate, then zero bytes where it was padded).  A block with a non-zero status has no packet: the state is left as
 * it is and final_bits = -1, choice = 0.  Either class's arrays may be NULL where it has no blocks. */
int vamd_bitrate_walk(vamd_ctx *ctx, const int32_t *order, const int64_t *stream_start, long nstreams,
                      const int32_t *const packet_bits[2], const uint8_t *const status[2], vamd_bitrate_state *states,
                      int32_t *const choice[2], int32_t *const final_bits[2]);
/* vamd_analyze_streams_mixed for a bitrate-managed setup: each block's fifteen candidate packets (m_short / m_long as
 * vamd_analyze_batch_managed; posts / post_valid / iwork / nonzero required, packets and packet_bits for the walk above),
 * the ampmax chains per stream through ampmax_states, the blocks read in place where io->pcm_src is given. */
int vamd_analyze_streams_mixed_managed(vamd_ctx *ctx, const vamd_batch_desc *desc_short, const vamd_batch_io *io_short,
                                       const vamd_managed_io *m_short, const vamd_batch_desc *desc_long,
                                       const vamd_batch_io *io_long, const vamd_managed_io *m_long, const int32_t *order,
                                       const int64_t *stream_start, long nstreams, long nblocks_total, float *ampmax_states);

/* One block from host memory all the way to its packet(s): what mapping0_forward leaves in
 * vbi->packetblob[] (lib/mapping0.c:593-687).  managed == 0: one packet (candidate PACKETBLOBS/2, the
 * VBR case); managed != 0: all 15 candidates of a bitrate-managed block.  packets [1 or 15][packet_stride]
 * and packet_bits [1 or 15] are host memory; rows need vamd_packet_capacity(ctx, W) bytes.  Fails with
 * VAMD_EIMPL where vamd_packet_capacity() is 0. */
int vamd_encode_block(vamd_ctx *ctx, const float *const *pcm, int lW, int W, int nW, int blocktype, float ampmax_in,
                      int managed, float *ampmax_out, uint8_t *packets, long packet_stride, int32_t *packet_bits);

/* The same for `nblocks` CONSECUTIVE blocks of one stream, in stream order, in one launch sequence -- for a caller that
 * already holds the samples of several blocks: a libvorbis application that writes more than a block's worth per
 * vorbis_analysis_wrote() (lib/block.c:470-532) has determined every block its buffer covers, and the binding looks ahead
 * (integration/mapping0_vamd.c).  managed == 0: one packet per block (VBR); managed != 0: the fifteen
 * candidate packets of a bitrate-managed block, as vamd_encode_block.  Host memory throughout:
 *   pcm[b * ch + c]   channel c of block b (blocksize[W[b]] samples), read during the call only
 *   lW / W / nW / blocktype [nblocks]   what vorbis_analysis_blockout decides per block (lib/block.c:589-611)
 *   ampmax_in_first   vbi->ampmax of block 0 as blockout left it; block b > 0 receives _vp_ampmax_decay of block b-1's
 *                     result exactly as the next blockout would hand it on (lib/block.c:626-628, lib/psy.c:837-848) --
 *                     ampmax_in[b] (optional out) is what each block received, ampmax_out[b] (optional) what it left
 *   packets [nblocks][1 or 15][packet_stride], packet_bits [nblocks][1 or 15]   as vamd_encode_block (rows need
 *                     vamd_packet_capacity of the larger size class)
 *   verdict [nblocks] VAMD_OK, or VAMD_EDOMAIN / VAMD_ENONFINITE for a block outside the input domain (no packet; its
 *                     ampmax still feeds the chain, as the reference's would)
 * Returns VAMD_OK when the batch ran; per-block trouble is in verdict[]. */
int vamd_encode_blocks(vamd_ctx *ctx, long nblocks, const float *const *pcm, const int32_t *lW, const int32_t *W,
                       const int32_t *nW, const int32_t *blocktype, float ampmax_in_first, int managed, float *ampmax_in,
                       float *ampmax_out, uint8_t *packets, long packet_stride, int32_t *packet_bits, int32_t *verdict);

/* winlength / searchstep of the detector (128 / 64 in every libvorbis setup). */
int vamd_envelope_geometry(const vamd_ctx *ctx, int *winlength, int *searchstep);

/* ---- device-resident stream control (reference lib/block.c:534-693 vorbis_analysis_blockout's decisions,
 * lib/envelope.c:262-353 cursor walk and _ve_envelope_mark): whole streams in, block lists out, no host round
 * trip per block.
 *
 * vamd_plan_streams: `nstreams` streams of `nsamples` samples per channel, device-resident -- stream s, channel c
 * at pcm + s*stream_stride + c*channel_stride -- each laid out as the encoder's own PCM buffer would be had
 * nothing been shifted out of it: what vorbis_analysis_buffer()/vorbis_analysis_wrote() accumulate, the
 * start-of-stream pre-extrapolation included (lib/block.c:398-458: host code in the reference, the caller's
 * here), so the first block is centred at blocksizes[1]/2.  Runs the block-switching detector over every
 * stream (as vamd_envelope_search_batch; `states` [nstreams], device, all-zero = fresh streams, updated),
 * then one thread per stream replays blockout's size / window / blocktype decisions and the plan's device
 * arrays are filled.  A plan covers the blocks the reference hands out while the given data suffices
 * (eofflag == 0); a caller closing a stream appends the reference's end-of-stream tail (lib/block.c:486-532)
 * to the buffer first.  Synchronises the context's stream once (the block counts come back to size the
 * outputs).  The plan's arrays belong to the context and stay valid until the next vamd_plan_streams on it.
 *
 * vamd_gather_blocks: the planned blocks of size class W copied out of the streams into a batch
 * pcm_blocks[nblocks[W]][ch][blocksize[W]] (device), the layout vamd_analyze_streams_mixed takes -- whose
 * descriptor arrays, order[] and stream_start[] are the plan's. */
typedef struct vamd_stream_plan {
  int64_t nstreams;
  int64_t nblocks[2];            /* blocks of each size class over all streams */
  const int32_t *lW[2], *nW[2], *blocktype[2];   /* device, per size class [nblocks[W]] */
  const int64_t *src[2];         /* device [nblocks[W]]: offset of the block's first sample from `pcm` (channel 0) */
  const int32_t *order;          /* device [nblocks[0] + nblocks[1]]: W << 30 | index, stream after stream */
  const int64_t *stream_start;   /* device [nstreams + 1] into order[] */
} vamd_stream_plan;

int vamd_plan_streams(vamd_ctx *ctx, const float *pcm, long stream_stride, long channel_stride, long nstreams,
                      long nsamples, vamd_envelope_state *states, vamd_stream_plan *plan);
int vamd_gather_blocks(vamd_ctx *ctx, const vamd_stream_plan *plan, int W, const float *pcm, long channel_stride,
                       float *pcm_blocks);
/* vamd_plan_streams for COMPLETE streams, the two ends included (ABI 9): what the application loop of
 * examples/encoder_example.c:179-236 makes of a stream it writes 1024 frames at a time and then closes with
 * vorbis_analysis_wrote(v, 0).  Stream s, channel c occupies pcm + s*stream_stride + c*channel_stride, laid out
 *   [ blocksizes[1]/2 samples of room | nframes real samples | 3 * blocksizes[1] samples of room ]
 * (channel_stride >= their sum).  The call fills the room in front with the reference's backward LPC extrapolation of
 * the stream's first samples (_preextrapolate_helper, lib/block.c:417-458: order 16, from the first blocksizes[1] + 1024
 * samples), the room behind with its forward extrapolation of the last ones (lib/block.c:474-512: order 32, from as much
 * of the last long block as the encoder still holds when the stream is closed -- which depends on where its block walk
 * stands, so the walk is run up to there first), takes the detector over all of it and plans every block up to and
 * including the stream's last (vb->eofflag, lib/block.c:664-670).  lib/lpc.c's arithmetic -- serial fp64 sums,
 * Levinson-Durbin, the fp32 predictor chain -- is reproduced operation for operation.  `states` as vamd_plan_streams
 * (all-zero on entry). */
int vamd_plan_streams_whole(vamd_ctx *ctx, float *pcm, long stream_stride, long channel_stride, long nstreams,
                            long nframes, vamd_envelope_state *states, vamd_stream_plan *plan);
/* The same for streams of UNEQUAL length: nframes[s] (HOST array [nstreams], each 1 .. max_frames) real samples in stream s,
 * every buffer laid out for max_frames (the room behind a shorter stream's samples starts where ITS samples end and must be
 * zero up to the buffer's end).  One launch sequence for all: every stream gets its own extrapolations, its own share of the
 * detector's steps (the state a stream is left in is the state after exactly its steps) and its own walk. */
int vamd_plan_streams_whole_v(vamd_ctx *ctx, float *pcm, long stream_stride, long channel_stride, long nstreams,
                              long max_frames, const int64_t *nframes, vamd_envelope_state *states, vamd_stream_plan *plan);
/* A plan's lists copied to host arrays (any may be NULL): per size class W lW / nW / blocktype / src [nblocks[W]],
 * order [nblocks[0] + nblocks[1]], stream_start [nstreams + 1].  Synchronises. */
int vamd_plan_fetch(vamd_ctx *ctx, const vamd_stream_plan *plan, int32_t *const lW[2], int32_t *const nW[2],
                    int32_t *const blocktype[2], int64_t *const src[2], int32_t *order, int64_t *stream_start);

/* ---- synthesis: the decoded signal beside the packets (still ABI 9: additions only).  The decoder's per-block, data-parallel
 * back half -- _01inverse's vector adds, the inverse coupling, floor1_inverse2, mdct_backward (lib/mapping0.c:698-799) and
 * vorbis_synthesis_blockin's windowed overlap-add (lib/block.c:779-823) -- run from what the encoder holds of a block in
 * HBM: the floor's integer curve and flags, the residue classes and codebook entries.  No bitstream is read; the entropy
 * decode, the only serial part of vorbis_synthesis(), is not needed.  Bit for bit (signed zeros included) what libvorbis'
 * decoder computes from the packets of the same blocks (tests/test_synth_cpu.py, tests/test_synth_gpu.py).
 *   vamd_analyze_batch_synth   vamd_analyze_batch(level FULL) with the residue search on whether or not `io` takes its
 *     outputs, then synth [nb][ch][n] (device): vb->pcm as vorbis_synthesis() leaves it for each block's packet, un-windowed.
 *     VAMD_EIMPL where vamd_residue_capacity() is 0, where a block's spectrum and butterfly vectors do not fit a workgroup's
 *     LDS, and for a floor of more than two posts whose range (postlist[1]) is no power of two: floor1_pack writes the range
 *     as a bit count and a decoder rebuilds 1 << bits (lib/floor1.c:102-103,160), so such a floor is drawn differently by the
 *     two sides.  libvorbisenc ships one kind, the 5.1 setups' LFE floor (two posts, range 12, decoded as 16): its one line is
 *     drawn the decoder's way here, which is NOT the integer curve the encoder quantised against (the `ilogmask` tap).
 *   vamd_synth_streams         the decoded samples of the streams of a plan, out of the tensors the context's LAST
 *     vamd_analyze_streams_mixed left (a VBR run with packets or residue outputs on, of exactly the plan's blocks; else
 *     VAMD_EINVAL): k_synth per size class into scratch_short / scratch_long ([nblocks[W]][ch][blocksizes[W]] floats, device;
 *     NULL where the class has no blocks), then the lap: stream s, channel c, frame k at pcm[offset[s] + c * frames[s] + k]
 *     (frames, offset: DEVICE arrays [nstreams]; max_frames: the longest, sizes the launch).  Frame 0 is the first block's
 *     centre, the stream's first sample; a stream yields no more frames than its blocks' centres span, which is what the last
 *     packet's granule position cuts a decoder's output to.  Enqueued on the context's stream; no host wait.  The call reads the
 *     run's floor flags, integer curves and residue rows where the run had them: output buffers the caller gave that run
 *     (post_valid, res_class / res_entries / res_count) must still be alive and unwritten; anything that grows the context's
 *     workspace in between (vamd_reserve, another call) makes the call answer VAMD_EINVAL rather than read what has moved.  A
 *     run of another plan with the same block counts cannot be told apart: analyse, then synthesise.  (Public because the
 *     feed, which is built on this ABI alone, is its caller.)
 *   vamd_synth_check           VAMD_OK where size class W's blocks can be synthesised, else VAMD_EIMPL as above (vamd_last_error
 *     says why). */
int vamd_synth_check(vamd_ctx *ctx, int W);
int vamd_analyze_batch_synth(vamd_ctx *ctx, const vamd_batch_desc *desc, const vamd_batch_io *io, float *synth);
int vamd_synth_streams(vamd_ctx *ctx, const vamd_stream_plan *plan, long nstreams, long max_frames, const int64_t *frames,
                       const int64_t *offset, float *scratch_short, float *scratch_long, float *pcm);

/* ---- the packet decoder: audio packets in, PCM out (still ABI 9: additions only).  The front half the synthesis above
 * lacked -- the packet head (lib/synthesis.c:25-88), floor1_inverse1, the phrase words and codebook entries in the order
 * _01inverse / res2_inverse read them, every codeword by table (lib/codebook.c:264-365) -- as a kernel of its own, k_unpack,
 * one lane per packet; it writes exactly the rows the synthesis reads, and k_synth and the lap run on them unchanged.  Bit
 * for bit libvorbis' decoder on the same packets (tests/test_unpack_cpu.py, tests/test_decode_gpu.py).
 *
 * The context's setup blob IS the setup: the packets must come from an encoder of that setup (ours or libvorbis'); header
 * packets are not read.  `bytes` holds the audio packets of all streams back to back in HOST memory, packet p at
 * [offset[p], offset[p+1]), stream s = packets [stream_start[s], stream_start[s+1]).  end_granule (or NULL): per stream
 * the granule position of its last packet, -1 = none; the last block's frames are cut to it as vorbis_synthesis_blockin
 * cuts them (lib/block.c:906-935) for a stream that begins at granule 0.
 *
 *   vamd_decode_plan     host only, nothing is enqueued: frames[s] (host [nstreams]) = the frames stream s decodes to --
 *     the span of its blocks' centres (bs[lW]/4 + bs[W]/4 apart, lib/block.c:840-842; W from each packet's mode bits), cut
 *     as above; zero or one packet gives 0 -- and nblocks[2], the blocks per size class.  VAMD_EINVAL with the reason in
 *     vamd_last_error for a bad descriptor (counts, offsets or stream_start not monotone or out of range); VAMD_EIMPL for a
 *     setup vamd_synth_check refuses, with its text.
 *   vamd_decode_streams  plans again, then on the context's stream: the packets and the plan go up (one copy each),
 *     k_unpack, k_synth per size class, the lap into pcm (DEVICE) -- stream s, channel c, frame k at
 *     pcm[offset_out[s] + c * frames[s] + k], frames as vamd_decode_plan gave them -- and status[s] (host) comes back; the
 *     call returns when it has (one stream synchronisation).  A bad descriptor launches nothing.
 *
 * status[s] is 0, or the VAMD_STATUS_* of the stream's flagged packets or-ed: such a stream has NO frames -- what its part
 * of pcm holds is not its signal -- and the other streams are untouched.
 *   VAMD_STATUS_NOTAUDIO   the packet-type bit is set, or the mode number names no mode
 *   VAMD_STATUS_BADCODE    bits that are no codeword of the book they are read with, or a phrase word beyond the classes
 *   VAMD_STATUS_TRUNCATED  the packet ends before its block is complete (an empty packet too)
 * BY DEFAULT A DELIBERATE DEVIATION: libvorbis decodes what a truncated packet still holds (a floor that meets the end is
 * no floor, a residue keeps what it has -- eopbreak, lib/res0.c:650,709) and returns 0; here the stream is flagged, as a
 * decoded feed's stream with a missing packet is.  The packets a bitrate-managed encoder CUT to fit its reservoir are such
 * packets.  vamd_decode_partial, below, closes it for a context that asks.
 *
 * Workspace: in the context, grown on demand, released with it -- per block 4 ch + ch n/2 + 2048 S + 2 *
 * vamd_residue_capacity + 8 S bytes of rows, 4 ch n of vb->pcm and 29 of plan (ch channels, n the block's size, S its
 * submaps), and the packets themselves.
 *
 * Out of scope: header packets and setups other than the context's; packets in device memory; skipping a packet
 * vorbis_synthesis refuses (vamd_decode_partial, below).  Streams that begin at a nonzero granule and the first page's trim
 * take per-packet marks: vamd_decode_streams_marked, below.  Ogg files: vamd_decode_ogg, below.  A stream that is still being made, its packets in pieces: vamd_decode_live, below. */
#define VAMD_STATUS_NOTAUDIO  4
#define VAMD_STATUS_BADCODE   8
#define VAMD_STATUS_TRUNCATED 16
#define VAMD_STATUS_PARTIAL   128
typedef struct vamd_decode_desc {
  int64_t nstreams, npackets;
  const uint8_t *bytes;          /* HOST: the audio packets, back to back */
  const int64_t *offset;         /* host [npackets + 1], bytes */
  const int64_t *stream_start;   /* host [nstreams + 1], into packets */
  const int64_t *end_granule;    /* host [nstreams] or NULL: the last packet's granule position, -1 = none */
} vamd_decode_desc;
int vamd_decode_plan(vamd_ctx *ctx, const vamd_decode_desc *desc, int64_t *frames /* host [nstreams] */, int64_t *nblocks /* [2] */);
int vamd_decode_streams(vamd_ctx *ctx, const vamd_decode_desc *desc, const int64_t *offset_out /* host [nstreams] */,
                        float *pcm /* device */, uint8_t *status /* host [nstreams] */);

/* ---- packets libvorbis decodes in part (still ABI 9: an addition).  A policy of the context, off by default: with keep
 * != 0 every later decode call on the context -- vamd_decode_streams, vamd_decode_ogg, vamd_decode_live_wrote,
 * vamd_decode_ogg_live_wrote, vamd_decode_window, vamd_decode_ogg_window -- decodes an audio packet for which libvorbis'
 * vorbis_synthesis() returns 0 to what libvorbis leaves in vb->pcm for it, bit for bit, and laps it like any other block
 * (tests/test_unpack_partial_cpu.py, tests/test_decode_partial_gpu.py).  keep > 0 turns it on, 0 off, keep < 0 changes
 * nothing (a query).  -> the setting before the call (0 or 1); VAMD_EINVAL for a null context; VAMD_EIMPL as
 * vamd_decode_plan gives it.  Nothing is enqueued.
 *
 * WHAT IS KEPT.  A packet that stops being read before its block is complete, as libvorbis reads it:
 *   - a read past the packet's end fails, and so does every read after it;
 *   - a channel whose floor meets such a read has no floor (a floor of two posts and no codeword -- the 5.1 LFE's -- whose
 *     posts are missing is, as in libvorbis, a flat floor); the next channel reads on;
 *   - a submap whose residue meets one -- or a phrase word beyond the classes, or a phrase book without used entries, which
 *     fail without moving the reader -- ends there with every vector it had added, an entry whole or not at all; the next
 *     submap reads on.
 * Such a packet sets VAMD_STATUS_PARTIAL in its stream's status[s]: INFORMATIVE.  A stream whose status is 0 or
 * VAMD_STATUS_PARTIAL alone has its planned frames, and they are its signal; a live stream stays alive.  "A flagged stream
 * has no frames" reads status[s] & ~VAMD_STATUS_PARTIAL everywhere.  The _plan calls do not change: a kept packet is a
 * whole block.
 * WHAT STILL FLAGS A STREAM, as by default: a packet vorbis_synthesis() refuses -- the packet-type bit set, a mode number
 * that names no mode or whose block size is not the plan's (VAMD_STATUS_NOTAUDIO), an empty packet or a head that does
 * not complete (VAMD_STATUS_TRUNCATED); and all container damage (VAMD_STATUS_BADPAGE / _BADHEADER, a file that ends inside a page).
 * A LIMIT OF HEADER-MADE SETUPS (vamd_create_decoder): a setup may hold a residue VALUE book without used entries.  libvorbis
 * adds nothing for such a book, reads on and returns 0; here a packet that reaches one is VAMD_STATUS_BADCODE under either
 * policy and its stream has no frames -- flagged, never decoded to something else.  No encoder's setup has such a book.
 * OUT OF SCOPE: skipping a refused packet as a caller of libvorbis does -- that takes per-packet granule positions to lap
 * and count as the reference then does; resynchronising a damaged container.
 * The encoder side and the default policy run the kernels they ran before; the policy launches k_unpack_partial and the
 * bounded k_synth forms in their place. */
int vamd_decode_partial(vamd_ctx *ctx, int keep);

/* ---- packets with marks: the reader's granule walk (still ABI 9: additions only).  vamd_decode_plan / vamd_decode_streams
 * with what a reader of the container knows of every packet in end_granule's place (desc->end_granule is ignored):
 *   granule[p]  the granule position of the page on which packet p completes, where p is the LAST packet to complete there;
 *               -1 elsewhere.  A position below -1 is none, as the page walk reads it.
 *   eos[p]      libogg's e_o_s: the packet is the last to complete on a page with the end-of-stream flag.  NULL: each
 *               stream's last packet.
 * The frames a stream keeps are those vorbis_synthesis_blockin leaves a caller who drains after every packet
 * (lib/block.c:858-937; examples/decoder_example.c, vorbisfile).  With W_p the packets' size classes, add_0 = 0 and
 * add_p = bs[W_{p-1}]/4 + bs[W_p]/4, `count` the frames added so far and `pos` the tracked position, -1 at first: after
 * packet p has added its frames,
 *   while pos == -1 and granule[p] != -1:  pos = granule[p]; if count > granule[p], min(count - granule[p], add_p) of packet
 *     p's OWN frames are cut -- from their end if eos[p], else from their beginning;
 *   otherwise, when pos != -1:  pos += add_p; if granule[p] != -1 and pos != granule[p]: where pos > granule[p] and eos[p],
 *     min(pos - granule[p], add_p) frames are cut from the end of packet p's; pos = granule[p] either way.
 * So a stream that begins at a large granule is cut at its end against the position the pages give, not against a count
 * from 0; a first page whose granule is short of its samples costs frames of the LAST packet of that page; a last page
 * without the end-of-stream flag cuts nothing; no cut exceeds what its packet adds.  Bit for bit the reference over the
 * same marks (tests/test_decode_links_cpu.py, tests/test_decode_links_gpu.py).
 * frames[s], nblocks, offset_out, pcm's layout, status and the errors are vamd_decode_plan's / vamd_decode_streams'; the
 * lap is k_lap_segments, a row per run of kept frames.  Packets vorbis_synthesis refuses flag their stream as before:
 * skipping them stays out of scope.  vamd_decode_partial applies as everywhere. */
typedef struct vamd_decode_marks {
  const int64_t *granule;  /* host [npackets] */
  const uint8_t *eos;      /* host [npackets], or NULL: each stream's last packet */
} vamd_decode_marks;
int vamd_decode_plan_marked(vamd_ctx *ctx, const vamd_decode_desc *desc, const vamd_decode_marks *marks, int64_t *frames /* host [nstreams] */,
                            int64_t *nblocks /* [2] */);
int vamd_decode_streams_marked(vamd_ctx *ctx, const vamd_decode_desc *desc, const vamd_decode_marks *marks, const int64_t *offset_out /* host [nstreams] */,
                               float *pcm /* device */, uint8_t *status /* host [nstreams] */);

/* ---- the live decoder: continuing streams decoded in pieces (still ABI 9: additions only).  The counterpart of a live
 * feed (vamd_feed_create_live): a caller who receives a stream's packets while the stream is still being made -- a live
 * feed's consumer, a receiver -- hands over the next piece of up to max_streams streams per call and gets that piece's
 * samples.  A stream's pieces laid end to end are, bit for bit, what vamd_decode_streams gives for the whole stream, at ANY
 * cut of its packet list into pieces, empty pieces and pieces of one packet included (tests/test_decode_live_cpu.py,
 * tests/test_decode_live_gpu.py).  What is carried between a stream's pieces is its last block's second half, on the
 * device (k_decode_carry_out writes it behind k_synth, k_decode_carry_in stands it in front of the next piece's blocks
 * ahead of k_lap), and that block's size class and a frame count on the host; the rest of a call is the packet decoder
 * above, on the context's stream and in the context's workspace.
 *
 * Slots, as a live feed has them: stream s of a call is the stream of slot[s] (distinct, 0 .. max_streams-1) -- the same
 * stream until a piece closes it.  A slot is free until its first piece, which opens a stream at granule 0; a piece with
 * close[s] != 0 ends the stream behind its blocks, and the slot's next piece opens a fresh one.  Slots a call does not
 * name keep their state.  The pieces are packets as vamd_decode_desc lays them, in HOST memory.
 *
 *   vamd_decode_live_plan   host only, changes nothing: frames[s] of this piece and nblocks[2], the packets per size
 *     class.  The frames of a piece: the stream's blocks of this piece, with the block carried from its last piece (if
 *     any) in front, its centre at 0 -- the span of those centres, bs[lW]/4 + bs[W]/4 apart.  So a first piece of one packet
 *     gives 0 frames (and leaves a carry), an empty piece gives 0 and leaves the slot as it stood, a carried block and m >= 1
 *     packets give the sum of the m steps.  end_granule[s] is read for a closing piece that holds at least one packet:
 *     frames -= min(total - end_granule, step) where it lies below total, the frames handed out since the stream opened
 *     (this piece's included) and step what the last block adds -- vamd_decode_plan's cut.  An EMPTY closing piece only
 *     frees the slot: its samples have already left, and its end_granule is not applied.
 *   vamd_decode_live_wrote  plans again, runs -- the packets and the plan up, k_unpack, k_synth, the two carry kernels,
 *     k_lap into pcm (DEVICE; stream s, channel c, frame k at pcm[offset_out[s] + c * frames[s] + k]), status[s] (host)
 *     back: one stream synchronisation -- and commits the slots' state only when the call has succeeded.
 *
 * status[s] is 0 or the VAMD_STATUS_* bits of the stream's flagged packets.  From the piece that holds a flagged packet
 * on the stream is dead: that piece and every later one have no frames (a packet flagged on the device leaves the piece's
 * planned frames in the layout of pcm; they are not its signal) and carry the status, until a piece closes the stream.
 * What earlier pieces handed out stands; other streams and the slot's next stream are untouched -- what a live feed does
 * with a block outside the input domain.
 *
 * VAMD_EINVAL with the reason in vamd_last_error(ctx), nothing enqueued and no state changed: null pointers; counts,
 * offsets or stream_start not monotone or out of range; a slot out of range or named twice; nstreams > max_streams; a
 * granule position below -1.  VAMD_EIMPL as vamd_decode_plan gives it (at create already).  Every index the kernels use
 * -- the slots, the carried rows, the last blocks' rows -- is computed and range-checked on the host before the first launch.
 *
 * Destroy a live decoder before its context.  Calls on one context are not concurrent, as everywhere.
 * Out of scope: streams that begin at a nonzero granule (per-packet marks are the whole-stream entry's:
 * vamd_decode_streams_marked); packets in device memory; the feed itself is unchanged
 * (VAMD_FEED_DECODED on a live feed is still refused: decode its packets here).  Ogg pages in pieces:
 * vamd_decode_ogg_live, below. */
typedef struct vamd_decode_live vamd_decode_live;
int vamd_decode_live_create(vamd_ctx *ctx, int64_t max_streams, vamd_decode_live **out);
void vamd_decode_live_destroy(vamd_decode_live *d);
typedef struct vamd_decode_live_desc {
  int64_t nstreams, npackets;
  const int64_t *slot;           /* host [nstreams]: distinct, 0 .. max_streams-1 */
  const uint8_t *bytes;          /* HOST: this call's audio packets, back to back */
  const int64_t *offset;         /* host [npackets + 1], bytes */
  const int64_t *stream_start;   /* host [nstreams + 1], into packets */
  const uint8_t *close;          /* host [nstreams] or NULL: != 0 ends the stream after this piece */
  const int64_t *end_granule;    /* host [nstreams] or NULL: read for closing streams only, -1 = none */
} vamd_decode_live_desc;
int vamd_decode_live_plan(vamd_decode_live *d, const vamd_decode_live_desc *desc, int64_t *frames /* host [nstreams] */, int64_t *nblocks /* [2] */);
int vamd_decode_live_wrote(vamd_decode_live *d, const vamd_decode_live_desc *desc, const int64_t *offset_out /* host [nstreams] */,
                           float *pcm /* device */, uint8_t *status /* host [nstreams] */);

/* ---- Ogg Vorbis files in, PCM out (still ABI 9: additions only).  The packet decoder above with a FILE per stream: what
 * vamd_feed_ogg writes, and libvorbis' files of the same setup, decode without a host loop over their bytes.  The contract
 * is vamd_decode_plan's / vamd_decode_streams': frames, offset_out, the layout of pcm, "a flagged stream has no frames", one
 * stream synchronisation per call, VAMD_EINVAL with a reason and nothing launched for a bad descriptor (null pointers; file
 * offsets that are negative, not monotone or beyond 2^40), VAMD_EIMPL as there, the workspace in the context.
 *
 * File s is bytes[file_offset[s] .. file_offset[s+1]) in HOST memory: ONE logical Ogg bitstream (RFC 3533, doc/framing.html)
 * that holds the three Vorbis header packets and then audio packets of the context's setup.  Its pages may be cut wherever
 * the container allows -- packets across pages, pages that complete no packet, pages without a segment, the setup header
 * and audio packets on one page -- not only as "the Ogg feed" below cuts them.  The stream's end granule is the granule
 * position of the page that completes its last audio packet (it feeds the last block's cut, as end_granule does above); a
 * missing end-of-stream flag is no error.
 *
 * Who does what.  The host walks each file's page headers and lacing tables -- serial in pages, about one byte in a
 * hundred -- reads the three header packets and each audio packet's first byte (its mode bits: the block plan), and never
 * reads outside the file's range, whatever the file claims.  The files go up in one copy as they lie.  On the device
 * k_ogg_depage, a wave per page, recomputes the page's checksum over header + lacing + body and moves the page's audio
 * bytes into a packed arena; from there on it is k_unpack, k_synth and k_lap as above.
 *
 * status[s]: the packet decoder's bits, or-ed with
 *   VAMD_STATUS_BADPAGE    the container is broken: a capture pattern or version is wrong; the file ends inside a page
 *                          header, a lacing table, a body or a packet (its last lacing value is 255); the serial number
 *                          changes; the page sequence numbers are not 0, 1, 2 ...; a continued flag disagrees with "a packet
 *                          is open"; a begin-of-stream flag anywhere but on page 0; a page's checksum does not match
 *   VAMD_STATUS_BADHEADER  there are fewer than three packets; packet 0 is not an identification header of version 0 whose
 *                          channels, rate and two block sizes are the blob's; packet 1 is no well-formed comment header
 *                          (type 3, "vorbis", the lengths inside the packet, the framing bit); packet 2 is not type 5 +
 *                          "vorbis", or differs from setup_header where one is given
 * The header packets are not parsed beyond that: the context's setup stays the setup -- its blob, or the headers a
 * decode-only context was made from (vamd_create_decoder, below: such a context holds every file's third packet to its own
 * setup header packet where setup_header is NULL).  A flagged stream costs only itself.
 *
 * DELIBERATE DEVIATIONS: libogg resynchronises behind a damaged page and reports a hole, and libvorbis decodes on out of
 * lap; here the stream is flagged.  BY DEFAULT a chained or multiplexed file is flagged BADPAGE at its second serial
 * number, a stream that begins at a nonzero granule is cut against a count from 0, and the first page's trim is not
 * applied: vamd_decode_follow, below, turns all three into what a reader does.  Out of scope, as above: setups other than
 * the context's (per call the setup header is compared; a context for ANY floor-1 file's setup is made from the file's own
 * headers: vamd_create_decoder, vamd_ogg_read_headers), files that start in device memory.  Seeking: "windows", below. */
#define VAMD_STATUS_BADPAGE   32
#define VAMD_STATUS_BADHEADER 64
typedef struct vamd_decode_ogg_desc {
  int64_t nstreams;
  const uint8_t *bytes;          /* HOST: the files, back to back */
  const int64_t *file_offset;    /* host [nstreams + 1]: file s = bytes[file_offset[s] .. file_offset[s+1]) */
  const uint8_t *setup_header;   /* or NULL: the setup header packet every file's third packet must equal */
  int64_t setup_header_bytes;
} vamd_decode_ogg_desc;
int vamd_decode_ogg_plan(vamd_ctx *ctx, const vamd_decode_ogg_desc *desc, int64_t *frames /* host [nstreams] */, int64_t *nblocks /* [2] */);
int vamd_decode_ogg(vamd_ctx *ctx, const vamd_decode_ogg_desc *desc, const int64_t *offset_out /* host [nstreams] */,
                    float *pcm /* device */, uint8_t *status /* host [nstreams] */);

/* ---- files as a reader takes them: links, foreign pages, page granules (still ABI 9: additions only).  A policy of the
 * context, off by default, for vamd_decode_ogg_plan and vamd_decode_ogg ALONE: on > 0 turns it on, 0 off, on < 0 changes
 * nothing (a query).  -> the setting before the call; VAMD_EINVAL for a null context.  The live, index and window entries
 * keep their behaviour.  With the policy off every entry gives what it gave before.  With it on:
 *   LINKS.  A file is one or more links (a chained file: an Icecast capture has one per title).  A link opens with its
 *     begin-of-stream pages -- the file's first page opens the first with or without the flag; its stream is the first of
 *     those whose first packet is a Vorbis identification header.  A begin-of-stream page behind a page without the flag
 *     opens the next link; the link in front ends there, with or without an end-of-stream page.
 *   FOREIGN PAGES.  Pages of any other serial number inside a link (a multiplexed file) are passed over: their headers and
 *     lacing tables are walked and every length is held against the file (VAMD_STATUS_BADPAGE where one runs past it), but
 *     they get no page row, so their checksums are not looked at.
 *   INSIDE A LINK'S STREAM the page sequence numbers are consecutive from its first page's, the continued flag agrees with
 *     the open packet, and the link does not end inside a packet: else VAMD_STATUS_BADPAGE.  A stream that begins twice in
 *     its link's begin-of-stream pages is BADPAGE.  A link without a Vorbis stream, or whose three headers do not hold to
 *     the context as a file's do above -- a link of another setup -- is VAMD_STATUS_BADHEADER.
 *   FRAMES.  Every audio packet gets the marks of vamd_decode_streams_marked from its page -- the granule position on the
 *     last packet a page completes (below -1: none), the end-of-stream flag on that packet -- and each link is walked as
 *     there, from a fresh lap: its first block gives no output.  A file's frames are its links' frames end to end in one
 *     [ch][frames] row.  A flagged link flags its file, which has no frames; other files are untouched.
 * Every link's byte range is itself a valid file under the policy.  Out of scope still: resynchronisation behind a damaged
 * page; skipping packets vorbis_synthesis refuses; links and start granules in the live, index and window entries; bytes
 * that start in device memory.
 *
 * vamd_ogg_links (host only): the links of file[0 .. bytes) as above, the first `cap` of them into out[], their number into
 * *nlinks whatever cap is.  `serial` is the link's Vorbis stream, or its first page's where it has none.  A C caller lists
 * links as files through file_offset, and makes a context per setup (vamd_ogg_read_headers_serial on the link's range).
 * -> VAMD_OK; VAMD_EINVAL where cap is too small or an argument is null; VAMD_EBADHEADER where a page header, lacing table
 * or body does not hold against the file -- the links begun up to there are listed, the last ending at the break.  No byte
 * outside the file is read.
 * vamd_ogg_read_headers_serial (host only): vamd_ogg_read_headers, below, for the first logical stream of the given serial
 * number instead of the file's first. */
typedef struct vamd_ogg_link {
  int64_t begin, end;  /* the link is file[begin .. end) */
  uint32_t serial;
} vamd_ogg_link;
int vamd_decode_follow(vamd_ctx *ctx, int on);
int vamd_ogg_links(const uint8_t *file, int64_t bytes, vamd_ogg_link *out, int64_t cap, int64_t *nlinks);
int vamd_ogg_read_headers_serial(const uint8_t *file, int64_t bytes, uint32_t serial, uint8_t *out, int64_t cap, int64_t len[3]);

/* ---- the decoded signal in the caller's format (still ABI 9: additions only).  Every decode entry above and below --
 * vamd_decode_streams, _streams_marked, vamd_decode_ogg, vamd_decode_window, vamd_decode_ogg_window, vamd_decode_live_wrote,
 * vamd_decode_ogg_live_wrote -- writes fp32, planar [ch][frames] per stream.  vamd_decode_output sets, PER CONTEXT, another
 * element type and/or layout for all of them; the conversion happens in the store of the last kernel (no second pass over
 * an fp32 buffer, and no fp32 buffer).  Off by default, and with it off (or set back with NULL) every entry gives what it
 * gave, byte for byte, from the same device code.
 *   The prototypes stay: `pcm` is read as a pointer to the format's element type, and it must be aligned to that type
 *     (else VAMD_EINVAL, before anything is enqueued).  offset_out[], and a window call's channel_stride[], count ELEMENTS
 *     of that type, not floats.  Any offset_out >= 0 works, odd ones included.
 *   planar       stream (or window) s, channel c, frame k at pcm[offset_out[s] + c * frames[s] + k], as before
 *   interleaved  ... at pcm[offset_out[s] + k * ch + c].  Crops of one length need no stride: offset_out[w] = w * length * ch,
 *                the tail behind a window's valid frames is left alone.  A window call that names channel_stride under an
 *                interleaved format is VAMD_EINVAL.
 *   No element outside a stream's own ch * frames (a window's ch * count) is written.
 *   A live decoder reads the context's format at each call: the carry between pieces stays fp32, so the format may change
 *     between two pieces of one stream.
 *   vamd_feed_decoded's tensors stay fp32 planar; vamd_pcm_convert, below, converts them.
 * VAMD_PCM_S16 is ov_read's conversion (lib/vorbisfile.c:2018-2036): val = vorbis_ftoi(x * 32768.f), clipped to
 *   [-32768, 32767], where vorbis_ftoi rounds to nearest, ties to even (lib/os.h:149-157, as compiled on x86-64).  For
 *   every float with |x * 32768| < 2^31 the result is bit for bit the reference's.
 *   DELIBERATE DEVIATION: beyond that (|x| >= 65536, the infinities, NaN) the reference's value is its instruction's
 *   "indefinite" result, -32768 for either sign and for NaN (its portable branch is undefined there).  Here such a value
 *   saturates by its sign -- +inf to 32767, -inf to -32768 -- and NaN gives 0.
 * VAMD_PCM_F16 / _BF16 round to nearest even; F16 overflows to the infinities; a NaN stays a NaN (BF16: 0x7fc0).
 * vamd_decode_output -> VAMD_OK; VAMD_EINVAL for an unknown dtype (the context's format stays as it was).
 * vamd_pcm_convert: the same device conversion over an fp32 planar tensor that exists already -- src [ch][frames] floats in
 *   device memory to dst in the given format (NULL: a copy), frames * ch elements, enqueued on the context's stream.  src
 *   and dst must not overlap.  -> VAMD_OK; VAMD_EINVAL for an unknown dtype, ch outside 1 .. 8, frames < 0, a null or
 *   misaligned pointer. */
#define VAMD_PCM_F32  0   /* what every entry gives by default */
#define VAMD_PCM_S16  1   /* int16_t, ov_read's conversion (above) */
#define VAMD_PCM_F16  2   /* IEEE binary16, round to nearest even, overflow to +-inf */
#define VAMD_PCM_BF16 3   /* bfloat16, round to nearest even, NaN stays NaN */
typedef struct vamd_pcm_format {
  int dtype;        /* VAMD_PCM_* */
  int interleaved;  /* 0: planar [ch][frames]; else [frames][ch] */
} vamd_pcm_format;
int vamd_decode_output(vamd_ctx *ctx, const vamd_pcm_format *fmt);
int vamd_pcm_convert(vamd_ctx *ctx, const float *src, int64_t frames, int ch, const vamd_pcm_format *fmt, void *dst);

/* ---- a decoder for a stream the caller did not encode: the context from the stream's own headers (still ABI 9: additions
 * only).  vamd_create_decoder parses the identification and setup header packets (Vorbis I 4.2.2, 4.2.4) as
 * vorbis_synthesis_headerin does and builds a DECODE-ONLY context: every decode entry above and below works on it as on a
 * blob context, bit for bit libvorbis' output under those headers.
 *   VAMD_ENOTVORBIS / VAMD_EBADHEADER / VAMD_EVERSION  what vorbis_synthesis_headerin answers for the packet
 *   VAMD_EIMPL   headers it accepts that lie outside the covered shape: floor 1; residue types 1 and 2; at most 8 channels, 2
 *                submaps and 4 coupling steps; block sizes 64 .. 4096; one mode, or two with mode i of block flag i; at
 *                most 255 books of at most 65 536 entries with a complete code tree (or one used entry of length 1, read from a bit of either value); and
 *                what the decode kernels take for granted of a setup ("Setups in", has the list)
 * with the reason in vamd_last_error(NULL) (per thread; no context exists to hold it).
 * Residue books whose values are the centred integer lattice of libvorbisenc's books -- decided by comparing values -- are
 * decoded by the arithmetic a blob context uses, and a setup that has only such books launches the kernels a blob context
 * launches; any other residue book (explicit value lists, non-integer steps, q_sequencep, another quantlist order) has its
 * value list [entries][dim], as _book_unquantize leaves it, in device memory (64 MiB a setup at most), read by k_synth_values.
 * The context keeps a copy of the setup header packet: vamd_decode_ogg*, vamd_ogg_index_create and the live Ogg decoder
 * hold every file's third packet to it where the call gives no setup_header (VAMD_STATUS_BADHEADER for another setup).
 * Every analysis, encode, envelope, stream-plan and bitrate entry, vamd_synth_streams and its kin and
 * vamd_mdct_forward_batch answer VAMD_EIMPL "decode-only context" and launch nothing; the context stays usable.
 * vamd_channels, vamd_blocksize, vamd_submaps and vamd_residue_capacity work.
 *
 * vamd_ogg_read_headers (host only): the three header packets of a file's first logical stream, which may span pages, back
 * to back into out[0 .. cap) with len[3] their sizes.  -> VAMD_OK; VAMD_EINVAL where cap is too small (len[] then holds
 * the sizes needed) or an argument is null; VAMD_EBADHEADER where the file's pages do not hold three packets (a broken
 * container, a file that ends first).  No byte outside file[0 .. bytes) is read. */
int vamd_create_decoder(vamd_ctx **ctx, const void *id_header, size_t id_bytes, const void *setup_header, size_t setup_bytes, int device);
int vamd_ogg_read_headers(const uint8_t *file, int64_t bytes, uint8_t *out, int64_t cap, int64_t len[3]);

/* ---- windows of streams and of Ogg files: a seek index, crops on the device (still ABI 9: additions only).  A caller who
 * wants a second out of each of a hundred files pays for that second: a window's frames are, bit for bit, the same frames
 * of the whole decode above (and therefore libvorbis'), out of the window's own blocks plus one
 * (tests/test_decode_window_cpu.py, tests/test_decode_window_gpu.py).
 *
 * One rule for both entries.  Stream s has T[s] frames, as vamd_decode_plan / vamd_decode_ogg_plan give them, the end
 * granule's cut included.  Window w names stream[w], start[w] >= 0 and count[w] >= 0; with a = min(start, T) and
 * b = min(start + count, T) it has frames[w] = b - a frames, channel c frame k at pcm[offset_out[w] + c * frames[w] + k] --
 * channel c, frame a + k of the whole decode of that stream.  Several windows of a call may name one stream, overlap, and
 * come in any order.  The blocks taken are the FEWEST: with the stream's block centres C_0 = 0 < C_1 < ..., kA the first k
 * with C_k > a and kB the first with C_k > b - 1, blocks kA - 1 .. kB and no others (a Vorbis block depends on its own
 * packet alone, and a frame between two centres on those two blocks).  An empty window takes no block, no page and no
 * byte.  nblocks[2] of the plan calls: the blocks taken per size class, summed over the windows -- a block two windows
 * share is unpacked once per window; no work is shared across windows.
 *
 *   vamd_decode_window_plan / vamd_decode_window   packets as vamd_decode_desc lays them (all of the streams' packets: the
 *     host reads their first bytes for the centres), and the window list.  Only the packets of the windows' blocks go up;
 *     then k_unpack and k_synth as above and k_lap_window, k_lap's gather with a first frame per window.
 *   vamd_ogg_index_create   one walk of the files and one block plan, kept: per stream the status (the host's bits:
 *     BADPAGE for the container's structure, BADHEADER, NOTAUDIO / an empty packet), T, the file's length, the page rows,
 *     the packet table with first bytes and centres.  It holds no pointer into the caller's bytes.  vamd_ogg_index_info
 *     gives nstreams, frames[] and status[] (any may be NULL).  Destroy an index before its context.
 *   vamd_decode_ogg_window_plan / vamd_decode_ogg_window   the caller hands the SAME files again (bytes, file_offset; the
 *     offsets may differ from create's, the lengths may not) and the window list.  Per window the host picks the pages
 *     from the one in which packet kA - 1 begins through the one that holds packet kB's last byte, copies exactly those
 *     pages into a pinned staging buffer of the context (grown on demand, released with it) and uploads them in one copy;
 *     k_ogg_depage runs over those rows alone; whole page bodies go to the arena and the window's packets are addressed
 *     inside them.  No host work is proportional to the file: a window call never walks pages again.  The plan call's
 *     staged[2] (or NULL): the bytes the call uploads and the pages they are.
 *     channel_stride: NULL, or host [nwindows] -- channel c of window w then lies at offset_out[w] + c * channel_stride[w]
 *     (>= frames[w]): a crop's row of fixed length whose tail the file's end cut stays as the caller left it.
 *
 * status[w]: a stream the index (or the packets' heads) flagged has T = 0; its windows have no frames and carry its bits.
 * What the device finds -- a page's checksum, BADCODE, TRUNCATED -- is reported for the pages and packets the window USES
 * and costs that window its frames, and no other window.  A DELIBERATE DEVIATION: damage outside a window is not seen by
 * that window, though a whole decode of the file would flag the stream.  A file that changed since the index was made:
 * another length is VAMD_EINVAL; other content of the same length is caught by the page checksums or the codebooks and
 * flagged -- every offset used is the index's and lies inside the recorded length, and ogg_depage_inside bounds the device
 * side -- never read out of range.
 *
 * VAMD_EINVAL with a reason, nothing enqueued: null pointers; negative nwindows; a stream out of range; start or count
 * negative or above 2^62; file offsets not monotone or lengths differing from the index's; an index of another context; a
 * channel stride below its window's frames.  VAMD_EIMPL as vamd_decode_plan gives it (at create already).  Every index
 * the kernels use is computed and range-checked on the host before the first launch.
 *
 * Out of scope: streams that begin at a nonzero granule and chained files (vamd_decode_follow is the whole-file entries'
 * alone: an index flags them as before); an index built without a full walk of the files;
 * bytes in device memory. */
typedef struct vamd_ogg_index vamd_ogg_index;
typedef struct vamd_ogg_window_desc {
  int64_t nwindows;
  const int64_t *stream;          /* host [nwindows]: the file of the index */
  const int64_t *start;           /* host [nwindows] */
  const int64_t *count;           /* host [nwindows] */
  const uint8_t *bytes;           /* HOST: the index's files again, back to back */
  const int64_t *file_offset;     /* host [nstreams + 1] */
  const int64_t *channel_stride;  /* or NULL: frames[w] */
} vamd_ogg_window_desc;
int vamd_decode_window_plan(vamd_ctx *ctx, const vamd_decode_desc *desc, int64_t nwindows, const int64_t *stream, const int64_t *start,
                            const int64_t *count, int64_t *frames /* host [nwindows] */, int64_t *nblocks /* [2] */);
int vamd_decode_window(vamd_ctx *ctx, const vamd_decode_desc *desc, int64_t nwindows, const int64_t *stream, const int64_t *start,
                       const int64_t *count, const int64_t *offset_out /* host [nwindows] */, float *pcm /* device */,
                       uint8_t *status /* host [nwindows] */);
int vamd_ogg_index_create(vamd_ctx *ctx, const vamd_decode_ogg_desc *desc, vamd_ogg_index **out);
void vamd_ogg_index_destroy(vamd_ogg_index *index);
int vamd_ogg_index_info(const vamd_ogg_index *index, int64_t *nstreams, int64_t *frames /* host [nstreams] */, uint8_t *status /* host [nstreams] */);
int vamd_decode_ogg_window_plan(vamd_ctx *ctx, const vamd_ogg_index *index, const vamd_ogg_window_desc *desc, int64_t *frames /* host [nwindows] */,
                                int64_t *nblocks /* [2] */, int64_t *staged /* or NULL; [2] */);
int vamd_decode_ogg_window(vamd_ctx *ctx, const vamd_ogg_index *index, const vamd_ogg_window_desc *desc,
                           const int64_t *offset_out /* host [nwindows] */, float *pcm /* device */, uint8_t *status /* host [nwindows] */);

/* ---- the live Ogg decoder: continuing Ogg Vorbis streams decoded in pieces of BYTES (still ABI 9: additions only).  The
 * counterpart of a live Ogg feed (vamd_feed_ogg_headers_live / vamd_feed_ogg, with or without vamd_feed_ogg_flush), of a
 * receiver on a socket: per slot and per call the caller hands over the next bytes of the stream's Ogg bitstream, in HOST
 * memory, cut at ANY byte -- inside a page header, a lacing table, a body, a header packet, an audio packet that spans
 * pages -- and gets PCM on the device for the audio packets those bytes complete.  For a clean stream whose last page
 * carries the end-of-stream flag (every file vamd_feed_ogg and libvorbis write) the pieces' samples laid end to end are,
 * bit for bit, what vamd_decode_ogg gives for the whole file, at any cut list, empty pieces and pieces of one byte
 * included (tests/test_demux_live_cpu.py, tests/test_decode_ogg_live_gpu.py).
 *
 * frames, offset_out, the layout of pcm, status, "a flagged stream has no frames", one stream synchronisation per call
 * and "slots are committed only when the call has succeeded" are vamd_decode_live_wrote's; VAMD_EINVAL comes with a reason
 * and nothing enqueued (null pointers; piece offsets negative, not monotone or beyond 2^40; a slot out of range or named
 * twice; nstreams > max_streams); vamd_decode_ogg_live_plan is host only and changes nothing.
 *
 * Options (NULL: all defaults): setup_header as in vamd_decode_ogg_desc (copied at create); max_packet_bytes, 0 = the
 * larger of vamd_packet_capacity(ctx, 0) and (ctx, 1); max_header_bytes, 0 = 1 MiB.
 *
 * Slots.  A slot is free until its first byte arrives; it then holds ONE logical bitstream until a piece with close[s] != 0
 * closes it.  A slot the call does not name keeps its state.
 * Headers.  Nothing decodes until the three header packets are complete; the host collects their bytes and holds them to
 * vamd_decode_ogg's checks when the third completes.  A failure is VAMD_STATUS_BADHEADER and a dead stream; so are more
 * than max_header_bytes of header bytes (a hostile stream cannot grow host memory without end).
 * A page the cut divides stays on the HOST until it is whole (at most 65 306 bytes per slot) and goes up with the piece
 * that completes it: only whole pages reach the device, gathered with the call's other whole pages into one upload.
 * A packet that whole pages leave open stays on the DEVICE, in a byte carry [max_streams][max_packet_bytes, rounded up to
 * 4]; the host keeps its length so far and its first byte (the mode bits of the block plan).  k_ogg_packet_carry_in puts
 * it in front of the stream's next pages in the call's arena, k_ogg_depage unpages those behind it,
 * k_ogg_packet_carry_out takes what is still open back.  A DELIBERATE DEVIATION from vamd_decode_ogg, which has no such
 * bound: an OPEN audio packet longer than max_packet_bytes is VAMD_STATUS_BADPAGE, flagged on the host before any launch
 * (a packet that completes inside the call that began it is not held to the bound).
 * The end granule is the granule position of the page that completed the stream's last audio packet.  It cuts the last
 * block's share, by vamd_decode_live_plan's rule, in the call that decodes that packet -- if that page carries the
 * end-of-stream flag (so closing later, with an empty piece, gives the same samples), or if the piece closes the stream.
 * A stream closed without the flag gets the cut only if the closing piece holds its last packet.  (The flag counts on the
 * page that COMPLETES the last audio packet, where every encoder puts it; an end-of-stream page that completes no packet
 * ends the stream without a cut, its samples having left with the packet.)
 * An ended stream.  A slot that has seen its end-of-stream page is ended: any further page before the close is
 * VAMD_STATUS_BADPAGE (A DELIBERATE DEVIATION: the whole-file walk ignores the flag).  The caller still closes to free it.
 * Closing.  A closing piece with a divided page still held, or a packet still open, is VAMD_STATUS_BADPAGE (the file "ends
 * inside a page / a packet"); one whose three headers are not complete -- an empty closing piece on a free slot included
 * -- is VAMD_STATUS_BADHEADER (vamd_decode_ogg's answer for a file of no bytes).  Either way the slot is free afterwards.
 * Container checks -- capture pattern, version, serial, sequence numbers, the continued flag, begin-of-stream on page 0
 * alone -- are vamd_decode_ogg's, the walk's state carried per slot; a page's checksum is k_ogg_depage's and arrives with
 * the call's statuses.  From the piece that is flagged on the stream is dead: no frames, and the status on every later
 * piece until one closes it.  What earlier pieces handed out stands; the neighbours and the slot's next stream are
 * untouched.
 * Memory safety.  No byte outside [piece_offset[s], piece_offset[s+1]) is read, whatever the stream claims.  Every index a
 * kernel uses -- the pages' runs of the upload and of the arena, the carry rows' slots and runs, the packets' places, and
 * the live decoder's rows -- is computed and range-checked on the host before the first launch; the kernels trust a row no
 * further than the buffers reach.
 *
 * Destroy a live Ogg decoder before its context.  Out of scope: resynchronisation behind a damaged page; chained or
 * multiplexed streams and streams that begin at a nonzero granule (vamd_decode_follow is the whole-file entries' alone); bytes that start in device memory; seeking; setups other
 * than the context's. */
typedef struct vamd_decode_ogg_live vamd_decode_ogg_live;
typedef struct vamd_decode_ogg_live_opts {
  const uint8_t *setup_header;   /* or NULL: the setup header packet every stream's third packet must equal */
  int64_t setup_header_bytes;
  int64_t max_packet_bytes;      /* 0: the larger vamd_packet_capacity */
  int64_t max_header_bytes;      /* 0: 1 MiB */
} vamd_decode_ogg_live_opts;
typedef struct vamd_decode_ogg_live_desc {
  int64_t nstreams;
  const int64_t *slot;           /* host [nstreams]: distinct, 0 .. max_streams-1 */
  const uint8_t *bytes;          /* HOST: this call's pieces, back to back */
  const int64_t *piece_offset;   /* host [nstreams + 1]: piece s = bytes[piece_offset[s] .. piece_offset[s+1]) */
  const uint8_t *close;          /* host [nstreams] or NULL: != 0 ends the stream after this piece */
} vamd_decode_ogg_live_desc;
int vamd_decode_ogg_live_create(vamd_ctx *ctx, int64_t max_streams, const vamd_decode_ogg_live_opts *opts, vamd_decode_ogg_live **out);
void vamd_decode_ogg_live_destroy(vamd_decode_ogg_live *d);
int vamd_decode_ogg_live_plan(vamd_decode_ogg_live *d, const vamd_decode_ogg_live_desc *desc, int64_t *frames /* host [nstreams] */,
                              int64_t *nblocks /* [2] */);
int vamd_decode_ogg_live_wrote(vamd_decode_ogg_live *d, const vamd_decode_ogg_live_desc *desc, const int64_t *offset_out /* host [nstreams] */,
                               float *pcm /* device */, uint8_t *status /* host [nstreams] */);

/* ---- the host shim for encoders that submit ONE block at a time from many threads.
 * libvorbis' unit of work is one block of one stream (mapping0_forward, reference lib/mapping0.c:233-687); a
 * batcher coalesces concurrent vamd_batcher_encode_block() calls -- same contract as vamd_encode_block() for a VBR
 * encoder, callable from any number of threads, one stream per thread as libvorbis itself requires -- into batched
 * launches.  It owns a few LANES (VAMD_BATCH_LANES in the environment, default 8, at most 16): a context, a HIP stream, a
 * pinned staging arena and one library thread each.  A caller queues its block and sleeps; a lane that is idle takes everything pending
 * of one size class (at most `max_batch` blocks) at once, runs it as a single vamd_analyze_batch() with packet output
 * and wakes exactly the owners of those blocks; blocks that arrive while every lane is busy gather for the next one
 * (a lane that finds both size classes waiting takes the one it did not take last time, so neither waits for ever).
 * There is no timer (`max_wait_us` is accepted and unused since round 4: waiting for stragglers cost more than it
 * gathered).  vamd_batcher_attach / _detach announce a stream (a vorbis_dsp_state); they are bookkeeping only.
 * Errors: OV_*-valued as everywhere; the text of the last one with vamd_batcher_last_error().  vamd_batcher_context()
 * is the first lane's context (capacities, geometry; NOT for launches).  Reference-side use:
 * integration/mapping0_vamd.c with VAMD_BATCH set in the environment. */
typedef struct vamd_batcher vamd_batcher;
int vamd_batcher_create(vamd_batcher **out, const void *setup_blob, size_t blob_bytes, int device, int max_batch,
                        int max_wait_us);
/* The same over several GPUs (ABI 9): lanes are dealt round `devices` (HIP ordinals; at least one lane per device), each with
 * its context, stream, arena and thread on its own device; a batch runs wherever its lane lives -- blocks are independent
 * (SURVEY.md 8e), so nothing crosses between devices. */
int vamd_batcher_create_multi(vamd_batcher **out, const void *setup_blob, size_t blob_bytes, const int *devices, int ndevices,
                              int max_batch, int max_wait_us);
void vamd_batcher_destroy(vamd_batcher *b);
void vamd_batcher_attach(vamd_batcher *b);
void vamd_batcher_detach(vamd_batcher *b);
int vamd_batcher_encode_block(vamd_batcher *b, const float *const *pcm, int lW, int W, int nW, int blocktype,
                              float ampmax_in, float *ampmax_out, uint8_t *packet, long packet_cap,
                              int32_t *packet_bits);
const char *vamd_batcher_last_error(const vamd_batcher *b);
/* batches run, blocks carried, seconds spent inside the batched GPU calls (any pointer may be NULL) */
void vamd_batcher_stats(vamd_batcher *b, long *batches, long *blocks, double *run_seconds);
/* where the batches' time went, as text (diagnostics): gather / staging / GPU / hand-out / wake-up per batch, why gathers
 * ended, batch-size histogram.  Returns the length written. */
long vamd_batcher_report(vamd_batcher *b, char *buf, long cap);
vamd_ctx *vamd_batcher_context(vamd_batcher *b);

/* ---- the host-fed farm (ABI 9): whole streams in from HOST memory, finished packets back to host memory, over one
 * or several GPUs (SURVEY.md 8d "report separately H2D/D2H-inclusive", 8e).  Everything above assumes samples that are
 * already in HBM, or one block per call; an encoder farm holds decoded audio in host memory -- 16-bit interleaved, as
 * examples/encoder_example.c:179-202 reads it -- and wants Ogg payloads back ("the Ogg feed", below).  A vamd_feed owns LANES (per device: a
 * context, a HIP stream, a library thread, pinned input and output arenas, the streams' HBM buffers); a GROUP of streams
 * travels through one lane:
 *     upload (one copy command out of the pinned arena) -> 16-bit to float on the device (x / 32768.f, exactly
 *     encoder_example.c:197-202) -> vamd_plan_streams_whole (both stream ends, detector, block walk) -> full analysis of
 *     every block where it lies in the stream buffers, 50 % overlap read in place, ampmax chains per stream ->
 *     residue search + packet assembly -> the packets laid end to end, written straight into the pinned output arena
 * and while one lane computes, the next group's upload runs beside it on another lane's stream (the link and the
 * shader array are separate resources).  Only samples cross the link upwards (4 bytes per stereo frame: 4 KB per long
 * stereo block) and only packet bytes downwards.  The call sequence mirrors libvorbis' own:
 *     slot = vamd_feed_buffer(f, &pcm)     like vorbis_analysis_buffer(): where to put the next group's samples
 *                                          (blocks while every lane is busy); interleaved [stream][frame][channel]
 *     vamd_feed_wrote(f, slot, ...)        like vorbis_analysis_wrote(): the group is the library's; returns at once
 *     vamd_feed_packets(f, slot, &out)     waits for the group; pointers into the lane's pinned output arena
 *     vamd_feed_release(f, slot)           the lane may be handed out again
 * Every stream of a group is complete; vamd_feed_wrote() takes streams of one length, vamd_feed_wrote_v() of any lengths.
 * Per stream the packets are byte for byte what the reference encoder emits for the same samples written 1024 frames
 * at a time and closed with vorbis_analysis_wrote(v, 0) -- first block to last (tests/test_feed.py).  Setups whose
 * packets the GPU assembles (vamd_packet_capacity() > 0): VBR, and bitrate-managed (ABR / CBR / min-max) ones whose blob
 * carries the manager's section -- then every block's fifteen candidates are made, the manager walks each stream
 * (vamd_bitrate_walk) and the chosen packet, cut or padded, is what comes back (tests/test_feed_managed.py).  The
 * candidates are made in slices of at most 2048 blocks of the group (about 0.5 MB of HBM per long stereo block in the
 * slice), the ampmax chains and the managers carried from slice to slice.  A managed blob without the section (packed
 * before it existed) is refused by vamd_feed_create (VAMD_EIMPL; vamd_feed_last_error(NULL) says why).  Thread rules: one thread drives a feed (or several, each
 * with its own slots); the lanes' threads are the library's.
 * LENGTH of a whole-stream feed's streams: anything up to 0x3fffffff samples per channel, head room and padding included
 * (blocksizes[1]/2 in front, 3 * blocksizes[1] behind: some 6 h 45 min at 44.1 kHz) -- the bound of a block's position, a
 * 32-bit int in the plan.  The block walk reads a stream's detector marks (one per 64 samples) through a window in LDS that
 * slides along the stream, so nothing on the path grows with a workgroup's LDS; what does grow with
 * max_frames is memory: each lane pins a whole group's samples and keeps them, their detector workspaces and their blocks in
 * HBM.  Sources that produce a stream while it plays, and callers that would rather not hold a whole recording, take a LIVE feed:
 *     vamd_feed_create_live(..., write_frames)   the same lanes; each keeps max_streams CONTINUING streams
 *     slot = vamd_feed_buffer(f, &pcm)           the next pieces of that lane's streams 0 .. nstreams-1, back to back
 *     vamd_feed_wrote_live(f, slot, nstreams, frames, close)
 *     vamd_feed_packets / vamd_feed_release      every packet whose block the samples so far determine
 * Stream (slot, s) is the same stream on every write to lane `slot` until a piece closes it; its next piece starts a fresh
 * one.  A stream's packets over all its groups are byte for byte what the reference's application loop emits when it gets
 * the same samples write_frames at a time and is closed with vorbis_analysis_wrote(v, 0) -- for any cut into pieces,
 * pieces of 0 or 1 frames included (tests/test_feed_live.py).  Between groups the device keeps per stream what the
 * reference keeps: the detector state, the walk's W, lW, centerW, cursor and curmark, the detector flags of the steps still
 * ahead of the walk, the ampmax chain, the bitrate manager, the granule position's origin and the samples from
 * centerW - blocksizes[1]/2 on (at most about 1.5 long blocks + 448 samples) -- so neither stream
 * length nor pinned memory grows with a stream.  A non-finite sample (VAMD_FEED_F32) ends its stream at the block that
 * holds it: that packet and every later one of the stream has bits = -1 and VAMD_STATUS_NONFINITE until it is closed. */
typedef struct vamd_feed vamd_feed;
#define VAMD_FEED_S16 0 /* int16_t, interleaved; sample = x / 32768.f */
#define VAMD_FEED_F32 1 /* float, interleaved, already scaled to +-1 */
/* devices: HIP ordinals (NULL / 0: the calling thread's current device); lanes_per_device >= 1 (2 or 3 overlap upload,
 * compute and hand-back; 4-5 keep the shader array fed while the chains of small kernels at a group's start and end
 * run); a group holds at most max_streams streams of at most max_frames frames each, all in `format`.  Pinned host
 * memory per lane: the group's samples plus about a quarter of that for its packets. */
int vamd_feed_create(vamd_feed **out, const void *setup_blob, size_t blob_bytes, const int *devices, int ndevices,
                     int lanes_per_device, long max_streams, long max_frames, int format /* VAMD_FEED_S16 / _F32 */);
void vamd_feed_destroy(vamd_feed *f);
int vamd_feed_lanes(const vamd_feed *f);
int vamd_feed_device(const vamd_feed *f, int slot);   /* the device lane `slot` runs on */
int vamd_feed_buffer(vamd_feed *f, void **pcm);       /* >= 0: the slot; < 0: an OV_*-valued error */
int vamd_feed_wrote(vamd_feed *f, int slot, long nstreams, long frames);
/* streams of unequal length: frames[s] (host array, each 1 .. max_frames, their sum <= max_streams * max_frames) frames of
 * stream s, the streams laid back to back in the arena (stream s starts at frame frames[0] + ... + frames[s-1]) */
int vamd_feed_wrote_v(vamd_feed *f, int slot, long nstreams, const int64_t *frames);
/* a live feed: max_frames is the longest PIECE; write_frames the reference's frames per vorbis_analysis_wrote() (1024 = the
 * example), which decides when a stream's backward extrapolation runs (lib/block.c:524-528: at
 * min(total, (blocksizes[1] / write_frames + 1) * write_frames) frames).  A write_frames whose extrapolation does not fit
 * a workgroup's LDS is refused (VAMD_EIMPL, vamd_feed_last_error(NULL) says why).  vamd_feed_wrote / _wrote_v refuse a live
 * feed and vamd_feed_wrote_live a whole-stream one (VAMD_EINVAL). */
int vamd_feed_create_live(vamd_feed **out, const void *setup_blob, size_t blob_bytes, const int *devices, int ndevices,
                          int lanes_per_device, long max_streams, long max_frames /* per piece */, int format,
                          int write_frames);
/* pieces of the lane's streams 0 .. nstreams-1 laid back to back in the arena as vamd_feed_wrote_v lays them; frames[s] in
 * 0 .. max_frames; close (NULL: none): close[s] != 0 ends stream s after its piece (VAMD_EINVAL for a stream that never had
 * a frame).  The lane's other open streams are left where they stand. */
int vamd_feed_wrote_live(vamd_feed *f, int slot, long nstreams, const int64_t *frames, const uint8_t *close);
typedef struct vamd_feed_result {
  int64_t nstreams, nblocks;      /* blocks == packets, all streams */
  const int64_t *stream_start;    /* [nstreams + 1]: stream s owns packets [stream_start[s], stream_start[s+1]), in stream order */
  const int64_t *offset;          /* [nblocks] where the packet starts in bytes[] (a multiple of 4) */
  const int32_t *bits;            /* [nblocks] oggpack_bits() of the packet: (bits + 7) / 8 bytes; -1: no packet, see info */
  const int64_t *granulepos;      /* [nblocks] ogg_packet.granulepos (vb->granulepos, lib/block.c:620) */
  const uint8_t *info;            /* [nblocks] bit 0: vb->W; bit 1: last packet of its stream (op.e_o_s); bits 2-3: VAMD_STATUS_*
                                     of a block outside the input domain (no packet); bits 4-7: the candidate the bitrate
                                     manager chose (0..14, info >> 4) on a managed setup, 0 on a VBR one */
  const uint8_t *bytes;           /* the packets, end to end */
  int64_t total_bytes;
  double upload_ms, device_ms, total_ms; /* of this group: the upload alone; upload to last kernel; wrote() to ready */
} vamd_feed_result;
int vamd_feed_packets(vamd_feed *f, int slot, vamd_feed_result *out);
int vamd_feed_release(vamd_feed *f, int slot);
/* the text of the feed's last failure; with f == NULL, of this thread's last vamd_feed_create() that failed */
const char *vamd_feed_last_error(const vamd_feed *f);

/* ---- device-fed groups: streams that are ALREADY in device memory (still ABI 9: additions only).  A model, a resampler or
 * a decoder on the same GPU leaves its waveforms in HBM as (batch, channels, frames) tensors -- fp32, fp16 or bf16, ragged,
 * often a view of a larger buffer.  Such a group names its samples where they lie instead of filling the pinned arena:
 *     slot = vamd_feed_buffer(f, &pcm)  or  vamd_feed_buffer_on(f, device, &pcm)      (the arena is simply not filled)
 *     ... [vamd_feed_ogg_serials] [vamd_feed_ogg_comments] [vamd_feed_ogg_flush] ...
 *     vamd_feed_wrote_device(f, slot, nstreams, frames, &src)                  in place of vamd_feed_wrote_v
 *     vamd_feed_wrote_live_device(f, slot, nstreams, frames, close, &src)      in place of vamd_feed_wrote_live
 *     [vamd_feed_source_done(f, slot, consumer, wait_on_host)]                 when the source may be overwritten
 *     vamd_feed_packets / vamd_feed_ogg / vamd_feed_release                    unchanged
 * Stream s of the group has frames[s] frames (1 .. max_frames on a whole-stream feed, 0 .. max_frames on a live one; no bound
 * on their sum: nothing is laid back to back) and its element (channel c, frame k) at base[s] + c * channel_stride +
 * k * frame_stride, in elements of `dtype`.  base[s] may be NULL where frames[s] == 0.  The samples that reach the stream
 * buffers are bit for bit what a host-fed VAMD_FEED_F32 / _S16 group of the same values puts there (a 16-bit float is
 * converted exactly), and everything behind the ingest -- plan, analysis, bitrate manager, packets, Ogg paging -- is the
 * same code: the packets and files are those of the host-fed group (tests/test_feed_device.py).  A non-finite sample is
 * treated as a host-fed VAMD_FEED_F32 group treats it.  A feed may alternate host-fed and device-fed groups, and a live
 * stream may take one piece from the arena and the next from a tensor; the group's dtype is its own, whatever the feed's
 * format.  Measured: profiles/r16_feed_device.txt.
 * LIFETIME: base, frames and close are copied before the call returns.  The source memory must stay valid and unwritten
 * until vamd_feed_source_done, vamd_feed_packets or vamd_feed_ogg has returned for the slot.
 * ORDERING: the lanes' streams are non-blocking streams, so nothing orders them against the work that produces the source.
 * The call records an event -- the lane's own, on the lane's device, which the call makes current for the record and then
 * restores the caller's -- on `producer`, and the lane's stream waits for it before the ingest.  upload_ms of such a group
 * is 0, device_ms runs from the ingest on, and the device's upload turn is not taken: the link is not used.
 * VALIDATION, before anything is enqueued (VAMD_EINVAL, the reason in vamd_feed_last_error, the slot still being filled and
 * the feed usable): dtype known and base non-NULL; every non-NULL base[s] a multiple of the element size and DEVICE memory on
 * vamd_feed_device(slot) as hipPointerGetAttributes tells (pinned or managed host memory is refused); the whole extent
 * stream s reads -- the minimum and the maximum of c * channel_stride + k * frame_stride over c < channels, k < frames[s],
 * plus one element, negative strides counted as such -- inside the allocation hipMemGetAddressRange reports for base[s] (a
 * pointer whose range cannot be had is refused).  So a bad stride is an error code and never a fault.  The allocation may
 * be larger than the caller's tensor (a caching allocator's segment): what is guaranteed is that nothing outside it is read.
 * vamd_feed_wrote_device refuses a live feed and vamd_feed_wrote_live_device a whole-stream one. */
#define VAMD_SRC_S16  0   /* int16_t,  sample = x / 32768.f              */
#define VAMD_SRC_F32  1   /* float,    already +-1                       */
#define VAMD_SRC_F16  2   /* IEEE binary16, converted exactly to float   */
#define VAMD_SRC_BF16 3   /* bfloat16, converted exactly to float        */
/* or'ed into vamd_feed_create[_live]'s format: the lanes allocate no pinned input arena -- vamd_feed_buffer[_on] returns the
 * slot with *pcm = NULL and vamd_feed_wrote / _wrote_v / _wrote_live answer VAMD_EINVAL; device-fed groups only */
#define VAMD_FEED_NO_ARENA 0x100
typedef struct vamd_feed_source {
  const void *const *base;     /* HOST array [nstreams] of DEVICE pointers: stream s, channel 0, frame 0 */
  int dtype;                   /* VAMD_SRC_* : of this group, whatever the feed's own format is */
  int64_t channel_stride;      /* in elements; any sign, 0 allowed (one channel shown to all) */
  int64_t frame_stride;        /* in elements; 1 = planar rows, ch = interleaved, anything else = a view */
  void *producer;              /* hipStream_t whose work enqueued so far must precede the read; 0 = the device's default stream */
} vamd_feed_source;
/* vamd_feed_buffer restricted to the lanes on `device` (a HIP ordinal): waits for one of those; VAMD_EINVAL if the feed has
 * no lane there.  vamd_feed_buffer's round robin may hand out a lane on any device; a tensor is on one. */
int vamd_feed_buffer_on(vamd_feed *f, int device, void **pcm);
int vamd_feed_wrote_device(vamd_feed *f, int slot, long nstreams, const int64_t *frames, const vamd_feed_source *src);
int vamd_feed_wrote_live_device(vamd_feed *f, int slot, long nstreams, const int64_t *frames, const uint8_t *close, const vamd_feed_source *src);
/* Of a slot whose group is device-fed (VAMD_EINVAL otherwise): waits until the lane's thread has enqueued the group's ingest;
 * then, with consumer != NULL, makes that stream wait for the ingest (hipStreamWaitEvent: work enqueued on it afterwards may
 * overwrite the source, no host wait needed); with wait_on_host != 0 also blocks until the ingest has finished. */
int vamd_feed_source_done(vamd_feed *f, int slot, void *consumer /* hipStream_t */, int wait_on_host);

/* ---- the decoded feed: the signal a listener gets back from the packets, on the device (still ABI 9: additions only).
 * Callers whose audio already lives in HBM -- a model, a resampler, a decoder -- also want what the codec makes of it, aligned
 * sample for sample with the input: Vorbis at quality q as an augmentation of device tensors, a quality check of a
 * rendition before the files leave the box, a self-check of a farm's output without a CPU decoder.  VAMD_FEED_DECODED,
 * or'ed into vamd_feed_create's format beside VAMD_FEED_NO_ARENA, gives every group that signal:
 *     ... vamd_feed_wrote / _wrote_v / _wrote_device ...
 *     vamd_feed_packets(f, slot, &out)        unchanged, and no later than without the flag
 *     vamd_feed_decoded(f, slot, &dec)        waits as vamd_feed_packets does, then for the decoded signal
 *     vamd_feed_release(f, slot)
 * Stream s's pcm is bit for bit what libvorbis' decoder returns for the feed's packets of that stream -- vorbis_synthesis +
 * vorbis_synthesis_blockin + vorbis_synthesis_pcmout, the packets' own granule positions given -- frames[s] samples per
 * channel, planar: as many as the stream had frames in, sample k the listener's sample k (tests/test_feed_decoded.py).
 * Nothing is decoded: behind the group's packet hand-over the lane's stream runs vamd_synth_streams over what the analysis
 * left in HBM ("synthesis", above) and records a second event; vamd_feed_decoded waits for that one.
 * A stream with a block that has no packet (bits = -1) gets no signal, exactly as it gets no file: frames[s] = 0 and
 * status[s] says why (frames[s] = 0 is the sign, whatever status[s] holds); the others are untouched.  Host-fed and device-fed groups alike, and together with the Ogg feed.
 * A feed without the flag behaves and allocates exactly as before: its packets and files are byte for byte what they were.
 * A lane of a decoded feed also holds, in HBM, the decoded arena (channels * max_streams * max_frames floats) and k_synth's
 * scratch (about twice that).  VAMD_EINVAL: vamd_feed_decoded on a feed without the flag; a slot that is not ready is
 * treated as vamd_feed_packets treats it.  VAMD_EIMPL from vamd_feed_create with the flag and a bitrate-managed blob (the
 * manager may CUT the chosen packet, and a decoder that runs out of bits stops in mid-residue: eopbreak, lib/res0.c:686,701),
 * from vamd_feed_create_live with the flag (the overlap would have to be carried between groups), and for a setup
 * vamd_analyze_batch_synth refuses; vamd_feed_last_error(NULL) says which. */
#define VAMD_FEED_DECODED 0x200
typedef struct vamd_feed_decoded_result {
  int64_t nstreams; int32_t channels;
  const int64_t *frames;   /* host [nstreams]: decoded frames == the stream's input frames; 0 where status[s] != 0 */
  const int64_t *offset;   /* host [nstreams + 1], in floats: stream s, channel c, frame k at pcm[offset[s] + c * frames[s] + k] */
  const uint8_t *status;   /* host [nstreams]: 0, or the VAMD_STATUS_* of the block that cost the stream its signal */
  const float   *pcm;      /* DEVICE memory on vamd_feed_device(slot); complete when the call returns; valid until vamd_feed_release */
  int64_t total_floats;
} vamd_feed_decoded_result;
int vamd_feed_decoded(vamd_feed *f, int slot, vamd_feed_decoded_result *out);   /* waits as vamd_feed_packets does */

/* ---- the Ogg feed: complete Ogg Vorbis I files beside the packets (whole-stream feeds; a live feed's files come in pieces,
 * "the live Ogg feed" below; still ABI 9: additions only).
 *     vamd_feed_ogg_headers(f, id, comment, setup)   once, before the first vamd_feed_buffer: the feed is an Ogg feed
 *     slot = vamd_feed_buffer(f, &pcm) ... [vamd_feed_ogg_serials(f, slot, ...)] [vamd_feed_ogg_comments(f, slot, ...)] ...
 *                                              vamd_feed_wrote / _wrote_v
 *     vamd_feed_ogg(f, slot, &files)                 waits as vamd_feed_packets does; one byte range per stream
 *     vamd_feed_packets(f, slot, &out)               unchanged, and still there
 * The three header packets are what vorbis_analysis_headerout() gives for the encoder setup the blob was packed from (the
 * setup header is libvorbis' codebook packing: the host's, once per setup); they are validated -- packet types 1 / 3 / 5
 * + "vorbis", a 30-byte identification header whose channels, rate and block sizes are the context's -- else VAMD_EINVAL,
 * the reason in vamd_feed_last_error.  A live feed answers VAMD_EIMPL here: what it returns are pieces of files, a contract
 * of its own that the caller opts into by name (vamd_feed_ogg_headers_live).  The comment packet given here is the
 * feed's own: every stream carries it unless its group names another for it (vamd_feed_ogg_comments, below).
 * Framing (doc/framing.html, doc/a1-encapsulation-ogg.tex) happens on the device behind the group's last packet: the
 * copy kernels keep a mirror of the packet arena in HBM, k_ogg_plan walks every stream's packet sizes into pages,
 * k_ogg_pages writes each page -- header, lacing, body, CRC -- straight into a second pinned arena; no further host wait.
 * THE PAGING POLICY is fixed, so a stream's file is a function of its packets, its serial number and its comment packet alone:
 *   - a packet of n bytes is n / 255 lacing values of 255 and one of n % 255;
 *   - page 0 holds the identification header alone (flags 0x02, granule position 0, sequence number 0; 58 bytes);
 *   - the comment and setup headers start on page 1, granule position 0; the page on which the setup header ends is closed;
 *   - the first audio packet starts a fresh page; segments are taken in order; before a segment is taken the page is
 *     closed if it holds 255 segments, wherever that falls; at a packet boundary it is closed once its body holds more
 *     than 4096 bytes and at least four packets have been completed on it; the end of the stream closes the last page;
 *   - flags: 0x01 where the page's first segment continues a packet, 0x04 on the page with the stream's last segment;
 *     sequence numbers count from 0; a page's granule position is that of the last packet completed on it, -1 if none
 *     (so the last page's is the stream's frame count, which trims the decoder's output); the CRC is framing.html's.
 * Byte equality with libogg's own page cuts is not claimed.  A stream in which any block has no packet (bits = -1) gets
 * NO file -- a hole would decode out of lap: its range is empty, status[s] carries that block's VAMD_STATUS_*; the other
 * streams of the group are untouched.  Serial numbers: stream s of a group gets the feed's running counter (0, 1, 2, ...
 * over all groups in vamd_feed_wrote order) unless vamd_feed_ogg_serials, between vamd_feed_buffer and vamd_feed_wrote*,
 * names the first n streams' itself.  Pinned memory: the file arena is sized from the packet arena (about 7 % more).
 * A COMMENT HEADER PER STREAM (title, artist, cover art): vamd_feed_ogg_comments, between vamd_feed_buffer and
 * vamd_feed_wrote*, gives stream s < n of THIS group the comment header comment[s] (bytes[s] long) in place of the feed's
 * own; comment[s] == NULL, and every stream from n on, keeps the feed's.  The packets are copied before the call returns.
 * It holds for that group only -- the slot's next group starts with none -- and a later call for the same group replaces
 * an earlier one.  Each packet is checked as far as its framing goes (Vorbis I 5.2.1): 7 to 2^24 bytes, type 3 + "vorbis",
 * the vendor length and string, the comment count, that many length + bytes pairs and then a byte with bit 0 set, every
 * one of them inside the packet; bytes behind the framing byte are allowed (taggers pad there), the strings are not looked
 * into.  A packet that fails: VAMD_EINVAL, vamd_feed_last_error names the stream's index and what is wrong, and nothing of
 * the call is kept.  VAMD_EINVAL as well: not an Ogg feed, a slot not between buffer and wrote, n < 0, n > max_streams,
 * bytes == NULL with n > 0.  The comment goes to the device with the group and is paged there like any packet: it starts
 * page 1, a long one (a picture) continues over as many pages as it needs, the setup header follows it, and every later
 * page's offset, sequence number and checksum come out of the same walk -- nothing is retagged on the host.  The page
 * table is sized from the group's longest comment, the file arena from the SUM of its comments, not from streams times
 * the longest.  A feed that never makes the call allocates nothing for it and its files are byte for byte what they were.
 *
 * THE LIVE OGG FEED: a live feed's streams as Ogg files, in pieces.
 *     vamd_feed_create_live(...); vamd_feed_ogg_headers_live(f, id, comment, setup)   once, before the first vamd_feed_buffer
 *     slot = vamd_feed_buffer(f, &pcm) ... [vamd_feed_ogg_serials] [vamd_feed_ogg_flush] ... vamd_feed_wrote_live(f, slot, nstreams, frames, close)
 *     vamd_feed_ogg(f, slot, &pieces)                 per stream the NEXT BYTES of its file; vamd_feed_packets unchanged
 * stream_offset[s] .. stream_offset[s + 1] is the next byte range of stream (slot, s)'s file: the pages the stream
 * completed in this group, a whole number of pages (npages[s] of them), empty where it completed none.  A page is handed
 * out once it is closed and never before; unless the caller flushes (below), nothing closes a page but the policy (a
 * silent stream, one one-byte packet per block, completes a page only every 255 packets).  The ranges of a stream over all
 * its groups, up to and including the group that closes it, laid end to end are byte for byte the file the whole-stream Ogg
 * feed makes of the same samples and serial number (where the stream fits one), and in every case the shipped host mux's of
 * its packets: the paging policy above is unchanged, and the result depends on no cut into pieces, write cadence or slice
 * size -- for a feed that never flushes.
 * Between groups the device keeps per stream the paging walk's state (the open page, the next sequence number, the
 * file offset), its serial number and the CARRY: the packets with a segment on the open page -- at most 255 packets and
 * 65 025 bytes, of a packet continued from an earlier page only the rest -- so neither stream length nor memory grows
 * with a stream.  Serial numbers belong to streams: entry s of vamd_feed_ogg_serials names the serial of stream (slot, s)
 * if that stream BEGINS with this group and is ignored for a stream already open; without the call a stream takes the
 * feed's running counter when it begins.  After a close the slot's next piece begins a new file: a bos page, sequence
 * numbers from 0, a new serial.  Comment headers likewise: entry s of vamd_feed_ogg_comments is the comment header of stream
 * (slot, s) if that stream BEGINS with this group and is ignored for a stream already open -- a live stream's header pages
 * all leave with the group that begins it, so nothing of a comment is kept between groups; after a close the slot's next
 * stream takes a new one, or the feed's own.
 * A stream that loses a packet (bits = -1; a non-finite sample): from that group on its ranges are empty and status[s]
 * carries that block's VAMD_STATUS_*, in every group until the stream is closed; the packets carried for its open page
 * are dropped.  Where a whole stream gets NO file, a live stream has already handed pages out: those bytes are a valid
 * Ogg prefix without an end-of-stream page.  Other streams, and the slot's next stream, are untouched.
 * A FLUSH PER WRITE (what ogg_stream_flush() is to a libogg user; a source that plays while it is made): vamd_feed_ogg_flush,
 * between vamd_feed_buffer and vamd_feed_wrote_live, names the streams of THIS group whose open page leaves with the group:
 * flush[s] != 0, s < n <= max_streams, flushes stream (slot, s) behind this group's packets; flush == NULL with n > 0 flushes
 * every one of the first n; streams from n on are not flushed.  A later call for the same group replaces an earlier one, and
 * the slot's next group starts with none.  What a flush does: if the stream's open page holds at least one segment after
 * the group's last packet has been walked, the page is closed there -- exactly as the end of the run closes it, but without
 * flag 0x04.  Its granule position is that of the last packet completed on it, never -1: at a group's end every packet on
 * the open page is complete (so its last lacing value is below 255).  The page leaves with this group's range and
 * npages[s] counts it; the next packet starts a fresh page with the next sequence number.  A flush that finds the open page
 * empty hands out nothing; a flushed 0-frame piece of an open stream hands out the carried packets' page.  Precedence: a
 * close in the same group wins -- the end-of-stream page is what it always was; a stream that begins with the group gets its
 * header pages, then its audio pages, then the flushed one; a stream that is absent, dead (it lost a packet) or not yet
 * begun is untouched, and flushing it is no error.
 * What is claimed of the bytes.  A feed that never makes the call, or flushes no stream, returns byte for byte what it
 * returned before the call existed: its files depend on no cut.  With flushes the file DOES depend on where the flushes fall:
 * it is the shipped host mux's of the same packets with the same flush points (k_ogg.h, ogg_mux_piece), a valid Ogg Vorbis I
 * stream that holds the same packets in the same order as the unflushed file, decodes to the same samples, and is longer by
 * one page header and lacing table per flush that closed a page.  After a flushing group the stream's ranges so far, laid end
 * to end, hold every packet vamd_feed_packets has reported for it, whole: what is still out is only what the encoder itself
 * has not yet determined, fewer than the live feed's retention bound (3 200 samples at 44.1 kHz).  Page table and file arena are sized
 * as before: the flushed page takes the place that the run's last page has in both bounds (k_ogg.h, ogg_live_slots).
 * VAMD_EINVAL, the reason in vamd_feed_last_error: a whole-stream feed, a live feed without Ogg headers, a slot not between
 * buffer and wrote, n < 0, n > max_streams.  The flags ride to the device in the word that already names each stream's begin
 * and close: no copy, launch or wait more. */
typedef struct vamd_feed_ogg_result {
  int64_t nstreams;
  const int64_t *stream_offset;   /* [nstreams + 1]: stream s's file (a live feed: its next piece) is bytes[stream_offset[s] .. stream_offset[s + 1]) */
  const int32_t *npages;          /* [nstreams] pages in that range */
  const uint8_t *status;          /* [nstreams] 0, or the VAMD_STATUS_* of the block that cost the stream its file */
  const uint8_t *bytes;           /* the files, end to end (the lane's pinned file arena; valid until vamd_feed_release) */
  int64_t total_bytes;
} vamd_feed_ogg_result;
int vamd_feed_ogg_headers(vamd_feed *f, const void *id, long id_bytes, const void *comment, long comment_bytes,
                          const void *setup, long setup_bytes);
/* a live feed's (a whole-stream feed answers VAMD_EINVAL); validates as vamd_feed_ogg_headers does */
int vamd_feed_ogg_headers_live(vamd_feed *f, const void *id, long id_bytes, const void *comment, long comment_bytes,
                               const void *setup, long setup_bytes);
int vamd_feed_ogg_serials(vamd_feed *f, int slot, const uint32_t *serials, long n);
/* between vamd_feed_buffer and vamd_feed_wrote / _wrote_v / _wrote_live, like vamd_feed_ogg_serials:
 * comment[s] (bytes[s] long) is the Vorbis comment header of stream s of this group, s < n <= max_streams;
 * comment[s] == NULL: the feed's own (the one given to vamd_feed_ogg_headers[_live]).  Copied before it returns. */
int vamd_feed_ogg_comments(vamd_feed *f, int slot, const void *const *comment, const long *bytes, long n);
/* between vamd_feed_buffer and vamd_feed_wrote_live, like vamd_feed_ogg_serials; this group only: stream s < n is flushed
 * behind the group's packets where flush[s] != 0 (flush == NULL: all of the first n).  A live Ogg feed's only. */
int vamd_feed_ogg_flush(vamd_feed *f, int slot, const uint8_t *flush, long n);
int vamd_feed_ogg(vamd_feed *f, int slot, vamd_feed_ogg_result *out);

#ifdef __cplusplus
}
#endif
#endif /* VORBIS_AMD_H */
