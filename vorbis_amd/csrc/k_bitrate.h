// k_bitrate.h -- the bitrate manager's choice among a block's fifteen candidate packets: vorbis_bitrate_addblock()
// (reference lib/bitrate.c:73-227), per stream.  The manager does not feed back into the analysis -- mapping0_forward
// prepares the same fifteen candidates whatever it will pick -- so the whole of it is a serial walk over the blocks'
// candidate SIZES, one stream after the other's state: one lane per stream (k_bitrate_walk, vamd_hip.hip), with the
// reference's fp64 floater and its `long` (int64) reservoirs.
//
// bitrate_addblock() below is the one body: the library compiles it for gfx950, the CPU suite compiles this very file
// with the host compiler (tests/test_bitrate_walk.py).  Both builds are -ffp-contract=off (the floater's update is a
// divide, a multiply and an add, rounded one by one as C rounds them), rint() is round-half-even on both (v_rndne_f64
// on the device), and every `long x double` of the reference is kept as C does it: the long converted to double, the
// product or sum in double, the result truncated back where the reference assigns it to a long / int.
#pragma once
#include <math.h>
#include <stdint.h>
#include "vorbis_amd.h"

#if defined(__HIPCC__)
#define VAMD_BR_FN __host__ __device__ inline
#else
#define VAMD_BR_FN inline
#endif

namespace vamd {

// what bitrate_addblock did besides choosing (the CPU suite checks that every branch is exercised)
enum {
  BR_SLEW_CLAMPED = 1,  // the avg floater's slew hit +-slewlimit (lib/bitrate.c:133-134)
  BR_MIN_FORCED = 2,    // the minimum pushed the choice up (:143-150)
  BR_MAX_FORCED = 4,    // the maximum pushed the choice down (:155-161)
  BR_BELOW_ZERO = 8,    // choice < 0: candidate 0, cut to maxsize where it is longer (:167-178)
  BR_TRUNCATED = 16,    // ... and it was cut (oggpack_writetrunc)
  BR_PADDED = 32,       // zero bytes appended up to minsize (:178-190)
};

// The stream's state at its start: what vorbis_bitrate_init left in private_state.bms (lib/bitrate.c:45-53).
VAMD_BR_FN void bitrate_state_init(const vamd_bitrate_tab &t, vamd_bitrate_state &st) {
  st.avgfloat = t.avgfloat;
  st.minmax_reservoir = t.minmax_reservoir;
  st.avg_reservoir = t.avg_reservoir;
  st.pad = 0;
}

// One block through vorbis_bitrate_addblock (lib/bitrate.c:73-227).  bytes[k] = oggpack_bytes(vbi->packetblob[k]) of
// the fifteen candidates, W = vb->W, samples = blocksizes[W] >> 1.  Returns the chosen candidate (bm->choice) and sets
// *final_bytes = oggpack_bytes() of the packet vorbis_bitrate_flushpacket hands out (the candidate cut or zero-padded),
// *flags = the BR_* branches taken.  `st` is updated as bm is.
VAMD_BR_FN int bitrate_addblock(const vamd_bitrate_tab &t, vamd_bitrate_state &st, const int32_t *bytes, int W, int samples,
                                int64_t *final_bytes, int *flags) {
  const int PB = VAMD_PACKETBLOBS;
  int fl = 0;
  int choice = (int)rint(st.avgfloat);                                                         // :82
  int64_t this_bits = (int64_t)bytes[choice] * 8;                                              // :83
  const int64_t min_target_bits = W ? t.min_bitsper * t.short_per_long : t.min_bitsper;        // :84
  const int64_t max_target_bits = W ? t.max_bitsper * t.short_per_long : t.max_bitsper;        // :85
  const int64_t desired_fill = (int64_t)((double)t.reservoir_bits * t.reservoir_bias);         // :87

  // look ahead for avg floater (:100-138)
  if (t.avg_bitsper > 0) {
    double slew = 0.;
    const int64_t avg_target_bits = W ? t.avg_bitsper * t.short_per_long : t.avg_bitsper;      // :103
    const double slewlimit = 15. / t.slew_damp;                                                // :104
    if (st.avg_reservoir + (this_bits - avg_target_bits) > desired_fill) {                     // :117-123
      while (choice > 0 && this_bits > avg_target_bits && st.avg_reservoir + (this_bits - avg_target_bits) > desired_fill) {
        choice--;
        this_bits = (int64_t)bytes[choice] * 8;
      }
    } else if (st.avg_reservoir + (this_bits - avg_target_bits) < desired_fill) {              // :124-130
      while (choice + 1 < PB && this_bits < avg_target_bits && st.avg_reservoir + (this_bits - avg_target_bits) < desired_fill) {
        choice++;
        this_bits = (int64_t)bytes[choice] * 8;
      }
    }
    slew = rint((double)choice - st.avgfloat) / (double)samples * (double)t.rate;              // :132
    if (slew < -slewlimit) slew = -slewlimit, fl |= BR_SLEW_CLAMPED;                           // :133
    if (slew > slewlimit) slew = slewlimit, fl |= BR_SLEW_CLAMPED;                             // :134
    st.avgfloat = st.avgfloat + slew / (double)t.rate * (double)samples;                       // :135
    choice = (int)rint(st.avgfloat);
    this_bits = (int64_t)bytes[choice] * 8;                                                    // :136
  }

  // enforce min (if used) on the current floater (:140-150)
  if (t.min_bitsper > 0) {
    if (this_bits < min_target_bits) {
      while (st.minmax_reservoir - (min_target_bits - this_bits) < 0) {
        fl |= BR_MIN_FORCED;
        choice++;
        if (choice >= PB) break;
        this_bits = (int64_t)bytes[choice] * 8;
      }
    }
  }

  // enforce max (if used) on the current floater (:152-162)
  if (t.max_bitsper > 0) {
    if (this_bits > max_target_bits) {
      while (st.minmax_reservoir + (this_bits - max_target_bits) > t.reservoir_bits) {
        fl |= BR_MAX_FORCED;
        choice--;
        if (choice < 0) break;
        this_bits = (int64_t)bytes[choice] * 8;
      }
    }
  }

  int64_t out_bytes;
  if (choice < 0) {  // :167-178: a smaller candidate is not enough; candidate 0 is truncated
    const int64_t maxsize = (max_target_bits + (t.reservoir_bits - st.minmax_reservoir)) / 8;
    choice = 0;
    fl |= BR_BELOW_ZERO;
    out_bytes = bytes[0];
    if (out_bytes > maxsize) {  // oggpack_writetrunc(packetblob[0], maxsize * 8)
      out_bytes = maxsize;
      fl |= BR_TRUNCATED;
    }
    this_bits = out_bytes * 8;
  } else {  // :178-190: pad the packet with zero bytes up to minsize
    int64_t minsize = (min_target_bits - st.minmax_reservoir + 7) / 8;
    if (choice >= PB) choice = PB - 1;
    minsize -= bytes[choice];
    out_bytes = bytes[choice];
    if (minsize > 0) {  // while(minsize-->0) oggpack_write(packetblob[choice], 0, 8)
      out_bytes += minsize;
      fl |= BR_PADDED;
    }
    this_bits = out_bytes * 8;
  }

  // min and max reservoir (:194-219)
  if (t.min_bitsper > 0 || t.max_bitsper > 0) {
    if (max_target_bits > 0 && this_bits > max_target_bits) {
      st.minmax_reservoir += (this_bits - max_target_bits);
    } else if (min_target_bits > 0 && this_bits < min_target_bits) {
      st.minmax_reservoir += (this_bits - min_target_bits);
    } else {
      // in between: take the reservoir toward but not past desired_fill
      if (st.minmax_reservoir > desired_fill) {
        if (max_target_bits > 0) {
          st.minmax_reservoir += (this_bits - max_target_bits);
          if (st.minmax_reservoir < desired_fill) st.minmax_reservoir = desired_fill;
        } else {
          st.minmax_reservoir = desired_fill;
        }
      } else {
        if (min_target_bits > 0) {
          st.minmax_reservoir += (this_bits - min_target_bits);
          if (st.minmax_reservoir > desired_fill) st.minmax_reservoir = desired_fill;
        } else {
          st.minmax_reservoir = desired_fill;
        }
      }
    }
  }

  // avg reservoir (:222-225)
  if (t.avg_bitsper > 0) {
    const int64_t avg_target_bits = W ? t.avg_bitsper * t.short_per_long : t.avg_bitsper;
    st.avg_reservoir += this_bits - avg_target_bits;
  }

  *final_bytes = out_bytes;
  *flags = fl;
  return choice;
}

// oggpack_bits() of the packet the manager hands out, from the candidate's own bit count `bits` (its bytes: (bits+7)/8):
// untouched, the candidate's; cut, maxsize * 8 (oggpack_writetrunc); padded, eight more per zero byte appended
// (oggpack_write(b, 0, 8) from wherever the last write ended).
VAMD_BR_FN int64_t bitrate_final_bits(int32_t bits, int64_t final_bytes) {
  const int64_t own = ((int64_t)bits + 7) >> 3;
  if (final_bytes < own) return final_bytes * 8;
  return (int64_t)bits + 8 * (final_bytes - own);
}

}  // namespace vamd
