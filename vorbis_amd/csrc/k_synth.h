// k_synth.h -- the decoder's per-block back half, from what the encoder already holds of a block: what vorbis_synthesis()
// leaves in vb->pcm for the block's packet (mapping0_inverse, reference lib/mapping0.c:698-799) and, over a stream's
// blocks, what vorbis_synthesis_blockin() / _pcmout() hand a listener (lib/block.c:779-823).  No bitstream is read: the
// floor posts' integer curve, the residue classes and codebook entries and the floor flags are the encoder's own outputs.
//
//   synth_block   one workgroup per block, a wave per channel:
//     1. the residue, from the ENTRIES (not from iwork: local_book_besterror subtracts the unclamped lattice point, lib/
//        res0.c:338,345, where the index it emits is clamped; what a decoder adds is the entry's vector): res_class /
//        res_entries walked in emission order (stage, partition, stream, vector) with residue_offsets, every entry turned
//        into its vector by the lattice rule (_book_unquantize maptype 1, lib/sharedbook.c) and added into a zeroed
//        spectrum in LDS -- type 1 consecutive (vorbis_book_decodev_add), type 2 interleaved over the bundle's channels
//        (vorbis_book_decodevv_add); lib/res0.c:651-711,757-835.  Within a stage no two vectors touch the same value.
//     2. inverse coupling, steps in reverse order (lib/mapping0.c:754-779), and the floor: out[j] *= FLOOR1_fromdB_LOOKUP[y]
//        with y the integer curve (lib/floor1.c:1041-1080); a channel without a floor is +0.
//     3. mdct_backward (lib/mdct.c:396-490), a wave per channel: the reference's expression trees on the same operands;
//        only who computes an item differs.  The butterflies are the forward transform's (k_transform.h).
//   lap_sample    one decoded sample: the four cases of the windowed overlap-add, two multiplies and one add.
#pragma once
#include "vamd_wave.h"
#include "vamd_params.h"
#include "k_transform.h"
#include "k_couple.h"
#include "k_residue.h"

namespace vamd {

#if VAMD_GPU
#define VAMD_SY_WAVE ((int)(threadIdx.x >> 6))
#define VAMD_SY_NWAVES ((int)(blockDim.x >> 6))
#else
#define VAMD_SY_WAVE 0
#define VAMD_SY_NWAVES 1
#endif

// LDS of synth_block, in 4-byte words: the spectrum [ch][n2], then -- one after the other in time -- the residue walk's
// tables (the stream -> channel map, cls, off, info) and a butterfly vector per wave.  A wave per channel: measured with
// four waves for a stereo block (the walk and the floor twice as wide, two waves idle in the transform) k_synth took 1.55
// against 1.29 ms per 53 163 long blocks -- the chip is full of blocks, and a block's idle waves are other blocks' slots.
#define VAMD_SY_W2_FLOATS(n2) ((VAMD_PW_SIZE(n2) + 3) & ~3)
#define VAMD_SY_RES_INTS(off_ints) (VAMD_MAX_CH + VAMD_RES_CLASS_STRIDE + 2 * (off_ints))
VAMD_HOSTDEV size_t synth_lds_words(int ch, int n2, int waves, int off_ints) {
  const size_t a = (size_t)waves * VAMD_SY_W2_FLOATS(n2), b = (size_t)VAMD_SY_RES_INTS(off_ints);
  return (size_t)ch * n2 + (((a > b ? a : b) + 3) & ~(size_t)3);
}

// mdct_backward, lib/mdct.c:396-490.  in: LDS [n/2], 16-byte aligned; w2: LDS, the padded butterfly vector
// (VAMD_PW_SIZE(n/2) floats); out: [n].  The reference works in place -- in == out, the rotated input in the upper half,
// the bit-reversed vector in the lower -- and its last three loops only move what the first of them computed; here the
// bit-reverse item u, which forms the pairs (w[2u], w[2u+1]) and (w[n/2-2u-2], w[n/2-2u-1]), rotates them straight into
// the four places each ends up in (as the forward transform's last items do).
// Stopwatch marks: 2 the rotation, 3 the butterfly stages, 4 the 32-point groups, 5 bit-reverse + tail.
template <class Team = WaveTeam>
VAMD_DEV void mdct_backward_wave(const XformP &P, const float *in, float *w2, float *__restrict__ out, PhaseClock &pc, const Team &tm = Team()) {
  const int n = P.n, n2 = n >> 1, n4 = n >> 2, n8 = n >> 3, log2n = P.log2n;
  const float *__restrict__ trig = P.trig;
  // rotate (:403-429): iteration m of both loops reads the same eight inputs
  TEAM_EACH(m, n8 >> 1, tm) {
    const F4 a = *(const F4 *)(in + n2 - 8 - 8 * m), c = *(const F4 *)(in + n2 - 4 - 8 * m);
    const F4 T = *(const F4 *)(trig + n4 + 4 * m), U = *(const F4 *)(trig + n4 - 4 - 4 * m);
    F2 o0, o1, q0, q1;
    o0.x = -a.w * T.w - a.y * T.z;
    o0.y = a.y * T.w - a.w * T.z;
    o1.x = -c.w * T.y - c.y * T.x;
    o1.y = c.y * T.y - c.w * T.x;
    q0.x = c.x * U.w + c.z * U.z;
    q0.y = c.x * U.z - c.z * U.w;
    q1.x = a.x * U.y + a.z * U.x;
    q1.y = a.x * U.x - a.z * U.y;
    const int lo = n4 - 4 - 4 * m, hi = n4 + 4 * m;
    *(F2 *)(w2 + VAMD_PW(lo)) = o0;
    *(F2 *)(w2 + VAMD_PW(lo + 2)) = o1;
    *(F2 *)(w2 + VAMD_PW(hi)) = q0;
    *(F2 *)(w2 + VAMD_PW(hi + 2)) = q1;
  }
  tm.sync();
  pc.mark(2);
  // mdct_butterflies on the upper half (:316-336), as mdct_forward_wave runs them: two stages a trip through LDS where
  // there are two to take, then the 32-point groups in registers
  auto bfly = [](F2 &a, F2 &b, const F2 T) {
    const float r0 = a.x - b.x, r1 = a.y - b.y;
    a.x += b.x;
    a.y += b.y;
    b.x = r1 * T.y + r0 * T.x;
    b.y = r1 * T.x - r0 * T.y;
  };
  auto stage_trig = [&](int s, int q) { return *(const F2 *)(trig + (4 << s) * q); };
  const int nstages = log2n - 6;
  int s = 0;
  for (; s + 1 < nstages; s += 2) {
    const int pts = n2 >> s, lq = log2n - 4 - s;
    TEAM_EACH(g, n8 >> 1, tm) {
      const int j = g >> lq, q = g & ((1 << lq) - 1);
      const int base = pts * j - 2 - 2 * q;
      F2 *pA = (F2 *)(w2 + VAMD_PW(base + pts)), *pB = (F2 *)(w2 + VAMD_PW(base + (pts >> 1)));
      F2 *pC = (F2 *)(w2 + VAMD_PW(base + 3 * (pts >> 2))), *pD = (F2 *)(w2 + VAMD_PW(base + (pts >> 2)));
      const F2 Tab = stage_trig(s, q), Tcd = stage_trig(s, q + (pts >> 3)), T1 = stage_trig(s + 1, q);
      F2 A = *pA, B = *pB, C = *pC, D = *pD;
      bfly(A, B, Tab);
      bfly(C, D, Tcd);
      bfly(A, C, T1);
      bfly(B, D, T1);
      *pA = A;
      *pB = B;
      *pC = C;
      *pD = D;
    }
    tm.sync();
  }
  for (; s < nstages; s++) {
    const int pts = n2 >> s, lper = log2n - 3 - s;
    TEAM_EACH(g, n8, tm) {
      const int j = g >> lper, q = g & ((1 << lper) - 1);
      F2 *pa = (F2 *)(w2 + VAMD_PW(pts * j + pts - 2 - 2 * q)), *pb = (F2 *)(w2 + VAMD_PW(pts * j + (pts >> 1) - 2 - 2 * q));
      F2 a = *pa, b = *pb;
      bfly(a, b, stage_trig(s, q));
      *pa = a;
      *pb = b;
    }
    tm.sync();
  }
  pc.mark(3);
  TEAM_EACH(g, n2 / 32, tm) {
    F2 *pg = (F2 *)(w2 + 34 * g);
    F2 e[16];
#pragma unroll
    for (int k = 0; k < 16; k++) e[k] = pg[k];
#pragma unroll
    for (int a = 0; a < 8; a++) {
      const PairOp r = bfly_level32(a, e[a], e[8 + a]);
      e[a] = r.lo;
      e[8 + a] = r.hi;
    }
#pragma unroll
    for (int h = 0; h < 2; h++) {
#pragma unroll
      for (int b2 = 0; b2 < 4; b2++) {
        const PairOp r = bfly_level16(b2, e[8 * h + b2], e[8 * h + 4 + b2]);
        e[8 * h + b2] = r.lo;
        e[8 * h + 4 + b2] = r.hi;
      }
    }
#pragma unroll
    for (int o = 0; o < 4; o++) {
      float v[8] = {e[4 * o].x, e[4 * o].y, e[4 * o + 1].x, e[4 * o + 1].y, e[4 * o + 2].x, e[4 * o + 2].y, e[4 * o + 3].x, e[4 * o + 3].y};
      bfly_level8(v);
#pragma unroll
      for (int k = 0; k < 4; k++) {
        F2 t;
        t.x = v[2 * k];
        t.y = v[2 * k + 1];
        pg[4 * o + k] = t;
      }
    }
  }
  tm.sync();
  pc.mark(4);
  // mdct_bitreverse (:346-394) and the rotate / negate / copy tail (:436-489)
  TEAM_EACH(u, n8, tm) {
    I2 bi;
    if (P.bitrev_std) {  // lib/mdct.c:77-88
      bi.y = (int)(brev32((unsigned)u) >> (32 - (log2n - 1)));
      bi.x = ((~bi.y) & ((1 << (log2n - 1)) - 1)) - 1;
    } else {
      bi = *(const I2 *)(P.bitrev + 2 * u);
    }
    const F2 x0 = *(const F2 *)(w2 + VAMD_PW(bi.x));
    const F2 x1 = *(const F2 *)(w2 + VAMD_PW(bi.y));
    const F2 T = *(const F2 *)(trig + n + 2 * u);
    float r0 = x0.y - x1.y;
    float r1 = x0.x + x1.x;
    const float r2 = r1 * T.x + r0 * T.y;
    const float r3 = r1 * T.y - r0 * T.x;
    r0 = (x0.y + x1.y) * .5f;
    r1 = (x0.x - x1.x) * .5f;
    F2 lo, hi;
    lo.x = r0 + r2;
    lo.y = r1 + r3;
    hi.x = r0 - r2;
    hi.y = r3 - r1;
    // item i of the tail's first loop reads (w[2i], w[2i+1]): i = u takes lo, i = n/4-1-u takes hi.  Its first result ends
    // up at out[n/4-1-i] and, negated, at out[n/4+i]; its second, negated, at out[3n/4-1-i] and out[3n/4+i].
    auto tail = [&](const F2 x, int i) {
      const F2 R = *(const F2 *)(trig + n2 + 2 * i);
      const float A = x.x * R.y - x.y * R.x;
      const float B = -(x.x * R.x + x.y * R.y);
      out[n4 - 1 - i] = A;
      out[n4 + i] = -A;
      out[n2 + n4 - 1 - i] = B;
      out[n2 + n4 + i] = B;
    };
    tail(lo, u);
    tail(hi, n4 - 1 - u);
  }
  tm.sync();
  pc.mark(5);
}

// component `digit` of a lattice book's vector (_book_unquantize maptype 1): the quantlist runs ze, ze-1, ze+1, ze-2, ... --
// the order local_book_besterror numbers its steps in (lib/res0.c:336,343) -- and a step v is worth v * delta + minval
VAMD_HOSTDEV float synth_lattice_value(int digit, int ze, int delta, int minval) {
  const int v = (digit & 1) ? ze - ((digit + 1) >> 1) : ze + (digit >> 1);
  return (float)(v * delta + minval);
}

// The residue books whose values are NOT that lattice (a setup made from a stream's own headers, vamd_headers.h: explicit
// value lists, non-integer steps, q_sequencep, a quantlist in another order): component j of entry e of book b is
// values[book_off[b] + e * dim + j], the float _book_unquantize leaves (lib/sharedbook.c:285-334); book_off[b] < 0: b is
// a lattice book.  Only the TABLE form of synth_residue reads it.
struct ValueP {
  const int *book_off;   // [nbooks]
  const float *values;
};

// One submap's residue added into the spectrum (res1_inverse / res2_inverse with the entropy decode already done).
//   TABLE: a book's vectors come from ValueP where it has a value list -- the same stage order, the same positions, one
//          float addition per component as without.  A setup whose residue books are all lattice books never takes it.
//   BOUNDED: the rows of a packet that stopped being read early (k_unpack.h, the keep policy): res_count[1] is the number of
//          entries READ, and a vector whose place in reading order (base + v: stage-major, slots ascending, as the rows are
//          written) is at or past it is not added.  Exact: a slot's stage-0 offset depends only on the classes of the slots
//          before it, which were read, and every stage behind the stop begins at or past the count.  The other forms add a
//          vector beyond R.cap as entry 0, which the encoder's rows rely on; only the decoder under that policy takes this one.
//   chans LDS [VAMD_MAX_CH]: the bundle's channels in order (type 2), or those of them that take part (type 1: the
//                            streams, lib/res0.c:757-767); filled here
//   coded                    bit c: channel c takes part in a residue (mapping0_inverse's nonzero[], :715-733)
//   res_class / res_entries / res_count: this submap's rows of one block (k_residue.h)
//   spec LDS [ch][n2]; cls LDS [slots]; off LDS [stages*slots + 1]; info LDS [stages*slots]
template <bool TABLE = false, bool BOUNDED = false>
VAMD_DEV void synth_residue(const ResP &R, const ChMap &cm, int sm, int ch, int n2, unsigned coded, const int *__restrict__ res_class,
                            const unsigned short *__restrict__ res_entries, const int *__restrict__ res_count, float *spec,
                            int *chans, int *cls, int *off, int *info, const ValueP &V = ValueP()) {
  const vamd_residue_tab &t = *R.tab;
  const int slots = res_count[0];
  if (slots <= 0 || slots > R.slots) return;  // no channel of the bundle is coded: res*_inverse reads nothing
  const int partvals = R.partvals, ns = slots / partvals, spp = t.grouping, stages = t.stages, bundle = R.bundle;
  const bool interleaved = t.type == 2;
  const int count = BOUNDED ? res_count[1] : 0;
  if (TEAM_LEADER) {
    int k = 0;
    for (int c = 0; c < ch; c++)
      if (cm.sub[c] == sm && (interleaved || ((coded >> c) & 1))) chans[k++] = c;
    for (; k < VAMD_MAX_CH; k++) chans[k] = 0;  // (every entry names a channel, whatever the rows' stream count says)
  }
  TEAM_FOR(i, slots) {  // (a class indexes the setup's tables: kept inside them whatever the row holds)
    const int c = res_class[i];
    cls[i] = c < 0 ? 0 : (c >= R.nparts ? R.nparts - 1 : c);
  }
  TEAM_SYNC();
  residue_offsets(R, slots, cls, off, info);
  for (int s = 0; s < stages; s++) {
    const int *so = off + s * slots;
    const int base = so[0], total = so[slots] - base;
    TEAM_FOR(v, total) {
      if (BOUNDED && base + v >= count) continue;
      int lo = 0, hi = slots - 1;  // the slot whose vectors include v (residue_block's search)
      while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (so[mid] - base <= v) lo = mid; else hi = mid - 1;
      }
      const int q = lo, k = v - (so[q] - base);
      const int i = q / ns, strm = q - i * ns;
      const int bn = info[s * slots + q];
      const vamd_book_tab &bk = R.books[bn];
      const int dim = bk.dim, qv = bk.quantvals, ze = qv >> 1, delta = bk.delta, minval = bk.minval;
      unsigned e = base + v < R.cap ? (unsigned)res_entries[base + v] : 0u;
      const int pos = t.begin + i * spp + k * dim;
      // (an entry number is k_unpack's: below the book's entries; held there all the same, the list is read by it)
      const float *row = nullptr;
      if (TABLE) {
        const int at = V.book_off[bn];
        if (at >= 0) row = V.values + (size_t)at + (size_t)(e < (unsigned)bk.entries ? e : 0u) * dim;
      }
      for (int j = 0; j < dim; j++) {
        float val;
        if (TABLE && row) {
          val = row[j];
        } else {
          const unsigned d = e / (unsigned)qv;
          val = synth_lattice_value((int)(e - d * (unsigned)qv), ze, delta, minval);
          e = d;
        }
        float *p;
        if (interleaved) {
          const int at = pos + j, bin = at / bundle;
          p = spec + chans[at - bin * bundle] * n2 + bin;
        } else {
          p = spec + chans[strm & (VAMD_MAX_CH - 1)] * n2 + pos + j;
        }
        *p += val;
      }
    }
    TEAM_SYNC();
  }
}

// The floor's range as the two sides hold it.  floor1_pack writes it as a bit count, ilog(postlist[1] - 1), and floor1_unpack
// rebuilds postlist[1] = 1 << that (lib/floor1.c:102-103,147,160): the same number where it is a power of two, as a floor over
// the whole spectrum has it.  The LFE floor of libvorbisenc's 5.1 setups has postlist[1] = 12; a decoder draws its one line
// to x = 16, and the encoder's integer curve (ilogmask) is not what a listener's floor is.  Such a floor is drawn here again,
// the decoder's way, where it is one line (two posts); with more posts the last used post's place would have to come from the
// posts' flags, and synth_floor_ranges() says no.
struct SynthFloorP {
  int enc_n[VAMD_MAX_SUBMAPS], dec_n[VAMD_MAX_SUBMAPS];
};
inline bool synth_floor_ranges(const FloorP &F0, const FloorP &F1, int submaps, int n2, SynthFloorP *o) {
  bool ok = true;
  for (int sm = 0; sm < VAMD_MAX_SUBMAPS; sm++) {
    const FloorP &F = sm && sm < submaps ? F1 : F0;
    int bits = 0;
    for (unsigned v = F.look_n > 0 ? (unsigned)(F.look_n - 1) : 0; v; v >>= 1) bits++;  // ov_ilog
    o->enc_n[sm] = F.look_n, o->dec_n[sm] = 1 << bits;
    if (o->dec_n[sm] != F.look_n && (F.posts != 2 || F.look_n >= n2)) ok = false;
  }
  return ok;
}
// render_line (lib/floor1.c:347-374) at x, for the line from (0, y0) to (x1, y1): k steps of its error walk take the
// long step floor(k * ady / adx) times
VAMD_DEV int synth_line_at(int x, int x1, int y0, int y1) {
  const int dy = y1 - y0, base = dy / x1;
  const int ady = (dy < 0 ? -dy : dy) - (base < 0 ? -base : base) * x1;
  return y0 + x * base + (dy < 0 ? -1 : 1) * ((x * ady) / x1);
}

// One block: vb->pcm [ch][n] as vorbis_synthesis() leaves it (see the head of the file).
//   post_valid [ch]; ilogmask [ch][n2]; res_class [submaps][VAMD_RES_CLASS_STRIDE], res_entries [row], res_count [submaps][2]
//   lds: synth_lds_words(ch, n2, waves, off_ints) words, 16-byte aligned
//   stopwatch marks (per wave): 0 the residue walk (the spectrum's zeroing included), 1 inverse coupling + floor, 2-5 the transform
template <bool TABLE = false, bool BOUNDED = false>
VAMD_DEV void synth_block(const XformP &X, const ResP &R0, const ResP &R1, const ChMap &cm, const CoupleP &C, const SynthFloorP &S, int ch, int off_ints,
                          const int *__restrict__ post_valid, const ilog_t *__restrict__ ilogmask, const int *__restrict__ res_class,
                          const unsigned short *__restrict__ res_entries, const int *__restrict__ res_count, float *lds,
                          float *__restrict__ out, PhaseClock &pc, const ValueP &V = ValueP()) {
  const int n = X.n, n2 = n >> 1;
  float *spec = lds;
  int *chans = (int *)(spec + (size_t)ch * n2), *cls = chans + VAMD_MAX_CH, *off = cls + VAMD_RES_CLASS_STRIDE, *info = off + off_ints;
  // which channels have a floor, and which take part in a residue: coupling dirties the latter (lib/mapping0.c:715-733)
  unsigned floored = 0;
  for (int c = 0; c < ch; c++) floored |= (post_valid[c] ? 1u : 0u) << c;
  unsigned coded = floored;
#pragma unroll
  for (int i = 0; i < VAMD_MAX_COUPLING; i++)
    if (i < C.coupling_steps && (((coded >> C.mag[i]) | (coded >> C.ang[i])) & 1u)) coded |= (1u << C.mag[i]) | (1u << C.ang[i]);
  TEAM_FOR(i, ch * n2) spec[i] = 0.f;
  TEAM_SYNC();
  for (int sm = 0; sm < cm.submaps; sm++) {
    const ResP &R = sm ? R1 : R0;
    synth_residue<TABLE, BOUNDED>(R, cm, sm, ch, n2, coded, res_class + R.cls_base, res_entries + R.ent_base, res_count + 2 * sm, spec, chans, cls,
                         off, info, V);
  }
  pc.mark(0);
  // four bins a trip: every channel's four curve bytes are one load, all of them in flight before the first is used
  TEAM_FOR(q, n2 >> 2) {
    const int j = q << 2;
    unsigned yw[VAMD_MAX_CH];
#pragma unroll
    for (int c = 0; c < VAMD_MAX_CH; c++) yw[c] = c < ch ? *(const unsigned *)(ilogmask + c * n2 + j) : 0u;
#pragma unroll
    for (int i = VAMD_MAX_COUPLING - 1; i >= 0; i--)
      if (i < C.coupling_steps) {  // lib/mapping0.c:754-779
        float m4[4], a4[4];
        F4 *pm = (F4 *)(spec + C.mag[i] * n2 + j), *pa = (F4 *)(spec + C.ang[i] * n2 + j);
        f4_get(*pm, m4);
        f4_get(*pa, a4);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const float mag = m4[k], ang = a4[k];
          if (mag > 0) {
            if (ang > 0) {
              a4[k] = mag - ang;
            } else {
              a4[k] = mag;
              m4[k] = mag + ang;
            }
          } else {
            if (ang > 0) {
              a4[k] = mag + ang;
            } else {
              a4[k] = mag;
              m4[k] = mag - ang;
            }
          }
        }
        *pm = f4_make(m4);
        *pa = f4_make(a4);
      }
#pragma unroll
    for (int c = 0; c < VAMD_MAX_CH; c++)
      if (c < ch) {  // floor1_inverse2, lib/floor1.c:1041-1080
        F4 *p = (F4 *)(spec + c * n2 + j);
        float v[4];
        f4_get(*p, v);
        const ilog_t *curve = ilogmask + c * n2;
        const int en = cm.sub[c] ? S.enc_n[1] : S.enc_n[0], dn = cm.sub[c] ? S.dec_n[1] : S.dec_n[0];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          int y = (int)((yw[c] >> (8 * k)) & 255u);
          if (dn != en) y = j + k < dn ? synth_line_at(j + k, dn, curve[0], curve[en]) : curve[en];  // (one line, en < n2: synth_floor_ranges)
          v[k] = ((floored >> c) & 1u) ? v[k] * floor1_fromdB(y) : 0.f;
        }
        *p = f4_make(v);
      }
  }
  TEAM_SYNC();  // (the residue tables are dead: the butterfly vectors take their place)
  pc.mark(1);
  float *w2 = (float *)chans + (size_t)VAMD_SY_WAVE * VAMD_SY_W2_FLOATS(n2);
  for (int c = VAMD_SY_WAVE; c < ch; c += VAMD_SY_NWAVES) mdct_backward_wave(X, spec + (size_t)c * n2, w2, out + (size_t)c * n, pc);
}

// ---- the lap: vorbis_synthesis_blockin's windowed overlap-add (lib/block.c:779-823) as a gather ----------------------------
// A stream's decoded sample lies between the centres of two of its blocks, A before and B after; sample 0 is the first
// block's centre (the stream's first sample; the first block gives no output, :835-837).
// The reference keeps A's second half in v->pcm and adds B's first half into it; each output sample reads at most one
// value of each.
struct LapP {
  int ch, bs0, bs1;
  const float *win0, *win1;       // the rising half windows [bs/2] (XformP::win_short / win_long)
  const int *order;               // a group's blocks in stream order: W << 30 | index inside W's batch
  const long long *stream_start;  // [streams + 1] into order[]
  const long long *src0, *src1;   // [blocks of the class]: the block's first sample in its stream's buffer (vamd_stream_plan::src)
  const float *synth0, *synth1;   // [blocks of the class][ch][bs]: synth_block's output per size class
};

// the centre of block k of order[], in the coordinates of src[]
VAMD_DEV long long lap_centre(const LapP &L, long long k) {
  const int o = L.order[k], i = o & 0x3fffffff;
  return ((o >> 30) & 1) ? L.src1[i] + (L.bs1 >> 1) : L.src0[i] + (L.bs0 >> 1);
}

// the block B of stream [k0, k1) with centre(B-1) <= at < centre(B); centre(k0) <= at < centre(k1-1)
VAMD_DEV long long lap_find(const LapP &L, long long k0, long long k1, long long at) {
  long long lo = k0 + 1, hi = k1 - 1;  // first k with centre(k) > at
  while (lo < hi) {
    const long long mid = (lo + hi) >> 1;
    if (lap_centre(L, mid) > at) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// the sample at `at` (src[] coordinates) of channel c, B = block k of order[]
VAMD_DEV float lap_sample(const LapP &L, long long k, long long at, int c) {
  const int oa = L.order[k - 1], ob = L.order[k];
  const int lW = (oa >> 30) & 1, W = (ob >> 30) & 1;
  const int na = lW ? L.bs1 : L.bs0, nb = W ? L.bs1 : L.bs0;
  const float *A = (lW ? L.synth1 : L.synth0) + ((size_t)(oa & 0x3fffffff) * L.ch + c) * na + (na >> 1);  // A's second half
  const float *B = (W ? L.synth1 : L.synth0) + ((size_t)(ob & 0x3fffffff) * L.ch + c) * nb;
  const int i = (int)(at - lap_centre(L, k - 1));
  const int n0 = L.bs0 >> 1, n1 = L.bs1 >> 1;
  if ((unsigned)i >= (unsigned)((na >> 2) + (nb >> 2))) return 0.f;  // (two blocks' centres are never further apart: lib/block.c:840-842)
  if (lW == W) {  // large/large, small/small
    const int h = na >> 1;
    const float *w = W ? L.win1 : L.win0;
    return A[i] * w[h - i - 1] + B[i] * w[i];
  }
  const int d = n1 / 2 - n0 / 2;
  if (lW) {  // large/small: A's flat part, then the short window
    if (i < d) return A[i];
    const int j = i - d;
    return A[i] * L.win0[n0 - j - 1] + B[j] * L.win0[j];
  }
  // small/large: the short window, then B's flat part
  if (i < n0) return A[i] * L.win0[n0 - i - 1] + B[d + i] * L.win0[i];
  return B[d + i];
}

// ---- the lap for a window: frames [a, a + F) of a stream out of the blocks around them alone (vamd_decode_window.h) ---------
// Blocks [k0, k1) of order[] are the window's own, src[] in the stream's coordinates: centre(k0) <= a and
// a + F - 1 < centre(k1 - 1) (vamd_decode_window_plan.h picks the fewest such).  Thread q of the window takes frames
// 4q .. 4q + 3 as k_lap's does: one search for the block pair of the first, a step along order[] where a later one lies
// past the pair's end.  Channel c goes to out[c * stride ..]: stride >= F (a crop's row may be longer than what the file
// still holds).  A window the plan did not bound as above is left alone.
VAMD_DEV void lap_window(const LapP &L, long long k0, long long k1, long long a, long long F, long long stride, long long q, float *out) {
  if (k1 - k0 < 2 || a < lap_centre(L, k0)) return;
  const long long span = lap_centre(L, k1 - 1) - a, count = F < span ? F : span;
  if (4 * q >= count) return;
  long long k = lap_find(L, k0, k1, a + 4 * q), end = lap_centre(L, k);
  for (long long t = 4 * q; t < 4 * q + 4 && t < count; t++) {
    while (a + t >= end && k < k1 - 1) end = lap_centre(L, ++k);
    for (int c = 0; c < L.ch; c++) out[c * stride + t] = lap_sample(L, k, a + t, c);
  }
}

// ---- the lap for segments: the runs of frames a reader keeps of a stream (vamd_decode_plan.h, decode_plan_build_marked) ------
// A stream whose page granules cut frames out of its middle, or whose file is several links, is a few windows laid end to
// end: each row is one lap_window call, its blocks [k0, k1) of order[] -- rows of one link share them -- its frames
// [first, first + count) of those blocks' span, at out + `out`, channel c `stride` floats further on.
struct LapSegment {
  long long k0, k1, first, count, stride, out;
};
VAMD_DEV void lap_segment(const LapP &L, const LapSegment &g, long long q, float *out) { lap_window(L, g.k0, g.k1, g.first, g.count, g.stride, q, out + g.out); }

// ---- the lap in the caller's format (include/vorbis_amd.h, vamd_decode_output) -----------------------------------------------
// D is a VAMD_PCM_* element type, IL the layout.  <VAMD_PCM_F32, planar> is the code above, untouched; the other seven go
// through lap_row below.  The conversions are what the header states: S16 is ov_read's (lib/vorbisfile.c:2018-2036,
// vorbis_ftoi as cvtsd2si rounds: to nearest, ties to even -- x * 32768 is exact in a float, so rintf of it is that
// value), saturating by sign where the reference's instruction gives its "indefinite" result, NaN to 0; F16 and BF16
// round to nearest even.
VAMD_DEV uint32_t pcm_bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}
VAMD_DEV int16_t pcm_s16(float x) {
  const float r = rintf(x * 32768.f);  // (v_cvt_i32_f32 truncates: round first)
  if (!(r == r)) return 0;
  return (int16_t)(int)(r > 32767.f ? 32767.f : r < -32768.f ? -32768.f : r);
}
VAMD_DEV uint16_t pcm_f16(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const _Float16 h = (_Float16)x;  // (v_cvt_f16_f32; the compiler packs pairs)
  uint16_t o;
  memcpy(&o, &h, 2);
  return o;
#else  // (a host compiler without _Float16: the same rounding by hand; tests/test_decode_formats_cpu.py holds it to torch's)
  const uint32_t u = pcm_bits(x), sign = (u >> 16) & 0x8000u, m = u & 0x7fffffffu;
  if (m > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);
  if (m < 0x38800000u) return (uint16_t)(sign | (uint32_t)rintf(fabsf(x) * 16777216.f));  // below 2^-14: a multiple of 2^-24
  uint32_t r = m - 0x38000000u;
  r = (r + 0xfffu + ((r >> 13) & 1u)) >> 13;
  return (uint16_t)(sign | (r < 0x7c00u ? r : 0x7c00u));
#endif
}
VAMD_DEV uint16_t pcm_bf16(float x) {
  const uint32_t u = pcm_bits(x);
  if ((u & 0x7fffffffu) > 0x7f800000u) return 0x7fc0;
  return (uint16_t)((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

template <int D> struct PcmElem { typedef float T; };  // VAMD_PCM_F32
template <> struct PcmElem<1> { typedef int16_t T; };   // VAMD_PCM_S16
template <> struct PcmElem<2> { typedef uint16_t T; };  // VAMD_PCM_F16, as bits
template <> struct PcmElem<3> { typedef uint16_t T; };  // VAMD_PCM_BF16, as bits
template <int D> VAMD_DEV typename PcmElem<D>::T pcm_from(float x) {
  if constexpr (D == 1) return pcm_s16(x);
  else if constexpr (D == 2) return pcm_f16(x);
  else if constexpr (D == 3) return pcm_bf16(x);
  else return x;
}

// The output policy: a thread takes `per_thread` consecutive ELEMENTS of a row in `stores` 16-byte stores of `wide`
// elements.  A planar row is one channel's frames; an interleaved row is all of a stream's (or window's, or segment's)
// frames x channels.  Eight elements a thread everywhere -- what k_lap's thread gathers of a stereo stream behind one
// search: DESIGN.md section 5 has what else was tried (more loses: the gather is bound by latency, not by stores).
template <int D, bool IL> struct PcmOut {
  typedef typename PcmElem<D>::T T;
  static constexpr int wide = 16 / (int)sizeof(T);
  static constexpr int stores = IL && sizeof(T) == 4 ? 2 : 1;
  static constexpr int per_thread = stores * wide;
};
template <class T> struct alignas(16) PcmWide { T v[16 / sizeof(T)]; };

// where a thread stands in order[]: the block pair of frame `frame`, found once and kept while the thread's rows (a planar
// window's channels) begin at the same frame -- they do wherever the rows are equally aligned
struct LapAt {
  long long frame = -1, k = 0, end = 0;
};

// Elements [0, n) of one row, at `row`: element e is frame a + e of channel c0 (planar), or frame a + e / ch of channel
// e % ch (interleaved), out of blocks [k0, k1) of order[] as lap_window takes them.  The row may begin at any element:
// thread 0 takes the elements in front of the first 16-byte boundary one by one, thread q >= 1 the q-th group of
// per_thread behind it in whole 16-byte stores, and one by one where the row ends inside one.  No element outside
// [0, n) is touched.  A row needs threads 0 .. n / per_thread + 1.
template <int D, bool IL>
VAMD_DEV void lap_row(const LapP &L, long long k0, long long k1, long long a, long long n, int c0, long long q, typename PcmElem<D>::T *row, LapAt &at) {
  typedef PcmOut<D, IL> O;
  typedef typename O::T T;
  long long head = (long long)(((16 - ((uintptr_t)row & 15)) & 15) / sizeof(T));
  if (head > n) head = n;
  const long long lo = q ? head + (q - 1) * O::per_thread : 0;
  long long hi = q ? lo + O::per_thread : head;
  if (hi > n) hi = n;
  if (lo >= hi) return;
  long long t = IL ? lo / L.ch : lo;
  int c = IL ? (int)(lo - t * L.ch) : c0;
  if (at.frame != t) at.frame = t, at.k = lap_find(L, k0, k1, a + t), at.end = lap_centre(L, at.k);
  long long k = at.k, end = at.end;
#pragma unroll
  for (int s = 0; s < O::stores; s++) {
    const long long e = lo + s * O::wide;
    const bool whole = q && hi - e >= O::wide;
    PcmWide<T> pack;
#pragma unroll
    for (int j = 0; j < O::wide; j++)
      if (e + j < hi) {
        while (a + t >= end && k < k1 - 1) end = lap_centre(L, ++k);
        const T v = pcm_from<D>(lap_sample(L, k, a + t, c));
        if (whole) pack.v[j] = v;
        else row[e + j] = v;
        if (!IL) t++;
        else if (++c == L.ch) c = 0, t++;
      }
    if (whole) *(PcmWide<T> *)(row + e) = pack;
  }
}

// lap_window in format <D, IL>: the same window, the same bounds.  Planar, channel c's row is out + c * stride; interleaved,
// the window is one row of count * ch elements at out and `stride` is not read.
template <int D, bool IL>
VAMD_DEV void lap_window_as(const LapP &L, long long k0, long long k1, long long a, long long F, long long stride, long long q, typename PcmElem<D>::T *out) {
  if (k1 - k0 < 2 || a < lap_centre(L, k0)) return;
  const long long span = lap_centre(L, k1 - 1) - a, count = F < span ? F : span;
  LapAt at;
  if (IL) lap_row<D, true>(L, k0, k1, a, count * L.ch, 0, q, out, at);
  else
    for (int c = 0; c < L.ch; c++) lap_row<D, false>(L, k0, k1, a, count, c, q, out + c * stride, at);
}
// the threads a window of F frames needs (the grid's sizing and the kernels' loops)
template <int D, bool IL> VAMD_DEV long long lap_threads_as(long long F, int ch) { return (IL ? F * ch : F) / PcmOut<D, IL>::per_thread + 2; }

// ---- the lap across pieces: a continuing stream's last block, carried between calls (vamd_decode_live.h) --------------------
// lap_sample reads, of the block in front, its second half and its size class.  A live decoder keeps that half per slot
// in `carry` ([slots][ch][bs1/2]; a short block's half fills the front of its row) and, in the next call, stands it in an
// extra row of its size class behind the rows k_synth wrote, so that the lap above runs on the call's plan as on any other.
struct CarryRow {
  int slot, W, row;  // the slot's row of `carry`; the size class; the block's row in that class's synth buffer
};
struct CarryP {
  int ch, bs0, bs1;
  float *carry;
  float *synth0, *synth1;  // [rows of the class][ch][bs]
};
VAMD_DEV float *carry_slot_half(const CarryP &P, const CarryRow &r, int c) { return P.carry + ((size_t)r.slot * P.ch + c) * (size_t)(P.bs1 >> 1); }
VAMD_DEV float *carry_block_half(const CarryP &P, const CarryRow &r, int c) {
  const int n = r.W ? P.bs1 : P.bs0;
  return (r.W ? P.synth1 : P.synth0) + ((size_t)r.row * P.ch + c) * (size_t)n + (n >> 1);
}
// channel c of a continuing stream: the slot's carried half into the second half of the stream's extra row.  The row's
// first half is never read (lap_sample reads A from na/2 on, and an extra row is only ever an A) and is left as it is.
VAMD_DEV void decode_carry_in(const CarryP &P, const CarryRow &r, int c) {
  const F4 *src = (const F4 *)carry_slot_half(P, r, c);
  F4 *dst = (F4 *)carry_block_half(P, r, c);
  TEAM_FOR(i, (r.W ? P.bs1 : P.bs0) >> 3) dst[i] = src[i];
}
// channel c of a stream that goes on: the second half of its last block's row into the slot's carry
VAMD_DEV void decode_carry_out(const CarryP &P, const CarryRow &r, int c) {
  const F4 *src = (const F4 *)carry_block_half(P, r, c);
  F4 *dst = (F4 *)carry_slot_half(P, r, c);
  TEAM_FOR(i, (r.W ? P.bs1 : P.bs0) >> 3) dst[i] = src[i];
}

}  // namespace vamd
