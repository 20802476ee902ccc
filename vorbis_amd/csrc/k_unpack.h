// k_unpack.h -- the decoder's front half: one audio packet's bits turned into the rows k_synth reads (k_synth.h).  The
// inverse of k_pack.h: the packet head (reference lib/synthesis.c:25-88), per channel floor1_inverse1 and the integer
// curve floor1_inverse2 walks (lib/floor1.c:975-1080), per submap the phrase words and codebook entries in the order
// _01inverse / res2_inverse read them (lib/res0.c:651-711,812-871), every codeword by table as decode_packed_entry_number
// finds it (lib/codebook.c:264-365, the tables of lib/sharedbook.c:294-437).
//
// Entropy decode is serial inside a packet and independent between packets: ONE LANE takes one packet, 64 packets a wave.
// The bits come through a 64-bit window in registers, refilled by aligned dword loads; the rows go out to the block's own
// places as they are decoded (scattered stores by nature; the curve four bytes a store).
//
// Safety is structural.  Every loop bound -- posts, partitions, stages, vectors of a partition -- is the setup's, none the
// stream's; a table index taken from the stream is an entry number the decode table produced (< the book's entries, the
// table's builder saw to it) or a digit of one (< the residue's classes), or it is masked to its table (the floor's
// cascade word); every read is held against the packet's end.  A malformed packet ends in a status, with rows that name
// nothing (post_valid and res_count zero): never in an access outside the rows, never in a loop without an end.
//
// TRUNCATED PACKETS -- a deliberate deviation.  libvorbis treats a packet that ends early as "stop working": a floor that
// meets the end is no floor, a residue that meets it keeps what it has (eopbreak, lib/res0.c:650,709-710), and
// vorbis_synthesis returns 0.  Here such a packet carries VAMD_STATUS_TRUNCATED and its stream yields no frames, as a
// decoded feed's stream with a missing packet does.  A bitrate-managed feed's CUT packets (lib/bitrate.c trims a packet to
// the byte count the reservoir allows) are truncated packets in this sense.
#pragma once
#include "vamd_wave.h"
#include "vamd_params.h"
#include "vamd_bind.h"

// per-packet status bits beside VAMD_STATUS_RANGE / _NONFINITE (include/vorbis_amd.h holds the same values)
#define VAMD_STATUS_NOTAUDIO 4    // the packet-type bit is set, the mode number names no mode, or its size class is not the plan's
#define VAMD_STATUS_BADCODE 8     // bits that are no codeword of the book they are read with, or a phrase word beyond the classes
#define VAMD_STATUS_TRUNCATED 16  // the packet ends before the block is complete

// Packets a wave of k_unpack (vamd_kernels.h), the rest of its lanes idle.  Measured (profiles/r22_decode.txt).
#define VAMD_UNPACK_LANES 64

namespace vamd {

// One codebook's decode tables inside the table image (unpack_build_tables, vamd_decode_plan.h): the first level answers the
// next `k` bits of the stream -- {entry, length} for a codeword of at most k bits, else the range [lo, hi) of the list
// of longer codewords that begin with those bits.  The list is sorted by the codeword read most significant bit first
// (bit-reversed as the stream holds it, left aligned in 32 bits): the codeword that matches is the last one not above
// the next 32 bits of the stream, read the same way.
struct UnpackBook {
  int32_t entries, k, nsorted, pad;
  uint32_t off_first;  // uint32 [1 << k][2]: {entry, length} (length > 0), or {lo, hi << 8} (low byte 0)
  uint32_t off_codes;  // uint32 [nsorted]
  uint32_t off_info;   // uint32 [nsorted]: entry | length << 24
  uint32_t pad2;
};
struct UnpackP {
  const unsigned char *tab;  // UnpackBook [nbooks], then the books' arrays; all offsets from here
  int nbooks, modes, modebits;
};

// oggpack_look / oggpack_adv on a packet inside a buffer of whole dwords: bits [pos, end) of words[], least significant first
struct BitIn {
  const uint32_t *words;
  long long nwords, pos, end, next;
  unsigned long long win;  // the bits from pos on, `have` of them valid, zero above
  int have;
};
VAMD_DEV void bits_open(BitIn &b, const uint32_t *words, long long nwords, long long bit0, long long bit1) {
  b.words = words, b.nwords = nwords, b.pos = bit0, b.end = bit1;
  const long long w = bit0 >> 5;
  const int sh = (int)(bit0 & 31);
  b.win = (unsigned long long)((w >= 0 && w < nwords ? words[w] : 0u) >> sh);
  b.have = 32 - sh;
  b.next = w + 1;
}
// the next k <= 32 bits, zero where the packet has ended
VAMD_DEV unsigned bits_peek(BitIn &b, int k) {
  if (b.have < 32) {
    const unsigned u = b.next >= 0 && b.next < b.nwords ? b.words[b.next] : 0u;
    b.win |= (unsigned long long)u << b.have;
    b.have += 32;
    b.next++;
  }
  const long long left = b.end - b.pos;
  const int keep = left < (long long)k ? (int)left : k;
  if (keep <= 0) return 0u;
  const unsigned v = (unsigned)b.win;
  return keep < 32 ? v & ((1u << keep) - 1u) : v;
}
VAMD_DEV void bits_adv(BitIn &b, int k) {  // after a bits_peek: have >= 32 >= k
  b.win >>= k;
  b.have -= k;
  b.pos += k;
}
// oggpack_read of k <= 32 bits: false where the packet ends first
VAMD_DEV bool bits_read(BitIn &b, int k, unsigned &v) {
  if (b.end - b.pos < (long long)k) return false;
  v = bits_peek(b, k);
  bits_adv(b, k);
  return true;
}

// vorbis_book_decode: the entry (< the book's entries), or -VAMD_STATUS_* .  A codeword that fits what is left of the
// packet is found whatever follows it (the reference retries with fewer bits, lib/codebook.c:312-318).
VAMD_DEV int unpack_book(const UnpackP &U, int booknum, BitIn &in) {
  if (booknum < 0 || booknum >= U.nbooks) return -VAMD_STATUS_BADCODE;
  const UnpackBook &bk = ((const UnpackBook *)U.tab)[booknum];
  const long long left = in.end - in.pos;
  if (left <= 0) return -VAMD_STATUS_TRUNCATED;
  const unsigned x = bits_peek(in, 32);
  const uint32_t *first = (const uint32_t *)(U.tab + bk.off_first) + 2 * (size_t)(x & ((1u << bk.k) - 1u));
  const uint32_t a = first[0], b = first[1];
  int len = (int)(b & 255u), entry = (int)a;
  if (!len) {
    int lo = (int)a, hi = (int)(b >> 8);
    if (lo < hi) {
      const uint32_t *codes = (const uint32_t *)(U.tab + bk.off_codes);
      const unsigned r = brev32(x);
      for (int it = 0; it < 32 && hi - lo > 1; it++) {  // (the range halves: 32 trips cover any list)
        const int mid = (lo + hi) >> 1;
        if (codes[mid] <= r) lo = mid; else hi = mid;
      }
      const uint32_t info = ((const uint32_t *)(U.tab + bk.off_info))[lo];
      const int l = (int)(info >> 24);
      if (l >= 1 && l <= 32 && ((r ^ codes[lo]) >> (32 - l)) == 0u) len = l, entry = (int)(info & 0xffffffu);
    }
  }
  if (!len) return left < 32 ? -VAMD_STATUS_TRUNCATED : -VAMD_STATUS_BADCODE;
  if ((long long)len > left) return -VAMD_STATUS_TRUNCATED;
  bits_adv(in, len);
  return entry;
}

// render_point, lib/floor1.c:257-272
VAMD_DEV int unpack_render_point(int x0, int x1, int y0, int y1, int x) {
  y0 &= 0x7fff;
  y1 &= 0x7fff;
  const int dy = y1 - y0, adx = x1 - x0, ady = dy < 0 ? -dy : dy;
  const int off = adx > 0 ? ady * (x - x0) / adx : 0;
  return dy < 0 ? y0 - off : y0 + off;
}

// The curve's bytes in increasing x, four to a store.  curve: 4-byte aligned, n a multiple of 4.
struct CurveOut {
  unsigned *w;
  unsigned acc;
  int x, n;
  VAMD_MEM void put(int y) {
    if (x >= n) return;
    acc |= (unsigned)(y & 255) << (8 * (x & 3));
    if ((x & 3) == 3) {
      w[x >> 2] = acc;
      acc = 0;
    }
    x++;
  }
};

// One channel's floor: floor1_inverse1 (the posts out of the packet, unwrapped against their predictions) and the integer
// curve floor1_inverse2 multiplies the residue by, left as the encoder's floor stage leaves its ilogmask -- lines between
// the posts in use at the SETUP's places, flat behind the last.  (Where the range is no power of two -- one line, the 5.1
// LFE floor -- a decoder draws to another place; k_synth redraws that line from curve[0] and curve[range]: SynthFloorP.)
//   fit: the lane's [posts] ints, element i at fit[i * fs]
// -> 0 or a status; *valid = the floor's nonzero flag
VAMD_DEV int unpack_floor(const FloorP &F, const vamd_floor1_tab &f, int qbits, const UnpackP &U, BitIn &in, int *fit, int fs,
                          ilog_t *curve, int n2, int *valid) {
  unsigned v;
  *valid = 0;
  if (!bits_read(in, 1, v)) return VAMD_STATUS_TRUNCATED;
  if (!v) return 0;
  const int posts = F.posts < VAMD_POSIT ? F.posts : VAMD_POSIT;
  if (posts < 2) return VAMD_STATUS_NOTAUDIO;
  for (int i = 0; i < 2; i++) {
    if (!bits_read(in, qbits, v)) return VAMD_STATUS_TRUNCATED;
    fit[i * fs] = (int)v;
  }
  const int parts = f.partitions < VAMD_FLOOR_PARTS ? f.partitions : VAMD_FLOOR_PARTS;
  int j = 2;
  for (int i = 0; i < parts; i++) {  // partition by partition (:971-996)
    const int cls = f.partitionclass[i] & (VAMD_FLOOR_CLASSES - 1);
    const int cdim = f.class_dim[cls], csubbits = f.class_subs[cls] & 3, csub = 1 << csubbits;
    int cval = 0;
    if (csubbits) {
      cval = unpack_book(U, f.class_book[cls], in);
      if (cval < 0) return -cval;
    }
    for (int k = 0; k < cdim && j < posts; k++, j++) {
      const int book = f.class_subbook[cls][cval & (csub - 1)];
      cval >>= csubbits;
      int val = 0;
      if (book >= 0) {
        val = unpack_book(U, book, in);
        if (val < 0) return -val;
      }
      fit[j * fs] = val;
    }
  }
  for (; j < posts; j++) fit[j * fs] = 0;  // (a setup whose classes name fewer posts than it has: unpack_check_setup refuses it)
  for (int i = 2; i < posts; i++) {  // unwrap (:999-1033)
    int lo = F.loneighbor[i - 2], hi = F.hineighbor[i - 2];
    lo = lo >= 0 && lo < posts ? lo : 0, hi = hi >= 0 && hi < posts ? hi : 1;  // (neighbours are posts: never)
    const int predicted = unpack_render_point(F.postlist[lo], F.postlist[hi], fit[lo * fs], fit[hi * fs], F.postlist[i]);
    const int hiroom = F.quant_q - predicted, loroom = predicted, room = (hiroom < loroom ? hiroom : loroom) << 1;
    int val = fit[i * fs];
    if (val) {
      if (val >= room) {
        val = hiroom > loroom ? val - loroom : -1 - (val - hiroom);
      } else {
        val = (val & 1) ? -((val + 1) >> 1) : val >> 1;
      }
      fit[i * fs] = (val + predicted) & 0x7fff;
      fit[lo * fs] &= 0x7fff;
      fit[hi * fs] &= 0x7fff;
    } else {
      fit[i * fs] = predicted | 0x8000;
    }
  }
  // the lines (floor1_inverse2 :1050-1075, render_line :347-374)
  auto height = [&](int q) {
    const int y = q * F.mult;
    return y < 0 ? 0 : (y > 255 ? 255 : y);
  };
  CurveOut o;
  o.w = (unsigned *)curve, o.acc = 0, o.x = 0, o.n = n2;
  int lx = 0, ly = height(fit[0] & 0x7fff);
  for (int q = 1; q < posts; q++) {
    const int current = F.forward_index[q] & 127;
    if (current >= posts) continue;
    const int fv = fit[current * fs];
    if (fv & 0x8000) continue;  // an unused post
    const int hx = F.postlist[current], hy = height(fv);
    if (hx <= lx) continue;  // (forward_index sorts distinct places: never)
    const int dy = hy - ly, adx = hx - lx, base = dy / adx, sy = dy < 0 ? base - 1 : base + 1;
    const int ady = (dy < 0 ? -dy : dy) - (base < 0 ? -base : base) * adx;
    const int to = hx < n2 ? hx : n2;
    int y = ly, err = 0;
    for (int x = lx; x < to; x++) {
      if (x > lx) {
        err += ady;
        if (err >= adx) {
          err -= adx;
          y += sy;
        } else {
          y += base;
        }
      }
      o.put(y);
    }
    lx = hx, ly = hy;
  }
  while (o.x < n2) o.put(ly);
  *valid = 1;
  return 0;
}

// One submap's residue: the phrase words into classes, the codewords into entries, in the order they are read -- which
// is the order residue_block leaves them in and synth_residue walks (k_residue.h).
//   coded: bit c = channel c takes part (mapping0_inverse's nonzero[] after the coupling rule)
VAMD_DEV int unpack_residue(const ResP &R, const ChMap &cm, int sm, int ch, unsigned coded, const UnpackP &U, BitIn &in, int *res_class,
                            unsigned short *res_entries, int *res_count) {
  const vamd_residue_tab &t = *R.tab;
  int ns = 0;
  for (int c = 0; c < ch; c++)
    if (cm.sub[c] == sm && ((coded >> c) & 1u)) ns++;
  if (t.type == 2 && ns) ns = 1;  // the bundle interleaved is one stream
  res_count[0] = 0, res_count[1] = 0;
  const int partvals = R.partvals;
  if (!ns || partvals <= 0) return 0;
  const int slots = partvals * ns;
  if (slots > R.slots || slots > VAMD_RES_CLASS_STRIDE) return VAMD_STATUS_NOTAUDIO;  // (never: slots is partvals x the bundle)
  const int ppw = R.groupbook_dim > 0 ? R.groupbook_dim : 1, nparts = R.nparts, spp = t.grouping;
  const int stages = R.nstages < VAMD_RES_MAXSTAGE ? R.nstages : VAMD_RES_MAXSTAGE;
  int words = 1;  // info->partvals: the phrase words that name classes (lib/res0.c:686)
  for (int p = 0; p < ppw && words < (1 << 24); p++) words *= nparts;
  int e = 0;
  for (int s = 0; s < stages; s++)
    for (int i = 0; i < partvals; i += ppw) {
      if (s == 0)
        for (int j = 0; j < ns; j++) {
          int temp = unpack_book(U, R.groupbook, in);
          if (temp < 0) return -temp;
          if (temp >= words) return VAMD_STATUS_BADCODE;
          for (int k = ppw - 1; k >= 0; k--) {  // decodemap (lib/res0.c:226-241): the first partition's class is the highest digit
            const int d = temp / nparts, digit = temp - d * nparts;
            temp = d;
            if (i + k < partvals) res_class[(i + k) * ns + j] = digit;
          }
        }
      for (int k = 0; k < ppw && i + k < partvals; k++)
        for (int j = 0; j < ns; j++) {
          const int c = res_class[(i + k) * ns + j];
          if (c < 0 || c >= nparts || c >= VAMD_RES_MAXCLASS || !((t.secondstages[c] >> s) & 1)) continue;
          const int bn = t.partbooks[c][s];
          if (bn < 0 || bn >= U.nbooks) continue;
          const int dim = R.books[bn].dim, nv = dim > 0 ? spp / dim : 0;
          for (int v = 0; v < nv; v++) {
            const int ent = unpack_book(U, bn, in);
            if (ent < 0) return -ent;
            if (e < R.cap) res_entries[e] = (unsigned short)ent;
            e++;
          }
        }
    }
  res_count[0] = slots, res_count[1] = e < R.cap ? e : R.cap;
  return 0;
}

// One packet -> one block's rows.
//   words / nwords: the buffer the packets lie in; [bit0, bit1): this packet's bits; W: the size class the plan gave it
//   post_valid [ch]; ilogmask [ch][n2] (4-byte aligned); res_class [submaps][VAMD_RES_CLASS_STRIDE]; res_entries [row];
//   res_count [submaps][2]; fit: the lane's [VAMD_POSIT] ints, fs apart
//   stopwatch marks: 0 the head, 1 the floors, 2 the residues
// -> 0, or VAMD_STATUS_* with post_valid and res_count zero
VAMD_DEV int unpack_packet(const Bound &B, const UnpackP &U, const uint32_t *words, long long nwords, long long bit0, long long bit1, int W,
                           int *post_valid, ilog_t *ilogmask, int *res_class, unsigned short *res_entries, int *res_count, int *fit, int fs,
                           PhaseClock &pc) {
  const int ch = B.channels < VAMD_MAX_CH ? B.channels : VAMD_MAX_CH, n2 = B.bs[W] >> 1;
  const ChMap &cm = B.chmap[W];
  BitIn in;
  bits_open(in, words, nwords, bit0, bit1 > bit0 ? bit1 : bit0);
  int status = 0;
  unsigned v = 0, floored = 0;
  // the head (lib/synthesis.c:44-66): packet type, mode number, a long block's neighbours
  if (!bits_read(in, 1, v)) status = VAMD_STATUS_TRUNCATED;
  else if (v) status = VAMD_STATUS_NOTAUDIO;
  if (!status) {
    if (!bits_read(in, U.modebits, v)) status = VAMD_STATUS_TRUNCATED;
    else if ((int)v >= U.modes || (U.modes > 1 ? (int)v : 0) != W) status = VAMD_STATUS_NOTAUDIO;
  }
  if (!status && W && !bits_read(in, 2, v)) status = VAMD_STATUS_TRUNCATED;
  pc.mark(0);
  for (int c = 0; c < ch && !status; c++) {
    const int sm = cm.sub[c] ? 1 : 0;
    int valid = 0;
    status = unpack_floor(B.floor[W][sm], *B.pack[W].ftab[sm], B.pack[W].qbits[sm], U, in, fit, fs, ilogmask + (size_t)c * n2, n2, &valid);
    post_valid[c] = valid;
    floored |= (valid ? 1u : 0u) << c;
  }
  pc.mark(1);
  if (!status) {
    unsigned coded = floored;  // lib/mapping0.c:715-733
    const CoupleP &C = B.couple[W];
    for (int i = 0; i < VAMD_MAX_COUPLING; i++)
      if (i < C.coupling_steps && (((coded >> C.mag[i]) | (coded >> C.ang[i])) & 1u)) coded |= (1u << C.mag[i]) | (1u << C.ang[i]);
    for (int sm = 0; sm < cm.submaps && sm < VAMD_MAX_SUBMAPS && !status; sm++) {
      const ResP &R = B.res[W][sm];
      status = unpack_residue(R, cm, sm, ch, coded, U, in, res_class + R.cls_base, res_entries + R.ent_base, res_count + 2 * sm);
    }
  }
  if (status) {
    for (int c = 0; c < ch; c++) post_valid[c] = 0;
    for (int sm = 0; sm < cm.submaps && sm < VAMD_MAX_SUBMAPS; sm++) res_count[2 * sm] = 0, res_count[2 * sm + 1] = 0;
  }
  pc.mark(2);
  return status;
}

}  // namespace vamd
