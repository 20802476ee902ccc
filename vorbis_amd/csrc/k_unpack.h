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
// nothing (post_valid and res_count zero) -- or, under the keep policy below, with the rows of what was read and class 0 in
// every slot that was not: never in an access outside the rows, never in a loop without an end, under either policy.
//
// TRUNCATED PACKETS -- two policies, the context's choice (vamd_decode_partial, include/vorbis_amd.h).  libvorbis treats a
// packet that ends early as "stop working": a floor that meets the end is no floor, a residue that meets it keeps what it
// has (eopbreak, lib/res0.c:650,709-710), and vorbis_synthesis returns 0.
//   The default (unpack_packet): such a packet carries VAMD_STATUS_TRUNCATED and its stream yields no frames, as a decoded
//   feed's stream with a missing packet does.  A bitrate-managed feed's CUT packets (lib/bitrate.c trims a packet to the
//   byte count the reservoir allows) are truncated packets in this sense.
//   The keep policy (unpack_packet_partial, the same walk's second instantiation): the packet decodes to what libvorbis
//   leaves in vb->pcm for it, and carries VAMD_STATUS_PARTIAL, which costs its stream nothing.  The reference's rules,
//   restated:
//     the reader   a read or advance past the packet's end leaves nothing to read: every later read fails (oggpack_read,
//                  and decode_packed_entry_number's advance over what is left, lib/codebook.c:336-369) -- bits_poison;
//     a floor      the flag bit that fails, or a codeword that does, is no floor for that channel (floor1_inverse1's eop);
//                  the two end posts are read UNCHECKED (lib/floor1.c:967-968): a read that fails leaves -1 there, and
//                  a floor with no codeword behind them -- two posts, the 5.1 LFE's -- is a floor all the same, flat at
//                  the first post's height (0 where that is the -1).  The next channel reads on where the reader stands;
//     a residue    a phrase word or an entry that fails ends its SUBMAP (eopbreak), and so do a phrase word beyond the
//                  classes and a phrase book without used entries, which leave the reader as it is.  Every vector added
//                  before stays: res_count = {slots, entries read}, and the bounded synthesis (k_synth.h) adds exactly
//                  those.  Slots never reached hold class 0.  The next submap reads on where the reader stands.
//   Fatal under both: what vorbis_synthesis refuses (the type bit, a mode that is none or not the plan's, an empty
//   packet, a head that does not complete: lib/synthesis.c:44-66) -- a caller of libvorbis skips such a packet, which
//   takes per-packet granule positions to lap and count as it does, and is not done here.  And what no complete book
//   can give: a residue value book without used entries (VAMD_STATUS_BADCODE) -- a limit of header-made setups, which may
//   hold such a book: libvorbis adds nothing for it and reads on, and its vectors have no numbers in the rows.
#pragma once
#include "vamd_wave.h"
#include "vamd_params.h"
#include "vamd_bind.h"

// per-packet status bits beside VAMD_STATUS_RANGE / _NONFINITE (include/vorbis_amd.h holds the same values)
#define VAMD_STATUS_NOTAUDIO 4    // the packet-type bit is set, the mode number names no mode, or its size class is not the plan's
#define VAMD_STATUS_BADCODE 8     // bits that are no codeword of the book they are read with, or a phrase word beyond the classes
#define VAMD_STATUS_TRUNCATED 16  // the packet ends before the block is complete
#define VAMD_STATUS_PARTIAL 128   // (the keep policy, informative) the packet stopped being read early and decoded as libvorbis decodes it

// Packets a wave of k_unpack (vamd_kernels.h), the rest of its lanes idle.  Measured (profiles/r22_decode.txt).
#define VAMD_UNPACK_LANES 64

namespace vamd {

// One codebook's decode tables inside the table image (unpack_build_tables, vamd_decode_plan.h): the first level answers the
// next `k` bits of the stream -- {entry, length} for a codeword of at most k bits, else the range [lo, hi) of the list
// of longer codewords that begin with those bits.  The list is sorted by the codeword read most significant bit first
// (bit-reversed as the stream holds it, left aligned in 32 bits): the codeword that matches is the last one not above
// the next 32 bits of the stream, read the same way.
struct UnpackBook {
  int32_t entries, k, nsorted, used;  // used: the entries that have a codeword (0: vorbis_book_decode gives -1 and reads nothing)
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

// the keep policy's reader: once a read has failed nothing is left, whatever a later read asks for
VAMD_DEV void bits_poison(BitIn &b) { b.end = b.pos; }
template <bool PARTIAL>
VAMD_DEV bool bits_take(BitIn &b, int k, unsigned &v) {
  if constexpr (!PARTIAL) return bits_read(b, k, v);
  if (bits_read(b, k, v)) return true;
  bits_poison(b);
  return false;
}

// Where a walk under the keep policy stopped, for the one-lane test program (tests/c/unpack_partial_host.cpp), which
// holds its cases to having met every one of them; the kernels pass UnpackNoNote, which is nothing.
enum { UNPACK_AT_FLAG = 1, UNPACK_AT_POST, UNPACK_AT_FLOORBOOK, UNPACK_AT_PHRASE, UNPACK_AT_CLASSES, UNPACK_AT_ENTRY };
struct UnpackNoNote {
  VAMD_MEM void stop(int, int, int) {}  // (place, channel or submap, stage)
  VAMD_MEM void entry(int, long long) {}  // (submap, the reader's place behind an entry that was read)
};

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

// vorbis_book_decode under either policy.  PARTIAL: -VAMD_STATUS_PARTIAL where libvorbis gives -1 -- the packet ends
// inside the codeword (the reader is left with nothing) or the book has no used entries (the reader is left alone)
template <bool PARTIAL>
VAMD_DEV int unpack_code(const UnpackP &U, int booknum, BitIn &in) {
  if constexpr (!PARTIAL) return unpack_book(U, booknum, in);
  if (booknum >= 0 && booknum < U.nbooks && !((const UnpackBook *)U.tab)[booknum].used) return -VAMD_STATUS_PARTIAL;
  const int r = unpack_book(U, booknum, in);
  if (r == -VAMD_STATUS_TRUNCATED) {
    bits_poison(in);
    return -VAMD_STATUS_PARTIAL;
  }
  return r;
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
// -> 0 or a status; *valid = the floor's nonzero flag.  PARTIAL (the head of the file): VAMD_STATUS_PARTIAL alone is a
// read that failed -- no floor, or the floor of end posts that were not there; c: the channel, for the note
template <bool PARTIAL, class Note>
VAMD_DEV int unpack_floor(const FloorP &F, const vamd_floor1_tab &f, int qbits, const UnpackP &U, BitIn &in, int *fit, int fs,
                          ilog_t *curve, int n2, int *valid, int c, Note &note) {
  unsigned v;
  int stopped = 0;  // (PARTIAL: VAMD_STATUS_PARTIAL once an end post was not there)
  *valid = 0;
  if (!bits_take<PARTIAL>(in, 1, v)) {
    if constexpr (PARTIAL) {
      note.stop(UNPACK_AT_FLAG, c, 0);
      return VAMD_STATUS_PARTIAL;
    }
    return VAMD_STATUS_TRUNCATED;
  }
  if (!v) return 0;
  const int posts = F.posts < VAMD_POSIT ? F.posts : VAMD_POSIT;
  if (posts < 2) return VAMD_STATUS_NOTAUDIO;
  for (int i = 0; i < 2; i++) {
    if (!bits_take<PARTIAL>(in, qbits, v)) {
      if constexpr (!PARTIAL) return VAMD_STATUS_TRUNCATED;
      if (!stopped) note.stop(UNPACK_AT_POST, c, 0);
      stopped = VAMD_STATUS_PARTIAL;
      v = ~0u;  // (oggpack_read's -1, kept: lib/floor1.c:967-968)
    }
    fit[i * fs] = (int)v;
  }
  const int parts = f.partitions < VAMD_FLOOR_PARTS ? f.partitions : VAMD_FLOOR_PARTS;
  int j = 2;
  for (int i = 0; i < parts; i++) {  // partition by partition (:971-996)
    const int cls = f.partitionclass[i] & (VAMD_FLOOR_CLASSES - 1);
    const int cdim = f.class_dim[cls], csubbits = f.class_subs[cls] & 3, csub = 1 << csubbits;
    int cval = 0;
    if (csubbits) {
      cval = unpack_code<PARTIAL>(U, f.class_book[cls], in);
      if constexpr (PARTIAL) {
        if (cval == -VAMD_STATUS_PARTIAL && !stopped) note.stop(UNPACK_AT_FLOORBOOK, c, 0);
      }
      if (cval < 0) return -cval;
    }
    for (int k = 0; k < cdim && j < posts; k++, j++) {
      const int book = f.class_subbook[cls][cval & (csub - 1)];
      cval >>= csubbits;
      int val = 0;
      if (book >= 0) {
        val = unpack_code<PARTIAL>(U, book, in);
        if constexpr (PARTIAL) {
          if (val == -VAMD_STATUS_PARTIAL && !stopped) note.stop(UNPACK_AT_FLOORBOOK, c, 1);
        }
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
  if constexpr (PARTIAL) ly = fit[0] < 0 ? 0 : ly;  // (the -1 of a failed read times mult, clamped: lib/floor1.c:1055-1057)
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
  if constexpr (PARTIAL) return stopped;
  return 0;
}

// The keep policy's end of a submap: the slots from partition p0 on -- of its phrase word's partitions only the streams from
// j0 on -- were never given a class and get class 0; e entries were read.
VAMD_DEV int unpack_residue_stop(const ResP &R, int partvals, int ns, int ppw, int p0, int j0, int e, int *res_class, int *res_count) {
  for (int p = p0; p < partvals; p++)
    for (int j = p < p0 + ppw ? j0 : 0; j < ns; j++) res_class[p * ns + j] = 0;
  res_count[0] = partvals * ns, res_count[1] = e < R.cap ? e : R.cap;
  return VAMD_STATUS_PARTIAL;
}

// One submap's residue: the phrase words into classes, the codewords into entries, in the order they are read -- which
// is the order residue_block leaves them in and synth_residue walks (k_residue.h).
//   coded: bit c = channel c takes part (mapping0_inverse's nonzero[] after the coupling rule)
// PARTIAL (the head of the file): VAMD_STATUS_PARTIAL is a submap that ended early, with res_count = {slots, the entries
// read} and class 0 in the slots that were never reached.
template <bool PARTIAL, class Note>
VAMD_DEV int unpack_residue(const ResP &R, const ChMap &cm, int sm, int ch, unsigned coded, const UnpackP &U, BitIn &in, int *res_class,
                            unsigned short *res_entries, int *res_count, Note &note) {
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
          int temp = unpack_code<PARTIAL>(U, R.groupbook, in);
          if constexpr (PARTIAL) {
            if (temp == -VAMD_STATUS_PARTIAL || temp >= words) {
              note.stop(temp < 0 ? UNPACK_AT_PHRASE : UNPACK_AT_CLASSES, sm, 0);
              return unpack_residue_stop(R, partvals, ns, ppw, i, j, e, res_class, res_count);
            }
          }
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
            const int ent = unpack_code<PARTIAL>(U, bn, in);
            if constexpr (PARTIAL) {
              if (ent == -VAMD_STATUS_PARTIAL) {
                if (!((const UnpackBook *)U.tab)[bn].used) return VAMD_STATUS_BADCODE;  // (libvorbis adds nothing and reads on: the head of the file)
                note.stop(UNPACK_AT_ENTRY, sm, s);
                return unpack_residue_stop(R, partvals, ns, ppw, s ? partvals : i + ppw, 0, e, res_class, res_count);
              }
            }
            if (ent < 0) return -ent;
            if constexpr (PARTIAL) note.entry(sm, in.pos);
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
// -> 0, or VAMD_STATUS_* with post_valid and res_count zero.  PARTIAL: or VAMD_STATUS_PARTIAL alone, with the rows of what
// was read (the head of the file)
template <bool PARTIAL, class Note>
VAMD_DEV int unpack_walk(const Bound &B, const UnpackP &U, const uint32_t *words, long long nwords, long long bit0, long long bit1, int W,
                           int *post_valid, ilog_t *ilogmask, int *res_class, unsigned short *res_entries, int *res_count, int *fit, int fs,
                           PhaseClock &pc, Note &note) {
  const int ch = B.channels < VAMD_MAX_CH ? B.channels : VAMD_MAX_CH, n2 = B.bs[W] >> 1;
  const ChMap &cm = B.chmap[W];
  BitIn in;
  bits_open(in, words, nwords, bit0, bit1 > bit0 ? bit1 : bit0);
  int status = 0, partial = 0;
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
    status = unpack_floor<PARTIAL>(B.floor[W][sm], *B.pack[W].ftab[sm], B.pack[W].qbits[sm], U, in, fit, fs, ilogmask + (size_t)c * n2, n2, &valid, c, note);
    if constexpr (PARTIAL) partial |= status & VAMD_STATUS_PARTIAL, status &= ~VAMD_STATUS_PARTIAL;
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
      status = unpack_residue<PARTIAL>(R, cm, sm, ch, coded, U, in, res_class + R.cls_base, res_entries + R.ent_base, res_count + 2 * sm, note);
      if constexpr (PARTIAL) partial |= status & VAMD_STATUS_PARTIAL, status &= ~VAMD_STATUS_PARTIAL;
    }
  }
  if (status) {
    for (int c = 0; c < ch; c++) post_valid[c] = 0;
    for (int sm = 0; sm < cm.submaps && sm < VAMD_MAX_SUBMAPS; sm++) res_count[2 * sm] = 0, res_count[2 * sm + 1] = 0;
  }
  pc.mark(2);
  if constexpr (PARTIAL) return status ? status : partial;
  return status;
}
VAMD_DEV int unpack_packet(const Bound &B, const UnpackP &U, const uint32_t *words, long long nwords, long long bit0, long long bit1, int W,
                           int *post_valid, ilog_t *ilogmask, int *res_class, unsigned short *res_entries, int *res_count, int *fit, int fs,
                           PhaseClock &pc) {
  UnpackNoNote note;
  return unpack_walk<false>(B, U, words, nwords, bit0, bit1, W, post_valid, ilogmask, res_class, res_entries, res_count, fit, fs, pc, note);
}
// the keep policy (the head of the file)
template <class Note>
VAMD_DEV int unpack_packet_partial(const Bound &B, const UnpackP &U, const uint32_t *words, long long nwords, long long bit0, long long bit1, int W,
                                   int *post_valid, ilog_t *ilogmask, int *res_class, unsigned short *res_entries, int *res_count, int *fit,
                                   int fs, PhaseClock &pc, Note &note) {
  return unpack_walk<true>(B, U, words, nwords, bit0, bit1, W, post_valid, ilogmask, res_class, res_entries, res_count, fit, fs, pc, note);
}

}  // namespace vamd
