// vamd_headers.h -- a decode-only setup out of a stream's own identification and setup header packets (include/vorbis_amd.h:
// vamd_create_decoder).  Three parts: the packets parsed from the Vorbis I specification's field lists, with the accept /
// reject line of the reference's vorbis_synthesis_headerin (held to it by tests/test_decode_headers_cpu.py); what the decode kernels take for granted of a setup, checked ("Setups in": the list);
// and the image bind_params (vamd_bind.h) binds -- a vamd_setup_header with the decode-side sections filled in and the
// encode-side ones zero, the transform tables as mdct_init computes them, the windows by their rule, the books' lengths and
// codewords -- with the residue books' VALUES beside it, for the books whose values are no centred integer lattice
// (k_synth.h: synth_residue's table form).  Plain C++, no HIP: the library and the one-lane test program
// (tests/c/decode_headers_host.cpp) share it.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "vamd_bind.h"
#include "k_synth.h"
#include "vamd_decode_plan.h"

#ifndef VAMD_ENOTVORBIS  // (include/vorbis_amd.h holds the same values)
#define VAMD_ENOTVORBIS (-132)
#define VAMD_EBADHEADER (-133)
#endif

namespace vamd {

#define VAMD_VALUES_MAX_FLOATS (16u << 20)  // the value lists of a setup's residue books: 64 MiB at most

// oggpack_read over one packet: a read that would pass the packet's end fails, and so does every read after it
struct HeaderBits {
  const uint8_t *p;
  int64_t nbits, pos = 0;
  bool dead = false;
  HeaderBits(const void *data, size_t bytes) : p((const uint8_t *)data), nbits(8 * (int64_t)bytes) {}
  long read(int bits) {
    if (dead || bits < 0 || bits > 32 || pos + bits > nbits) return dead = true, -1;
    uint64_t v = 0;
    for (int k = 0; k < bits; k++, pos++) v |= (uint64_t)((p[pos >> 3] >> (pos & 7)) & 1) << k;
    return (long)v;
  }
  int64_t bytes() const { return dead ? nbits / 8 + 1 : (pos + 7) / 8; }  // oggpack_bytes
  int64_t storage() const { return nbits / 8; }
};

inline int header_ilog(uint32_t v) {
  int r = 0;
  for (; v; v >>= 1) r++;
  return r;
}

// Vorbis I 9.2.2, float32_unpack: 21 bits of mantissa, 10 of exponent biased by 788, a sign; the result is mantissa * 2^exponent.
// (The reference holds the exponent to [-63, 63] before it scales: so does this.)
inline float header_float32(uint32_t x) {
  const double magnitude = (double)(x & 0x1fffffu);
  const int exponent = std::min(63, std::max(-63, (int)((x >> 21) & 0x3ffu) - 788));
  return (float)ldexp((x >> 31) ? -magnitude : magnitude, exponent);
}

// the greatest v with v^dim <= entries (Vorbis I 9.2.3, lookup1_values)
inline long header_lookup1_values(long dim, long entries) {
  if (entries < 1 || dim < 1) return 0;
  long v = (long)floor(pow((double)entries, 1.0 / (double)dim));
  auto pw = [&](long b) {  // b^dim, saturated above entries
    long acc = 1;
    for (long i = 0; i < dim; i++) {
      if (b && acc > entries / b) return entries + 1;
      acc *= b;
    }
    return acc;
  };
  if (v < 1) v = 1;
  while (pw(v) > entries) v--;
  while (pw(v + 1) <= entries) v++;
  return v;
}

struct HeaderBook {
  int dim = 0, entries = 0, maptype = 0, q_quant = 0, q_sequencep = 0;
  uint32_t q_min = 0, q_delta = 0;
  std::vector<signed char> len;  // [entries], 0: unused
  std::vector<uint16_t> quant;
};
struct HeaderFloor {
  int type = 1;
  vamd_floor1_tab t;  // posts, postlist, mult, partition and class tables (type 1)
};
struct HeaderResidue {
  int type = 0, begin = 0, end = 0, grouping = 0, partitions = 0, groupbook = 0;
  int secondstages[VAMD_RES_MAXCLASS];
  int partbooks[VAMD_RES_MAXCLASS][VAMD_RES_MAXSTAGE];
};
struct HeaderMapping {
  int submaps = 1, coupling_steps = 0;
  int mag[256], ang[256], chmux[256], floor[16], residue[16];
};
struct HeaderMode {
  int blockflag, mapping;
};
struct HeaderSetup {
  int channels = 0, bs[2] = {0, 0};
  int64_t rate = 0;
  std::vector<HeaderBook> books;
  std::vector<HeaderFloor> floors;
  std::vector<HeaderResidue> residues;
  std::vector<HeaderMapping> maps;
  std::vector<HeaderMode> modes;
};

// the packet type and "vorbis" (vorbis_synthesis_headerin, lib/info.c:394-402)
inline int header_open(HeaderBits &in, int want_type) {
  const long type = in.read(8);
  char name[6];
  for (char &ch : name) ch = (char)in.read(8);
  if (memcmp(name, "vorbis", 6) != 0) return VAMD_ENOTVORBIS;
  return type == want_type ? VAMD_OK : VAMD_EBADHEADER;  // (the other types are headers out of their order)
}

// the identification header (_vorbis_unpack_info)
inline int header_parse_ident(const void *data, size_t bytes, HeaderSetup *S) {
  HeaderBits in(data, bytes);
  int r = header_open(in, 1);
  if (r) return r;
  if ((int)in.read(32) != 0) return VAMD_EVERSION;
  const long channels = in.read(8), rate = in.read(32);
  in.read(32), in.read(32), in.read(32);
  const long b0 = in.read(4), b1 = in.read(4);
  if (b0 < 0 || b1 < 0 || rate < 1 || channels < 1) return VAMD_EBADHEADER;
  if ((1 << b0) < 64 || (1 << b1) < (1 << b0) || (1 << b1) > 8192) return VAMD_EBADHEADER;
  if (in.read(1) != 1) return VAMD_EBADHEADER;
  S->channels = (int)channels, S->rate = rate, S->bs[0] = 1 << b0, S->bs[1] = 1 << b1;
  return VAMD_OK;
}

// The unpackers below follow the Vorbis I specification's field lists (3.2.1 codebooks, 7.2.2 floor 1, 6.2.1 floor 0, 8.6.1
// residues, 4.2.4 the setup header) under the specification's names.  A read that fails leaves the reader dead, every later
// read fails too, and a section that ends with a dead reader is refused; beside that each section refuses what the reference
// decoder is observed to refuse (the conditions are named where they are tested).  -> false: refused.

// the bytes a field of `bits` bits needs, against the whole bytes the packet has left behind the byte being read: the
// reference asks this of a codebook's length list and value list before it reads them, so a list that would only just fit
// into the bits left of the current byte is refused
inline bool header_room(const HeaderBits &in, int64_t bits) { return (bits + 7) / 8 <= in.storage() - in.bytes(); }

// 3.2.1, the codeword lengths: entry by entry (with a flag per entry where the book is sparse), or run by run in order of
// length.  An ordered book is refused where a run is longer than what is left, where a length passes 32, and where a run
// of codewords of one length is more than twice what that length can hold.
inline bool header_book_lengths(HeaderBits &in, HeaderBook *c) {
  const int entries = c->entries;
  const long ordered = in.read(1);
  if (in.dead) return false;
  if (!ordered) {
    const bool sparse = in.read(1) != 0;
    if (!header_room(in, (int64_t)entries * (sparse ? 1 : 5))) return false;
    c->len.assign((size_t)entries, 0);
    for (signed char &length : c->len)
      if (!sparse || in.read(1) != 0) length = (signed char)(in.read(5) + 1);
    return !in.dead;
  }
  int current_entry = 0;
  long current_length = in.read(5) + 1;
  if (in.dead) return false;
  c->len.assign((size_t)entries, 0);
  for (; current_entry < entries; current_length++) {
    const int left = entries - current_entry;
    const long number = in.read(header_ilog((uint32_t)left));
    if (in.dead || current_length > 32 || number > left) return false;
    if (number > 0 && ((number - 1) >> (current_length - 1)) > 1) return false;
    std::fill_n(c->len.begin() + current_entry, (size_t)number, (signed char)current_length);
    current_entry += (int)number;
  }
  return true;
}

// 3.2.1, the vector lookup: none (type 0), or a minimum, a delta, the width of a multiplicand, the sequence flag and the
// multiplicands -- lookup1_values of them (type 1) or one per scalar of every entry (type 2)
inline bool header_book_lookup(HeaderBits &in, HeaderBook *c) {
  const long lookup_type = in.read(4);
  if (in.dead || lookup_type > 2) return false;
  c->maptype = (int)lookup_type;
  if (lookup_type == 0) return true;
  c->q_min = (uint32_t)in.read(32);
  c->q_delta = (uint32_t)in.read(32);
  c->q_quant = (int)in.read(4) + 1;
  c->q_sequencep = (int)in.read(1);
  if (in.dead) return false;
  const int64_t lookup_values = lookup_type == 1 ? header_lookup1_values(c->dim, c->entries) : (int64_t)c->entries * c->dim;
  if (!header_room(in, lookup_values * c->q_quant)) return false;
  c->quant.resize((size_t)lookup_values);
  for (uint16_t &multiplicand : c->quant) multiplicand = (uint16_t)in.read(c->q_quant);
  return !in.dead;
}

// 3.2.1: the sync pattern "BCV", 16 bits of dimensions, 24 of entries, the lengths, the lookup.  The reference keeps the
// dimension in eight signed bits and refuses a book whose dimension and entry count need more than 24 bits together
// (a dimension it reads as negative needs 32).
inline bool header_parse_book(HeaderBits &in, HeaderBook *c) {
  static const unsigned char sync[3] = {'B', 'C', 'V'};
  for (unsigned char ch : sync)
    if (in.read(8) != ch) return false;
  const long dimensions = in.read(16), entries = in.read(24);
  if (in.dead) return false;
  c->dim = (int)(int8_t)(uint8_t)(dimensions & 0xff);
  c->entries = (int)entries;
  if (header_ilog((uint32_t)c->dim) + header_ilog((uint32_t)c->entries) > 24) return false;
  return header_book_lengths(in, c) && header_book_lookup(in, c);
}

// 6.2.1, floor 0 (read to hold the accept / reject line; the setup is then refused as outside the covered shape): order,
// rate and bark map size at least 1, and books that exist, have a value mapping and a dimension
inline bool header_parse_floor0(HeaderBits &in, const HeaderSetup &S) {
  const long floor0_order = in.read(8), floor0_rate = in.read(16), floor0_bark_map_size = in.read(16);
  in.read(6), in.read(8);  // amplitude bits, amplitude offset
  const long floor0_number_of_books = in.read(4) + 1;
  if (in.dead || floor0_order < 1 || floor0_rate < 1 || floor0_bark_map_size < 1) return false;
  for (long k = 0; k < floor0_number_of_books; k++) {
    const long book = in.read(8);
    if (in.dead || book >= (long)S.books.size()) return false;
    if (S.books[(size_t)book].maptype == 0 || S.books[(size_t)book].dim < 1) return false;
  }
  return true;
}

// 7.2.2, floor 1: the partition class list; per class up to the highest in use its dimensions, sub-class bits, master book
// (with sub-classes) and sub-class books (one less than written: 0 is "none"); the multiplier, the range bits and the X
// list.  Refused: a book that does not exist, more than 63 posts beside the two end posts, two posts at one place.
inline bool header_parse_floor1(HeaderBits &in, const HeaderSetup &S, vamd_floor1_tab *f) {
  const int nbooks = (int)S.books.size();
  memset(f, 0, sizeof(*f));
  const long floor1_partitions = in.read(5);
  if (in.dead) return false;
  f->partitions = (int)floor1_partitions;
  int maximum_class = -1;
  for (int p = 0; p < f->partitions; p++) maximum_class = std::max(maximum_class, f->partitionclass[p] = (int)in.read(4));
  if (in.dead) return false;
  for (int c = 0; c <= maximum_class; c++) {
    f->class_dim[c] = (int)in.read(3) + 1;
    f->class_subs[c] = (int)in.read(2);
    if (in.dead) return false;
    if (f->class_subs[c]) f->class_book[c] = (int)in.read(8);
    if (in.dead || f->class_book[c] >= nbooks) return false;
    for (int k = 0; k < (1 << f->class_subs[c]); k++)
      if ((f->class_subbook[c][k] = (int)in.read(8) - 1) >= nbooks || in.dead) return false;
  }
  f->mult = (int)in.read(2) + 1;
  const long rangebits = in.read(4);
  if (in.dead) return false;
  f->posts = 2;
  for (int p = 0; p < f->partitions; p++) f->posts += f->class_dim[f->partitionclass[p]];
  if (f->posts > VAMD_POSIT) return false;
  f->postlist[0] = 0, f->postlist[1] = 1 << rangebits;
  for (int k = 2; k < f->posts; k++) f->postlist[k] = (int)in.read((int)rangebits);
  if (in.dead) return false;
  std::vector<int> places(f->postlist, f->postlist + f->posts);
  std::sort(places.begin(), places.end());
  return std::adjacent_find(places.begin(), places.end()) == places.end();
}

// 8.6.1, a residue of any of the three types: begin, end, partition size - 1, classifications - 1, the class book; per
// class a cascade of eight stage bits (three low, five high behind a flag); a book per set bit.  Refused: a book that does
// not exist, a stage book without a value mapping, a class book without a dimension or with fewer entries than there are
// tuples of classes.
inline bool header_parse_residue(HeaderBits &in, const HeaderSetup &S, HeaderResidue *r) {
  const int nbooks = (int)S.books.size();
  r->begin = (int)in.read(24), r->end = (int)in.read(24), r->grouping = (int)in.read(24) + 1;
  r->partitions = (int)in.read(6) + 1, r->groupbook = (int)in.read(8);
  if (in.dead || r->groupbook >= nbooks) return false;
  for (int c = 0; c < r->partitions; c++) {
    const long low_bits = in.read(3);
    const long high_bits = in.read(1) ? in.read(5) : 0;
    if (in.dead) return false;
    r->secondstages[c] = (int)(high_bits * 8 + low_bits);
  }
  for (int c = 0; c < r->partitions; c++)
    for (int stage = 0; stage < VAMD_RES_MAXSTAGE; stage++) {
      r->partbooks[c][stage] = -1;
      if (!((r->secondstages[c] >> stage) & 1)) continue;
      const long book = in.read(8);
      if (in.dead) return false;
      r->partbooks[c][stage] = (int)book;
    }
  for (int c = 0; c < r->partitions; c++)
    for (int book : r->partbooks[c])
      if (book >= nbooks || (book >= 0 && S.books[(size_t)book].maptype == 0)) return false;
  const HeaderBook &classbook = S.books[(size_t)r->groupbook];
  if (classbook.dim < 1) return false;
  int64_t tuples = 1;
  for (int d = 0; d < classbook.dim && tuples <= classbook.entries; d++) tuples *= r->partitions;
  return tuples <= classbook.entries;
}

// 4.2.4, step 5, a mapping of type 0: the submap count behind a flag, the coupling steps behind a flag (magnitude and angle
// in ilog(channels - 1) bits: two different channels that exist), two reserved bits that are zero, the channels' submaps
// where there is more than one, and per submap a byte that is not used, its floor and its residue, which exist
inline bool header_parse_mapping(HeaderBits &in, const HeaderSetup &S, HeaderMapping *m) {
  memset(m, 0, sizeof(*m));
  m->submaps = in.read(1) ? (int)in.read(4) + 1 : 1;
  if (in.dead) return false;
  if (in.read(1)) {
    m->coupling_steps = (int)in.read(8) + 1;
    const int field = header_ilog((uint32_t)(S.channels - 1));
    for (int step = 0; step < m->coupling_steps && !in.dead; step++) {
      const long magnitude = in.read(field), angle = in.read(field);
      if (in.dead || magnitude == angle || magnitude >= S.channels || angle >= S.channels) return false;
      m->mag[step] = (int)magnitude, m->ang[step] = (int)angle;
    }
  }
  if (in.read(2) != 0) return false;
  for (int c = 0; c < S.channels && m->submaps > 1; c++)
    if ((m->chmux[c] = (int)in.read(4)) >= m->submaps || in.dead) return false;
  for (int sm = 0; sm < m->submaps; sm++) {
    in.read(8);
    m->floor[sm] = (int)in.read(8), m->residue[sm] = (int)in.read(8);
    if (in.dead || m->floor[sm] >= (int)S.floors.size() || m->residue[sm] >= (int)S.residues.size()) return false;
  }
  return true;
}

// 4.2.4, the setup header: the codebooks; the time domain placeholders (zero); the floors (type 0 or 1); the residues (type
// 0, 1 or 2); the mappings (type 0); the modes (block flag; window and transform type zero; a mapping that exists); the
// framing bit.  S holds the identification header's fields.  Each count is one more than written.
inline int header_parse_setup(const void *data, size_t bytes, HeaderSetup *S) {
  HeaderBits in(data, bytes);
  const int r = header_open(in, 5);
  if (r) return r;
  auto count = [&](int bits) { return (size_t)(in.read(bits) + 1); };  // (a dead reader counts none)
  S->books.resize(count(8));
  for (HeaderBook &b : S->books)
    if (!header_parse_book(in, &b)) return VAMD_EBADHEADER;
  for (size_t k = count(6); k > 0; k--)
    if (in.read(16) != 0) return VAMD_EBADHEADER;
  S->floors.resize(count(6));
  for (HeaderFloor &f : S->floors) {
    f.type = (int)in.read(16);
    const bool ok = f.type == 0 ? header_parse_floor0(in, *S) : f.type == 1 && header_parse_floor1(in, *S, &f.t);
    if (!ok) return VAMD_EBADHEADER;
  }
  S->residues.resize(count(6));
  for (HeaderResidue &x : S->residues) {
    x.type = (int)in.read(16);
    if (in.dead || x.type > 2 || !header_parse_residue(in, *S, &x)) return VAMD_EBADHEADER;
  }
  S->maps.resize(count(6));
  for (HeaderMapping &m : S->maps)
    if (in.read(16) != 0 || !header_parse_mapping(in, *S, &m)) return VAMD_EBADHEADER;
  S->modes.resize(count(6));
  for (HeaderMode &m : S->modes) {
    m.blockflag = (int)in.read(1);
    const long windowtype = in.read(16), transformtype = in.read(16);
    m.mapping = (int)in.read(8);
    if (in.dead || windowtype != 0 || transformtype != 0 || m.mapping >= (int)S->maps.size()) return VAMD_EBADHEADER;
  }
  if (S->books.empty() || S->floors.empty() || S->residues.empty() || S->maps.empty() || S->modes.empty()) return VAMD_EBADHEADER;
  return in.read(1) == 1 ? VAMD_OK : VAMD_EBADHEADER;
}

// ---- the tables of a block size ----
// The inverse MDCT's tables for a block of n samples, in the layout mdct_backward_wave reads (XformP::trig, ::bitrev).
//   trig [n + n/4]: three lists of n/4, n/4 and n/8 unit vectors (cos, sin) -- the rotation by multiples of 4 pi / n, clockwise;
//                   the odd multiples of pi / 2n, counter-clockwise; the odd multiples of 2 pi / n, clockwise and halved.
//   bitrev [n/4]:   per i < n/8 the pair (complement of r, less one; r), r = i's log2(n) - 1 bits in reverse order.
// The angles are formed as (pi / n) * k resp. (pi / 2n) * k in double and the results stored as floats: the decoder's output
// depends on every bit of them, and this is the arithmetic whose bits equal the reference's tables (the image test).
inline void header_mdct_tables(int n, std::vector<float> *trig, std::vector<int32_t> *bitrev) {
  const int quarter = n / 4, eighth = n / 8, bits = header_ilog((uint32_t)n) - 2;  // bits = log2(n) - 1
  const double step = M_PI / n, half_step = M_PI / (2 * n);
  trig->clear();
  auto unit = [&](double angle, double turn, double scale) {
    trig->push_back((float)(cos(angle) * scale));
    trig->push_back((float)(turn * sin(angle) * scale));
  };
  for (int i = 0; i < quarter; i++) unit(step * (4 * i), -1., 1.);
  for (int i = 0; i < quarter; i++) unit(half_step * (2 * i + 1), 1., 1.);
  for (int i = 0; i < eighth; i++) unit(step * (4 * i + 2), -1., .5);
  bitrev->clear();
  for (int i = 0; i < eighth; i++) {
    int r = 0;
    for (int b = 0; b < bits; b++) r |= ((i >> b) & 1) << (bits - 1 - b);
    bitrev->push_back((~r & ((1 << bits) - 1)) - 1);
    bitrev->push_back(r);
  }
}

// The rising half of the Vorbis window of a block of n samples, [n/2], as lib/window.c holds it: the tables there are
// sin(pi/2 sin^2((i + 1/2) pi / n)) PRINTED WITH TEN DECIMALS, so the value is the double's "%.10f" text read as a float
// ("Setups in").
inline void header_window(int n, std::vector<float> *win) {
  win->assign((size_t)(n / 2), 0.f);
  for (int i = 0; i < n / 2; i++) {
    const double s = sin((i + .5) / n * M_PI);
    char text[40];
    snprintf(text, sizeof(text), "%.10f", sin(M_PI / 2. * s * s));
    (*win)[(size_t)i] = strtof(text, nullptr);
  }
}

// Vorbis I 3.2.1, the Huffman decision tree: entries take, in order, the lowest-valued codeword of their length that is still
// free -- codewords compared as the stream's bits in reading order.  Kept here as the list of free subtrees (a prefix and
// its depth; never two of one depth, so at most 33): an entry of length L takes the leftmost leaf of depth L under the free
// subtree of the lowest prefix among those no deeper than L, and the right-hand siblings along that path become free.
// -> the codewords as the stream holds them (least significant bit first); false for an over-populated tree (no subtree left
// for an entry) or an under-populated one (subtrees left at the end).  Two cases are neither, as the reference decoder has
// it: a book without used entries, and a book whose one used entry has length 1 (*single: that entry is read from one bit
// of either value).
inline bool header_make_words(const std::vector<signed char> &len, std::vector<uint32_t> *codes, bool *single) {
  struct Subtree {
    uint64_t prefix;  // left aligned in 32 bits
    int depth;
  };
  std::vector<Subtree> free_list = {{0u, 0}};
  codes->assign(len.size(), 0u);
  long used = 0;
  int only_length = 0;
  for (size_t e = 0; e < len.size(); e++) {
    const int L = len[e];
    if (L <= 0) continue;
    used++, only_length = L;
    int take = -1;
    for (int k = 0; k < (int)free_list.size(); k++)
      if (free_list[(size_t)k].depth <= L && (take < 0 || free_list[(size_t)k].prefix < free_list[(size_t)take].prefix)) take = k;
    if (take < 0) return false;
    const Subtree t = free_list[(size_t)take];
    free_list.erase(free_list.begin() + take);
    for (int d = t.depth + 1; d <= L; d++) free_list.push_back({t.prefix | (1ull << (32 - d)), d});
    uint32_t word = 0;  // the L bits of the prefix, first bit read = bit 0
    for (int b = 0; b < L; b++) word |= (uint32_t)((t.prefix >> (31 - b)) & 1u) << b;
    (*codes)[e] = word;
  }
  *single = used == 1 && only_length == 1;
  return used == 0 || *single || free_list.empty();
}

// _book_unquantize (lib/sharedbook.c:285-334) by entry number: [entries][dim], unused entries zero
inline void header_book_values(const HeaderBook &b, std::vector<float> *out) {
  out->assign((size_t)b.entries * b.dim, 0.f);
  const float mindel = header_float32(b.q_min), delta = header_float32(b.q_delta);
  const long qv = b.maptype == 1 ? header_lookup1_values(b.dim, b.entries) : 0;
  for (long j = 0; j < b.entries; j++) {
    float last = 0.f;
    long indexdiv = 1;
    for (int k = 0; k < b.dim; k++) {
      const float q = b.maptype == 1 ? (float)b.quant[(size_t)((j / indexdiv) % qv)] : (float)b.quant[(size_t)(j * b.dim + k)];
      const float val = (float)(fabs((double)q) * (double)delta + (double)mindel + (double)last);
      if (b.q_sequencep) last = val;
      (*out)[(size_t)(j * b.dim + k)] = val;
      indexdiv *= qv;
    }
  }
}

// what vorbis_book_init_encode makes of a book's value mapping (lib/sharedbook.c:364-377): the lattice's integers
inline void header_book_lattice(const HeaderBook &b, vamd_book_tab *t) {
  const float mn = header_float32(b.q_min), dl = header_float32(b.q_delta);
  t->quantvals = (int32_t)header_lookup1_values(b.dim, b.entries);
  t->minval = fabsf(mn) < 1e9f ? (int32_t)rint(mn) : 0;
  t->delta = fabsf(dl) < 1e9f ? (int32_t)rint(dl) : 0;
}

// Is the book a lattice book -- does synth_lattice_value give the reference's value, bit for bit, for every digit?
inline bool header_book_is_lattice(const HeaderBook &b, const vamd_book_tab &t) {
  if (b.maptype != 1 || b.q_sequencep || t.quantvals < 1 || (size_t)t.quantvals != b.quant.size()) return false;
  const float mindel = header_float32(b.q_min), delta = header_float32(b.q_delta);
  const int ze = t.quantvals >> 1;
  for (int d = 0; d < t.quantvals; d++) {
    const int64_t v = (d & 1) ? ze - ((d + 1) >> 1) : ze + (d >> 1), wide = v * t.delta + t.minval;
    if (wide < INT32_MIN || wide > INT32_MAX) return false;
    const float ref = (float)(fabs((double)(float)b.quant[(size_t)d]) * (double)delta + (double)mindel + 0.);
    const float got = synth_lattice_value(d, ze, t.delta, t.minval);
    if (memcmp(&ref, &got, 4) != 0) return false;
  }
  return true;
}

// What a decode-only context holds beside its image: the residue books' value lists (ValueP, k_synth.h)
struct HeaderImage {
  std::vector<unsigned char> image;
  std::vector<uint32_t> derived_off;   // bind_params' encode-side slots: all at the image's start, none read by a decode kernel
  std::vector<PsyDerived> derived;
  std::vector<int32_t> value_off;      // [nbooks] where the book's [entries][dim] floats begin in `values`; -1: a lattice book, or no residue book
  std::vector<float> values;
  int table_books = 0, lattice_books = 0;  // the residue books of either kind
};

inline int header_refuse(std::string *err, const std::string &what) {
  *err = "headers: " + what;
  return VAMD_EIMPL;
}

// The parsed setup -> the image, or VAMD_EIMPL with the first thing outside the covered shape.
inline int header_build_image(const HeaderSetup &S, HeaderImage *out, std::string *err) {
  auto num = [](long v) { return std::to_string(v); };
  if (S.channels > VAMD_MAX_CH) return header_refuse(err, num(S.channels) + " channels (at most " + num(VAMD_MAX_CH) + ")");
  if (S.rate > 0x7fffffff) return header_refuse(err, "a sample rate above 2^31 - 1");
  if (S.bs[1] > 4096) return header_refuse(err, "block size " + num(S.bs[1]) + " (block sizes above 4096 are not covered)");
  for (const HeaderFloor &f : S.floors)
    if (f.type != 1) return header_refuse(err, "floor type 0");
  for (const HeaderResidue &r : S.residues)
    if (r.type == 0) return header_refuse(err, "residue type 0");
  const int modes = (int)S.modes.size();
  if (modes > 2) return header_refuse(err, num(modes) + " modes (one, or two with mode i of block flag i)");
  for (int i = 0; i < modes; i++)
    if (S.modes[(size_t)i].blockflag != i) return header_refuse(err, "mode " + num(i) + " has block flag " + num(S.modes[(size_t)i].blockflag) + " (one mode, or two with mode i of block flag i)");
  const int nbooks = (int)S.books.size();
  if (nbooks > 255) return header_refuse(err, "256 codebooks (at most 255)");

  vamd_setup_header h;
  memset(&h, 0, sizeof(h));
  h.magic = VAMD_SETUP_MAGIC, h.version = VAMD_SETUP_VERSION;
  h.channels = S.channels, h.rate = (int32_t)S.rate, h.blocksizes[0] = S.bs[0], h.blocksizes[1] = S.bs[1];
  h.modes = modes, h.modebits = header_ilog((uint32_t)(modes - 1));
  std::vector<unsigned char> &im = out->image;
  im.assign(sizeof(h), 0);
  auto place = [&](const void *src, size_t bytes) {
    while (im.size() & 15) im.push_back(0);
    const uint32_t at = (uint32_t)im.size();
    im.insert(im.end(), (const unsigned char *)src, (const unsigned char *)src + bytes);
    return at;
  };
  for (int W = 0; W < 2; W++) {
    vamd_xform_tab &x = h.xform[W];
    const int n = S.bs[W];
    std::vector<float> trig, win;
    std::vector<int32_t> bitrev;
    header_mdct_tables(n, &trig, &bitrev);
    header_window(n, &win);
    x.n = n, x.log2n = header_ilog((uint32_t)n) - 1, x.mdct_scale = 4.f / n;
    x.off_mdct_trig = place(trig.data(), 4 * trig.size());
    x.off_mdct_bitrev = place(bitrev.data(), 4 * bitrev.size());
    x.off_window = place(win.data(), 4 * win.size());
  }
  // the modes: W's mode is mode W, or the only one (as the blob's packer fills both slots of a one-mode setup)
  std::vector<char> is_residue_book((size_t)nbooks, 0);
  for (int W = 0; W < 2; W++) {
    const HeaderMapping &mp = S.maps[(size_t)S.modes[(size_t)(W < modes ? W : 0)].mapping];
    vamd_mode_tab &m = h.mode[W];
    const int n2 = S.bs[W] / 2;
    if (mp.submaps > VAMD_MAX_SUBMAPS) return header_refuse(err, num(mp.submaps) + " submaps (at most " + num(VAMD_MAX_SUBMAPS) + ")");
    if (mp.coupling_steps > VAMD_MAX_COUPLING) return header_refuse(err, num(mp.coupling_steps) + " coupling steps (at most " + num(VAMD_MAX_COUPLING) + ")");
    m.submaps = mp.submaps, m.coupling_steps = mp.coupling_steps;
    for (int i = 0; i < mp.coupling_steps; i++) m.coupling_mag[i] = mp.mag[i], m.coupling_ang[i] = mp.ang[i];
    for (int c = 0; c < S.channels; c++) m.chmuxlist[c] = mp.submaps > 1 ? mp.chmux[c] : 0;
    for (int sm = 0; sm < mp.submaps; sm++) {
      int bundle = 0;
      for (int c = 0; c < S.channels; c++) bundle += m.chmuxlist[c] == sm;
      if (!bundle) return header_refuse(err, "a submap without channels");
      // the floor: floor1_look's derived tables (lib/floor1.c:180-255)
      vamd_floor1_tab &f = m.floor[sm];
      f = S.floors[(size_t)mp.floor[sm]].t;
      f.look_n = f.postlist[1];
      if (f.look_n > n2) return header_refuse(err, "a floor whose range (" + num(f.look_n) + ") exceeds half its block (" + num(n2) + ")");
      static const int quant_q[4] = {256, 128, 86, 64};
      f.quant_q = quant_q[f.mult - 1];
      std::vector<int> order((size_t)f.posts);
      for (int i = 0; i < f.posts; i++) order[(size_t)i] = i;
      std::sort(order.begin(), order.end(), [&](int a, int b) { return f.postlist[a] < f.postlist[b]; });  // (no ties: floor1_unpack)
      for (int i = 0; i < f.posts; i++) {
        f.forward_index[i] = order[(size_t)i];
        f.reverse_index[order[(size_t)i]] = i;
        f.sorted_index[i] = f.postlist[order[(size_t)i]];
      }
      for (int i = 0; i < f.posts - 2; i++) {
        int lo = 0, hi = 1, lx = 0, hx = f.look_n;
        const int cur = f.postlist[i + 2];
        for (int j = 0; j < i + 2; j++) {
          const int x = f.postlist[j];
          if (x > lx && x < cur) lo = j, lx = x;
          if (x < hx && x > cur) hi = j, hx = x;
        }
        f.loneighbor[i] = lo, f.hineighbor[i] = hi;
      }
      for (int i = 0; i < f.partitions; i++) {  // every book the floor reads codewords with exists (a class without sub-classes reads none)
        const int c = f.partitionclass[i];
        if (f.class_subs[c] && S.books[(size_t)f.class_book[c]].entries < 1) return header_refuse(err, "a floor class book without entries");
      }
      // the residue, its range held to the block as _01inverse / res2_inverse hold it (lib/res0.c:655-658,820-822)
      const HeaderResidue &r = S.residues[(size_t)mp.residue[sm]];
      vamd_residue_tab &t = h.res[W][sm];
      const int span = r.type == 2 ? n2 * bundle : n2;
      t.type = r.type, t.begin = r.begin, t.end = std::min(r.end, span), t.grouping = r.grouping, t.partitions = r.partitions;
      t.groupbook = r.groupbook, t.groupbook_dim = S.books[(size_t)r.groupbook].dim;
      if (t.end - t.begin < t.grouping) return header_refuse(err, "a residue that codes no partition of its block");
      if (t.groupbook_dim > 16) return header_refuse(err, "a phrase book of dimension " + num(t.groupbook_dim) + " (at most 16)");
      if (r.type == 2 && (t.begin % bundle || t.grouping % bundle))
        return header_refuse(err, "a type 2 residue whose begin or partition size is no multiple of its " + num(bundle) + " channels");
      const int partvals = (t.end - t.begin) / t.grouping;
      if ((int64_t)partvals * (r.type == 2 ? 1 : bundle) > VAMD_RES_CLASS_STRIDE)
        return header_refuse(err, "a residue of more than " + num(VAMD_RES_CLASS_STRIDE) + " partitions a block");
      for (int c = 0; c < r.partitions; c++) {
        t.secondstages[c] = r.secondstages[c];
        for (int s = 0; s < VAMD_RES_MAXSTAGE; s++) {
          const int bn = t.partbooks[c][s] = r.partbooks[c][s];
          if (bn < 0) continue;
          t.stages = std::max(t.stages, s + 1);
          const HeaderBook &b = S.books[(size_t)bn];
          if (b.dim < 1 || b.dim > 8 || r.grouping % b.dim) return header_refuse(err, "residue book " + num(bn) + ": dimension " + num(b.dim) + " does not divide the partition size " + num(r.grouping) + ", or is above 8");
          if (b.entries > 65535) return header_refuse(err, "residue book " + num(bn) + ": more than 65 535 entries");
          is_residue_book[(size_t)bn] = 1;
        }
      }
    }
  }
  // the books
  std::vector<vamd_book_tab> tabs((size_t)nbooks);
  out->value_off.assign((size_t)nbooks, -1);
  out->values.clear();
  out->table_books = out->lattice_books = 0;
  h.nbooks = nbooks;
  h.off_books = place(tabs.data(), sizeof(vamd_book_tab) * tabs.size());
  for (int i = 0; i < nbooks; i++) {
    const HeaderBook &b = S.books[(size_t)i];
    vamd_book_tab &t = tabs[(size_t)i];
    memset(&t, 0, sizeof(t));
    if (b.entries < 1 || b.dim < 1) return header_refuse(err, "book " + num(i) + ": no entries, or dimension 0");
    if (b.entries > 65536) return header_refuse(err, "book " + num(i) + ": more than 65 536 entries");
    std::vector<uint32_t> codes;
    bool single = false;
    if (!header_make_words(b.len, &codes, &single))
      return header_refuse(err, "book " + num(i) + ": an over- or under-populated code tree (vorbis_synthesis_init refuses the stream)");
    t.dim = b.dim, t.entries = b.entries;
    header_book_lattice(b, &t);
    t.off_lengths = place(b.len.data(), b.len.size());
    t.off_codes = place(codes.data(), 4 * codes.size());
    if (!is_residue_book[(size_t)i]) continue;
    if (header_book_is_lattice(b, t)) {
      out->lattice_books++;
      continue;
    }
    if (out->values.size() + (size_t)b.entries * b.dim > VAMD_VALUES_MAX_FLOATS) return header_refuse(err, "more than 64 MiB of residue book values");
    std::vector<float> v;
    header_book_values(b, &v);
    out->value_off[(size_t)i] = (int32_t)out->values.size();
    out->values.insert(out->values.end(), v.begin(), v.end());
    out->table_books++;
  }
  while (im.size() & 15) im.push_back(0);
  h.total_bytes = (uint32_t)im.size();
  memcpy(im.data(), &h, sizeof(h));
  memcpy(im.data() + h.off_books, tabs.data(), sizeof(vamd_book_tab) * tabs.size());
  out->derived_off.assign(VAMD_DERIVED_SLOTS, 0u);
  out->derived.assign(VAMD_PSY_LOOKS, PsyDerived());
  for (PsyDerived &d : out->derived) d.bark_i1 = d.bark_i2 = d.fix_i1 = d.fix_i2 = d.ngroups = d.tail_linpos = 0;
  // the project's own predicates of a setup, at parse time: k_unpack's list, the residue back-end's, the floor ranges
  if (!unpack_check_setup(im, err)) return VAMD_EIMPL;
  Bound B;
  bind_params(im, out->derived_off, out->derived, im.data(), &B);
  for (int W = 0; W < modes; W++) {
    SynthFloorP F;
    if (!B.res_cap[W]) return header_refuse(err, "a residue outside what the residue rows hold (vamd_residue_capacity is 0)");
    if (!synth_floor_ranges(B.floor[W][0], B.floor[W][1], B.chmap[W].submaps, S.bs[W] / 2, &F)) return header_refuse(err, "a floor range that is no power of two");
  }
  return VAMD_OK;
}

// Both packets -> the image.  VAMD_OK; VAMD_ENOTVORBIS / VAMD_EBADHEADER / VAMD_EVERSION where vorbis_synthesis_headerin
// gives OV_ENOTVORBIS / OV_EBADHEADER / OV_EVERSION for the packet; VAMD_EIMPL for what it accepts and this does not cover.
inline int headers_to_image(const void *id, size_t id_bytes, const void *setup, size_t setup_bytes, HeaderImage *out, std::string *err) {
  HeaderSetup S;
  if (!id || !setup) return *err = "headers: null packet", VAMD_EINVAL;
  int r = header_parse_ident(id, id_bytes, &S);
  if (r) return *err = "headers: the identification header is refused as vorbis_synthesis_headerin refuses it", r;
  if ((r = header_parse_setup(setup, setup_bytes, &S))) return *err = "headers: the setup header is refused as vorbis_synthesis_headerin refuses it", r;
  return header_build_image(S, out, err);
}

}  // namespace vamd
