// vamd_decode_plan.h -- the host half of the packet decoder (vamd_decode.h; k_unpack.h): what is worked out once per
// setup -- whether k_unpack's walk is safe on it, the codebooks' decode tables -- and once per call, before anything is
// enqueued: the block plan of a group of streams out of their packets' own mode bits.  Plain C++, no HIP: the library and
// the one-lane test program (tests/c/unpack_host.cpp) share it.
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <string>
#include <vector>
#include "k_unpack.h"

namespace vamd {

// What k_unpack takes for granted of a setup (its loops and table indices are the setup's): the floors' class tables
// name posts and books that exist, the residues' classes and books likewise.  build_image checks the blob's geometry;
// this is the decoder's own list.
inline bool unpack_check_setup(const std::vector<unsigned char> &image, std::string *err) {
  vamd_setup_header h;
  if (image.size() < sizeof(h)) return *err = "decode: no setup", false;
  memcpy(&h, image.data(), sizeof(h));
  auto bad = [&](const char *what) { return *err = std::string("decode: the setup's ") + what, false; };
  if (h.modes < 1 || h.modes > 2 || h.modebits < 0 || h.modebits > 6 || (1 << h.modebits) < h.modes) return bad("modes");
  if (h.nbooks < 1 || h.nbooks > 255 || (size_t)h.off_books + (size_t)h.nbooks * sizeof(vamd_book_tab) > image.size()) return bad("book list");
  const vamd_book_tab *bk = (const vamd_book_tab *)(image.data() + h.off_books);
  for (int b = 0; b < h.nbooks; b++) {
    if (bk[b].entries < 1 || bk[b].entries > 65536 || bk[b].dim < 1) return bad("codebook sizes");
    if ((size_t)bk[b].off_lengths + (size_t)bk[b].entries > image.size() || (size_t)bk[b].off_codes + 4 * (size_t)bk[b].entries > image.size())
      return bad("codebook tables");
    const signed char *len = (const signed char *)(image.data() + bk[b].off_lengths);
    for (int i = 0; i < bk[b].entries; i++)
      if (len[i] > 32) return bad("codeword lengths");
  }
  auto book_ok = [&](int b) { return b >= 0 && b < h.nbooks; };
  for (int W = 0; W < h.modes; W++) {
    const vamd_mode_tab &m = h.mode[W];
    if (m.submaps < 1 || m.submaps > VAMD_MAX_SUBMAPS) return bad("submaps");
    for (int sm = 0; sm < m.submaps; sm++) {
      const vamd_floor1_tab &f = m.floor[sm];
      if (f.posts < 2 || f.posts > VAMD_POSIT || f.partitions < 0 || f.partitions > VAMD_FLOOR_PARTS) return bad("floor posts");
      int posts = 2;
      for (int i = 0; i < f.partitions; i++) {
        const int c = f.partitionclass[i];
        if (c < 0 || c >= VAMD_FLOOR_CLASSES) return bad("floor partition classes");
        if (f.class_dim[c] < 1 || f.class_dim[c] > 8 || f.class_subs[c] < 0 || f.class_subs[c] > 3) return bad("floor class sizes");
        if (f.class_subs[c] && !book_ok(f.class_book[c])) return bad("floor class books");
        for (int k = 0; k < (1 << f.class_subs[c]); k++)
          if (f.class_subbook[c][k] >= h.nbooks) return bad("floor sub-books");
        posts += f.class_dim[c];
      }
      if (posts != f.posts) return bad("floor classes do not add up to its posts");
      for (int i = 0; i < f.posts; i++) {
        if (f.forward_index[i] < 0 || f.forward_index[i] >= f.posts || f.postlist[i] < 0) return bad("floor post order");
        if (i >= 2 && (f.loneighbor[i - 2] < 0 || f.loneighbor[i - 2] >= f.posts || f.hineighbor[i - 2] < 0 || f.hineighbor[i - 2] >= f.posts))
          return bad("floor neighbours");
      }
      const vamd_residue_tab &t = h.res[W][sm];
      if (t.partitions < 1 || t.partitions > VAMD_RES_MAXCLASS || t.stages < 0 || t.stages > VAMD_RES_MAXSTAGE || t.grouping < 1)
        return bad("residue classes");
      if (!book_ok(t.groupbook) || t.groupbook_dim < 1 || t.groupbook_dim > 16) return bad("residue phrase book");
      for (int c = 0; c < t.partitions; c++)
        for (int s = 0; s < t.stages; s++)
          if (((t.secondstages[c] >> s) & 1) && t.partbooks[c][s] >= h.nbooks) return bad("residue books");
    }
  }
  return true;
}

// The decode tables of every book (UnpackBook), as lib/sharedbook.c:294-437 builds a dec_codebook: a first level on
// ilog(used entries) - 4 bits, held to 5 .. 8, and the codewords longer than that sorted by their bit-reversed value.
inline void unpack_build_tables(const std::vector<unsigned char> &image, std::vector<unsigned char> *tab, UnpackP *U) {
  vamd_setup_header h;
  memcpy(&h, image.data(), sizeof(h));
  const vamd_book_tab *bk = (const vamd_book_tab *)(image.data() + h.off_books);
  std::vector<UnpackBook> head((size_t)h.nbooks);
  std::vector<uint32_t> body;
  const size_t body_at = ((size_t)h.nbooks * sizeof(UnpackBook) + 15) & ~(size_t)15;
  auto rev = [](uint32_t x) {
    uint32_t r = 0;
    for (int b = 0; b < 32; b++) r |= ((x >> b) & 1u) << (31 - b);
    return r;
  };
  for (int b = 0; b < h.nbooks; b++) {
    const signed char *len = (const signed char *)(image.data() + bk[b].off_lengths);
    std::vector<uint32_t> code((size_t)bk[b].entries);
    memcpy(code.data(), image.data() + bk[b].off_codes, 4 * code.size());
    int used = 0;
    for (int i = 0; i < bk[b].entries; i++) used += len[i] > 0;
    int k = 0;
    for (unsigned v = (unsigned)used; v; v >>= 1) k++;
    k = std::min(8, std::max(5, k - 4));
    std::vector<uint32_t> first((size_t)2 << k, 0u);
    struct Long {
      uint32_t key, info;
    };
    std::vector<Long> longs;
    for (int i = 0; i < bk[b].entries; i++) {
      const int l = len[i];
      if (l <= 0) continue;
      const uint32_t c = l < 32 ? code[i] & ((1u << l) - 1u) : code[i];
      if (l <= k) {
        // (a book whose one used entry has length 1: the reference reads that entry from one bit of either value,
        // lib/sharedbook.c:523-530 -- every slot is its)
        const uint32_t step = used == 1 && l == 1 ? 1u : 1u << l;
        for (uint32_t s = c & (step - 1u); s < (1u << k); s += step) first[2 * s] = (uint32_t)i, first[2 * s + 1] = (uint32_t)l;
      } else {
        longs.push_back({rev(c), (uint32_t)i | (uint32_t)l << 24});
      }
    }
    std::sort(longs.begin(), longs.end(), [](const Long &a, const Long &c) { return a.key < c.key; });
    for (size_t i = 0; i < longs.size();) {  // the run of codewords that share their first k bits
      const uint32_t s = rev(longs[i].key) & ((1u << k) - 1u);
      size_t j = i;
      while (j < longs.size() && (rev(longs[j].key) & ((1u << k) - 1u)) == s) j++;
      if (!first[2 * s + 1]) first[2 * s] = (uint32_t)i, first[2 * s + 1] = (uint32_t)j << 8;  // (a prefix code: no short word owns the slot)
      i = j;
    }
    UnpackBook &o = head[(size_t)b];
    memset(&o, 0, sizeof(o));
    o.entries = bk[b].entries, o.k = k, o.nsorted = (int)longs.size(), o.used = used;
    o.off_first = (uint32_t)(body_at + 4 * body.size());
    body.insert(body.end(), first.begin(), first.end());
    o.off_codes = (uint32_t)(body_at + 4 * body.size());
    for (const Long &e : longs) body.push_back(e.key);
    o.off_info = (uint32_t)(body_at + 4 * body.size());
    for (const Long &e : longs) body.push_back(e.info);
  }
  tab->assign(body_at + 4 * body.size() + 16, 0);
  memcpy(tab->data(), head.data(), head.size() * sizeof(UnpackBook));
  if (!body.empty()) memcpy(tab->data() + body_at, body.data(), 4 * body.size());
  U->tab = tab->data();
  U->nbooks = h.nbooks, U->modes = h.modes, U->modebits = h.modebits;
}

// A group of streams' blocks out of their packets: what LapP (k_synth.h) wants, and where each block's packet lies.
struct DecodePlan {
  int64_t nblocks[2] = {0, 0};
  std::vector<int32_t> order;      // the planned blocks, stream after stream: W << 30 | index inside W's batch
  std::vector<int64_t> lap_start;  // [nstreams + 1] into order[]
  std::vector<int64_t> src[2];     // [nblocks[W]] the block's first sample; a stream's first centre is 0
  std::vector<int64_t> packet;     // [blocks] the packet of each block of order[]
  // (a live decoder's plan, vamd_decode_live_plan.h, also holds carried blocks in order[], lap_start and src[W] -- extra[W]
  // rows behind the nblocks[W] unpacked ones -- and names the blocks that have a packet in lists of their own)
  int64_t extra[2] = {0, 0};
  std::vector<int64_t> frames;     // [nstreams]
  std::vector<uint8_t> status;     // [nstreams] what the packets' heads already tell: such a stream has no blocks
  int64_t max_frames = 0;
  // (a plan made from per-packet marks, decode_plan_build_marked below, also lists the runs of frames its streams keep)
  struct Segment {
    int64_t stream, k0, k1;        // blocks [k0, k1) of order[]: the link the run lies in, its first centre at 0
    int64_t first, count, out_at;  // frames [first, first + count) of the link, at out_at of the stream's frames
  };
  std::vector<Segment> segments;
};

// the size class a packet's first byte names, or -VAMD_STATUS_* (lib/synthesis.c:44-57; the mode number is the size class
// here: lib/mapping0.c:248 as the encoder side has it)
inline int decode_packet_class(const uint8_t *p, int64_t len, int modes, int modebits) {
  if (len < 1) return -VAMD_STATUS_TRUNCATED;
  if (p[0] & 1) return -VAMD_STATUS_NOTAUDIO;
  const int mode = (p[0] >> 1) & ((1 << modebits) - 1);
  if (mode >= modes) return -VAMD_STATUS_NOTAUDIO;
  return modes > 1 ? mode : 0;
}

// the frames between the centres of two neighbouring blocks of size classes lW and W (lib/block.c:840-842)
inline int64_t decode_step(const int bs[2], int lW, int W) { return bs[lW] / 4 + bs[W] / 4; }

// what every packet descriptor must hold (vamd_decode_desc, vamd_decode_live_desc) -> false with a reason
inline bool decode_desc_check(int64_t nstreams, int64_t npackets, const uint8_t *bytes, const int64_t *offset, const int64_t *stream_start,
                              const int64_t *end_granule, const uint8_t *first, std::string *err) {
  if (nstreams < 0 || npackets < 0) return *err = "decode: negative stream or packet count", false;
  if (!offset || !stream_start) return *err = "decode: null offset / stream_start", false;
  if (offset[0] < 0) return *err = "decode: negative packet offset", false;
  for (int64_t p = 0; p < npackets; p++)
    if (offset[p + 1] < offset[p]) return *err = "decode: packet offsets are not monotone", false;
  if (offset[npackets] > ((int64_t)1 << 40)) return *err = "decode: more than 2^40 bytes of packets", false;
  if (offset[npackets] > 0 && !bytes && !first) return *err = "decode: null bytes", false;
  if (stream_start[0] < 0 || stream_start[nstreams] > npackets) return *err = "decode: stream_start outside the packets", false;
  for (int64_t s = 0; s < nstreams; s++) {
    if (stream_start[s + 1] < stream_start[s]) return *err = "decode: stream_start is not monotone", false;
    if (end_granule && end_granule[s] < -1) return *err = "decode: a granule position below -1", false;
  }
  return true;
}

// -> false with a reason for a bad descriptor.  end_granule: NULL, or per stream the last packet's granule position
// (-1: none): the frames the stream's last block adds are cut to it, as vorbis_synthesis_blockin does for a stream that
// began at granule 0 (lib/block.c:906-935; never by more than that block adds).  first: NULL, or per packet its first byte --
// a caller whose packets are not yet together anywhere (vamd_demux.h: they lie in pages, and the packed arena exists on
// the device alone) hands the mode bits over this way, and `bytes` is not read.
inline bool decode_plan_build(const int bs[2], int modes, int modebits, int64_t nstreams, int64_t npackets, const uint8_t *bytes,
                              const int64_t *offset, const int64_t *stream_start, const int64_t *end_granule, DecodePlan *P, std::string *err,
                              const uint8_t *first = nullptr) {
  *P = DecodePlan();
  if (!decode_desc_check(nstreams, npackets, bytes, offset, stream_start, end_granule, first, err)) return false;
  P->frames.assign((size_t)nstreams, 0);
  P->status.assign((size_t)nstreams, 0);
  P->lap_start.assign((size_t)nstreams + 1, 0);
  std::vector<int> cls;
  for (int64_t s = 0; s < nstreams; s++) {
    const int64_t p0 = stream_start[s], p1 = stream_start[s + 1];
    cls.clear();
    uint8_t st = 0;
    for (int64_t p = p0; p < p1; p++) {
      const int W = decode_packet_class(first ? first + p : bytes + offset[p], offset[p + 1] - offset[p], modes, modebits);
      if (W < 0) st |= (uint8_t)-W;
      cls.push_back(W);
    }
    P->status[(size_t)s] = st;
    if (!st) {
      int64_t at = 0, step = 0;
      for (int64_t p = p0; p < p1; p++) {
        const int W = cls[(size_t)(p - p0)];
        step = p > p0 ? decode_step(bs, cls[(size_t)(p - p0 - 1)], W) : 0;
        at += step;
        if (P->nblocks[W] >= (1 << 30)) return *err = "decode: more than 2^30 blocks of a size class", false;
        P->order.push_back((int32_t)(W << 30) | (int32_t)P->nblocks[W]++);
        P->src[W].push_back(at - bs[W] / 2);
        P->packet.push_back(p);
      }
      int64_t frames = p1 - p0 >= 2 ? at : 0;
      if (end_granule && end_granule[s] >= 0 && end_granule[s] < frames) frames -= std::min(frames - end_granule[s], step);
      P->frames[(size_t)s] = frames;
      P->max_frames = std::max(P->max_frames, frames);
    }
    P->lap_start[(size_t)s + 1] = (int64_t)P->order.size();
  }
  return true;
}

// The plan from per-packet MARKS, as a reader of the container has them: granule[p] the granule position of the page on
// which packet p completes where it is the last to complete there, else -1 (a position below -1 is none too, as the page
// walk reads it: vamd_demux.h); eos[p] libogg's e_o_s (NULL: each stream's last packet).  What a stream keeps of its
// blocks' frames is what vorbis_synthesis_blockin leaves a caller who drains after every packet (lib/block.c:858-937):
// with count the frames added so far (0 after the first packet, + add_p = bs[W_{p-1}]/4 + bs[W_p]/4 per later one) and pos
// the tracked position (-1 at first),
//   pos == -1, granule[p] != -1   pos = granule[p]; where count > granule[p], min(count - granule[p], add_p) of packet p's
//                                 own frames go: its last with eos[p], else its first
//   pos != -1                     pos += add_p; where granule[p] != -1 and differs: with pos > granule[p] and eos[p],
//                                 min(pos - granule[p], add_p) of its last frames go; pos = granule[p] either way
// so no cut exceeds what its packet adds, and a first page's trim takes frames of the LAST packet of that page.
// links (or NULL) / nlinks: packet indices, ascending, at which a stream's packets begin a new LINK (vamd_demux.h): a
// fresh lap -- its first block gives no output -- and a fresh walk; a stream's frames are its links' end to end.
// Out come frames[] and segments[], a row per run of kept frames; order[], src[] and packet[] as above, src[] per link.
inline bool decode_plan_build_marked(const int bs[2], int modes, int modebits, int64_t nstreams, int64_t npackets, const uint8_t *bytes,
                                     const int64_t *offset, const int64_t *stream_start, const int64_t *granule, const uint8_t *eos, DecodePlan *P,
                                     std::string *err, const uint8_t *first = nullptr, const int64_t *links = nullptr, int64_t nlinks = 0) {
  *P = DecodePlan();
  if (!decode_desc_check(nstreams, npackets, bytes, offset, stream_start, nullptr, first, err)) return false;
  if (npackets > 0 && !granule) return *err = "decode: null granule marks", false;
  for (int64_t j = 0; j < nlinks; j++)
    if (links[j] < 0 || links[j] > npackets || (j && links[j] < links[j - 1])) return *err = "decode: link starts outside the packets", false;
  P->frames.assign((size_t)nstreams, 0);
  P->status.assign((size_t)nstreams, 0);
  P->lap_start.assign((size_t)nstreams + 1, 0);
  std::vector<int> cls;
  int64_t link = 0;
  for (int64_t s = 0; s < nstreams; s++) {
    const int64_t p0 = stream_start[s], p1 = stream_start[s + 1];
    cls.clear();
    uint8_t st = 0;
    for (int64_t p = p0; p < p1; p++) {
      const int W = decode_packet_class(first ? first + p : bytes + offset[p], offset[p + 1] - offset[p], modes, modebits);
      if (W < 0) st |= (uint8_t)-W;
      cls.push_back(W);
    }
    P->status[(size_t)s] = st;
    while (link < nlinks && links[link] <= p0) link++;
    int64_t out_at = 0;
    for (int64_t q0 = p0; !st && q0 < p1;) {
      int64_t q1 = p1;
      if (link < nlinks && links[link] < p1) q1 = links[link++];
      const int64_t k0 = (int64_t)P->order.size();
      const size_t seg0 = P->segments.size();
      int64_t count = 0, pos = -1, run_first = 0, run_end = 0;  // the open run of kept frames, in the link's frames
      auto close_run = [&]() {
        if (run_end > run_first) P->segments.push_back({s, k0, 0, run_first, run_end - run_first, out_at}), out_at += run_end - run_first;
      };
      for (int64_t p = q0; p < q1; p++) {
        const int W = cls[(size_t)(p - p0)];
        const int64_t add = p > q0 ? decode_step(bs, cls[(size_t)(p - p0 - 1)], W) : 0;
        if (P->nblocks[W] >= (1 << 30)) return *err = "decode: more than 2^30 blocks of a size class", false;
        P->order.push_back((int32_t)(W << 30) | (int32_t)P->nblocks[W]++);
        P->src[W].push_back(count + add - bs[W] / 2);
        P->packet.push_back(p);
        const int64_t lo = count, g = granule[p] < -1 ? -1 : granule[p];
        const bool e = eos ? eos[p] != 0 : p == p1 - 1;
        count += add;
        int64_t front = 0, back = 0;
        if (pos == -1) {
          if (g != -1) {
            pos = g;
            if (count > g) (e ? back : front) = std::min(count - g, add);
          }
        } else {
          pos = (int64_t)((uint64_t)pos + (uint64_t)add);  // (the reference's sum, wrapping where a position near 2^63 was believed)
          if (g != -1 && pos != g) {
            if (pos > g && e) back = std::min(pos - g, add);  // (g >= 0: the difference holds)
            pos = g;
          }
        }
        if (lo + front != run_end) close_run(), run_first = run_end = lo + front;
        run_end = count - back;
        if (back) close_run(), run_first = run_end = count;
      }
      close_run();
      for (size_t i = seg0; i < P->segments.size(); i++) P->segments[i].k1 = (int64_t)P->order.size();
      q0 = q1;
    }
    P->frames[(size_t)s] = out_at;
    P->max_frames = std::max(P->max_frames, out_at);
    P->lap_start[(size_t)s + 1] = (int64_t)P->order.size();
  }
  return true;
}

}  // namespace vamd
