// vamd_demux_live.h -- the host half of the live Ogg decoder (include/vorbis_amd.h: vamd_decode_ogg_live_*;
// vamd_decode_ogg_live.h; k_demux.h: k_ogg_depage between k_ogg_packet_carry_in and _out): the next bytes of continuing Ogg
// Vorbis streams, cut at any byte, to the tables a call's launches work from.  It is demux_scan_file's walk (vamd_demux.h)
// with its local state -- page count, serial, the open packet, the header packets, the granule -- moved into a per-slot
// struct, and two things a file does not have: a page the cut divides is HELD on the host until the piece that completes
// it, and an audio packet that whole pages leave open stays on the DEVICE, in the slot's row of a byte carry; the host
// keeps its length and its first byte (the mode bits the block plan needs once it completes).  Plain C++, no HIP: the
// library and the one-lane test program (tests/c/demux_live_host.cpp) share it.
//
// The per-page step is restated from demux_scan_file, check for check and in its order, not shared with it: there a
// length that does not fit is the file's end (BADPAGE), here it is "not yet" (hold), the header packets are checked when
// the third completes and not behind the last page, and a packet's first byte is recorded when it completes.
//
// A call's arena: stream after stream a region -- room for the slot's carried bytes (k_ogg_packet_carry_in fills it), then
// the audio bytes of the call's whole pages as k_ogg_depage lays them.  The packets completed in the call lie back to
// back from the region's start; the packet still open lies behind them and goes to the carry (k_ogg_packet_carry_out).  So
// packets of neighbouring streams do NOT lie back to back: `begin` says where each does, X.offset holds the lengths as a
// running sum.  No byte outside [piece_offset[s], piece_offset[s+1]) is read, whatever the stream claims.
#pragma once
#include "vamd_demux.h"

namespace vamd {

enum { OGG_MAX_PAGE = OGG_HEADER + OGG_MAX_SEGS + OGG_MAX_SEGS * 255 };  // 65 307 bytes: a held tail is shorter

// A slot between calls.  Free (as constructed) until its first byte arrives; then one logical bitstream until a piece
// closes it.
struct DemuxLiveSlot {
  int64_t pages = 0;       // whole pages walked: the next page's sequence number
  uint32_t serial = 0;     // page 0's
  bool open = false;       // a packet is open behind the last whole page
  int64_t npackets = 0;    // packets completed, the three headers included
  int64_t len = 0;         // bytes of the open packet so far; an audio packet's lie in the slot's carry row
  uint8_t first = 0;       // the open packet's first byte
  std::vector<uint8_t> header[3];  // the header packets so far; released once they have been checked
  int64_t header_bytes = 0;
  int64_t granule = -1;    // of the last page that completed an audio packet
  bool ended = false;      // the end-of-stream page has been seen: any further page is BADPAGE
  uint8_t dead = 0;        // the stream's status since it was flagged: no frames until a piece closes it
  std::vector<uint8_t> held;  // the bytes behind the last whole page: less than one page
};

struct DemuxLiveCall {
  DemuxScan X;                      // status, offset (the packets' lengths, a running sum), first, stream_start, end_granule
                                    // (what cuts the last block in THIS call, else -1), pages (src: into upload), page_start
  std::vector<int64_t> begin;       // [npackets] where the packet begins in the arena
  std::vector<uint8_t> close;       // [nstreams] what the block plan takes as "the stream ends here": close[] or the end-of-stream page
  std::vector<OggCarryRow> in, out; // k_ogg_packet_carry_in's and _out's tables
  std::vector<uint8_t> upload;      // the call's whole pages, stream after stream: what goes up in one copy
  int64_t arena_bytes = 0;
  std::vector<DemuxLiveSlot> next;  // [nstreams] the slot behind this call, unless the device flags the stream
};

// the three header packets, as demux_scan_file holds them against the setup behind its walk
inline uint8_t demux_headers_status(const std::vector<uint8_t> header[3], const DemuxSetup &S) {
  if (!demux_ident_ok(header[0].data(), (int64_t)header[0].size(), S)) return VAMD_STATUS_BADHEADER;
  if (ogg_comment_check(header[1].data(), (int64_t)header[1].size()) != OGG_COMMENT_OK) return VAMD_STATUS_BADHEADER;
  if (header[2].size() < 7 || header[2][0] != 5 || memcmp(header[2].data() + 1, "vorbis", 6) != 0) return VAMD_STATUS_BADHEADER;
  if (S.setup_header && ((int64_t)header[2].size() != S.setup_header_bytes || memcmp(header[2].data(), S.setup_header, header[2].size()) != 0))
    return VAMD_STATUS_BADHEADER;
  return 0;
}

// One stream's piece, p[0 .. n), behind what the slot holds.  Appends to `out` the stream's rows -- none where the status
// is not 0 -- and leaves the slot behind the piece in *now.
inline uint8_t demux_live_piece(const uint8_t *p, int64_t n, int stream, int slot, bool closing, const DemuxSetup &S, int64_t max_packet_bytes,
                                int64_t max_header_bytes, DemuxLiveSlot *now, DemuxLiveCall *out) {
  DemuxScan &X = out->X;
  const size_t packets0 = X.first.size(), pages0 = X.pages.size(), up0 = out->upload.size(), in0 = out->in.size();
  const int64_t region = out->arena_bytes;
  uint8_t st = now->dead;
  int64_t end_granule = -1;
  if (!st) {
    // the held tail and the piece, together, where the whole pages among them will go up from
    out->upload.insert(out->upload.end(), now->held.begin(), now->held.end());
    if (n) out->upload.insert(out->upload.end(), p, p + n);
    now->held.clear();
    const uint8_t *f = out->upload.data() + up0;
    const int64_t have = (int64_t)(out->upload.size() - up0);
    const int64_t carried = now->open && now->npackets >= 3 ? now->len : 0;
    int64_t arena = region + carried, start = region, pos = 0;  // start: where the next packet to complete begins
    bool done_any = false, done_last_eos = false;
    while (!st && have - pos >= OGG_HEADER) {  // (demux_scan_file's page step from here on)
      if (now->ended || memcmp(f + pos, "OggS", 4) != 0 || f[pos + 4] != 0) st = VAMD_STATUS_BADPAGE;  // a page behind the last; capture pattern, version
      if (st) break;
      const int flags = f[pos + 5], nseg = f[pos + 26];
      int64_t gp = 0;
      for (int i = 0; i < 8; i++) gp |= (int64_t)((uint64_t)f[pos + 6 + i] << (8 * i));
      const uint32_t ser = ogg_le32(f + pos + 14), seq = ogg_le32(f + pos + 18);
      if (now->pages == 0) now->serial = ser;
      if (ser != now->serial || seq != (uint32_t)now->pages || (now->pages > 0 && (flags & 2)) || (bool)(flags & 1) != now->open) st = VAMD_STATUS_BADPAGE;
      if (st) break;
      if (have - pos - OGG_HEADER < nseg) break;  // the cut lies inside the lacing table: held
      const uint8_t *lace = f + pos + OGG_HEADER;
      int64_t body = 0;
      for (int q = 0; q < nseg; q++) body += lace[q];
      if (have - pos - OGG_HEADER - nseg < body) break;  // ... inside the body: held
      const uint8_t *data = lace + nseg;
      int64_t at = 0, skip = 0;
      bool done_audio = false;
      for (int q = 0; q < nseg && !st; q++) {
        const int v = lace[q];
        if (now->npackets < 3) {
          std::vector<uint8_t> &h = now->header[now->npackets];
          now->header_bytes += v;
          if (now->header_bytes > max_header_bytes) st = VAMD_STATUS_BADHEADER;  // (before the bytes are kept)
          else h.insert(h.end(), data + at, data + at + v);
          skip += v;
        } else if (!now->open) {
          now->first = v ? data[at] : 0;
        }
        now->open = true, now->len += v, at += v;
        if (v < 255 && !st) {
          if (now->npackets >= 3) {
            X.first.push_back(now->first), out->begin.push_back(start), X.offset.push_back(X.offset.back() + now->len);
            start += now->len, done_audio = true;
          }
          now->npackets++, now->open = false, now->len = 0;
          if (now->npackets == 3) {
            st = demux_headers_status(now->header, S);
            for (int k = 0; k < 3; k++) std::vector<uint8_t>().swap(now->header[k]);
          }
        }
      }
      if (st) break;
      if (done_audio) now->granule = gp < -1 ? -1 : gp, done_any = true, done_last_eos = (flags & 4) != 0;
      if (flags & 4) now->ended = true;
      OggDepage row;
      row.src = (int64_t)up0 + pos, row.dst = arena;
      row.nseg = nseg, row.body = (int32_t)body, row.skip = (int32_t)skip, row.stream = stream;
      X.pages.push_back(row);
      arena += body - skip;
      pos += OGG_HEADER + nseg + body;
      now->pages++;
    }
    const bool audio_open = now->open && now->npackets >= 3;
    if (!st && closing) {
      if (pos < have || now->open) st = VAMD_STATUS_BADPAGE;      // the stream ends inside a page / a packet
      else if (now->npackets < 3) st = VAMD_STATUS_BADHEADER;     // ... before its three headers: a file of no bytes
    }
    if (!st && audio_open && now->len > max_packet_bytes) st = VAMD_STATUS_BADPAGE;  // more than a carry row holds
    if (!st) {
      now->held.assign(f + pos, f + have);
      out->upload.resize(up0 + (size_t)pos);
      if (X.pages.size() > pages0) {  // (a call that completes no page of the stream moves nothing: the carry stands)
        if (carried) out->in.push_back(OggCarryRow{region, slot, (int32_t)carried});
        if (audio_open) out->out.push_back(OggCarryRow{start, slot, (int32_t)now->len});
        out->arena_bytes = arena;
      }
      if (done_any && (done_last_eos || closing)) end_granule = now->granule;
    }
  }
  if (st) {  // no rows, no packets, nothing to upload; the stream is dead until a piece closes it
    X.first.resize(packets0), X.offset.resize(packets0 + 1), out->begin.resize(packets0), X.pages.resize(pages0);
    out->upload.resize(up0), out->in.resize(in0);
    out->arena_bytes = region;
    now->dead = st;
    now->held.clear();
    for (int k = 0; k < 3; k++) std::vector<uint8_t>().swap(now->header[k]);
  }
  X.end_granule.push_back(end_granule);
  out->close.push_back(closing || now->ended || st);
  if (closing) *now = DemuxLiveSlot();
  return st;
}

// -> false with a reason for a bad descriptor: nothing of the pieces has been read then.  Reads `slots` ([max_streams])
// and changes nothing.  Every index the kernels use -- the pages' runs of the upload and the arena, the carry rows' slots
// and runs -- is set here and checked against the buffers' sizes before it returns.
inline bool demux_live_scan(const std::vector<DemuxLiveSlot> &slots, int64_t nstreams, const int64_t *slot, const uint8_t *bytes, const int64_t *piece_offset,
                            const uint8_t *close, const DemuxSetup &S, int64_t max_packet_bytes, int64_t max_header_bytes, DemuxLiveCall *out,
                            std::string *err) {
  *out = DemuxLiveCall();
  const int64_t max_streams = (int64_t)slots.size();
  if (nstreams < 0) return *err = "decode_ogg_live: negative stream count", false;
  if (nstreams > max_streams) return *err = "decode_ogg_live: more streams than the decoder has slots", false;
  if (nstreams && !slot) return *err = "decode_ogg_live: null slot", false;
  if (!piece_offset) return *err = "decode_ogg_live: null piece_offset", false;
  if (piece_offset[0] < 0) return *err = "decode_ogg_live: negative piece offset", false;
  for (int64_t s = 0; s < nstreams; s++)
    if (piece_offset[s + 1] < piece_offset[s]) return *err = "decode_ogg_live: piece offsets are not monotone", false;
  if (piece_offset[nstreams] > ((int64_t)1 << 40)) return *err = "decode_ogg_live: more than 2^40 bytes of pieces", false;
  if (piece_offset[nstreams] > piece_offset[0] && !bytes) return *err = "decode_ogg_live: null bytes", false;
  std::vector<uint8_t> named((size_t)max_streams, 0);
  for (int64_t s = 0; s < nstreams; s++) {
    if (slot[s] < 0 || slot[s] >= max_streams) return *err = "decode_ogg_live: a slot outside 0 .. max_streams-1", false;
    if (named[(size_t)slot[s]]++) return *err = "decode_ogg_live: a slot named twice", false;
  }
  DemuxScan &X = out->X;
  X.offset.push_back(0), X.stream_start.push_back(0), X.page_start.push_back(0);
  out->next.reserve((size_t)nstreams);
  for (int64_t s = 0; s < nstreams; s++) {
    const int64_t o = piece_offset[s], n = piece_offset[s + 1] - o;
    out->next.push_back(slots[(size_t)slot[s]]);
    X.status.push_back(demux_live_piece(n ? bytes + o : nullptr, n, (int)s, (int)slot[s], close && close[s], S, max_packet_bytes, max_header_bytes,
                                        &out->next.back(), out));
    X.stream_start.push_back((int64_t)X.first.size());
    X.page_start.push_back((int64_t)X.pages.size());
  }
  // what the kernels index with, once more, against the buffers' sizes
  const int64_t stride = (max_packet_bytes + 3) & ~(int64_t)3;
  if (X.pages.size() > 0x7fffffffu) return *err = "decode_ogg_live: more than 2^31 pages", false;
  for (const OggDepage &pg : X.pages)
    if (!ogg_depage_inside(pg, (int64_t)out->upload.size(), out->arena_bytes)) return *err = "decode_ogg_live: a page outside its buffers", false;
  for (const OggCarryRow &r : out->in)
    if (!ogg_carry_inside(r, out->arena_bytes, max_streams, stride)) return *err = "decode_ogg_live: a carried packet outside its buffers", false;
  for (const OggCarryRow &r : out->out)
    if (!ogg_carry_inside(r, out->arena_bytes, max_streams, stride)) return *err = "decode_ogg_live: an open packet outside its buffers", false;
  for (size_t k = 0; k < out->begin.size(); k++)
    if (out->begin[k] < 0 || out->begin[k] + (X.offset[k + 1] - X.offset[k]) > out->arena_bytes) return *err = "decode_ogg_live: a packet outside the arena", false;
  return true;
}

// The slots behind a call that has succeeded: status[s] as the call gave it (the walk's, the block plan's, the device's).
// A stream flagged in a piece that does not close it is dead from there on.
inline void demux_live_commit(std::vector<DemuxLiveSlot> *slots, DemuxLiveCall *L, int64_t nstreams, const int64_t *slot, const uint8_t *close,
                              const uint8_t *status) {
  for (int64_t s = 0; s < nstreams; s++) {
    DemuxLiveSlot &now = L->next[(size_t)s];
    const uint8_t flagged = status[s] & (uint8_t)~VAMD_STATUS_PARTIAL;  // (a packet kept under vamd_decode_partial costs its stream nothing)
    if (flagged && !(close && close[s])) {
      now.dead = flagged;
      now.held.clear();
    }
    (*slots)[(size_t)slot[s]] = std::move(now);
  }
}

}  // namespace vamd
