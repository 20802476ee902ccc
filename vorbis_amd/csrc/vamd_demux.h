// vamd_demux.h -- the host half of the Ogg decode entry (include/vorbis_amd.h: vamd_decode_ogg_plan, vamd_decode_ogg;
// vamd_decode.h; k_demux.h: k_ogg_depage): per file one walk over its page headers and lacing tables (doc/framing.html), which
// is serial in pages and touches about one byte in a hundred -- 27 + nseg of a page of some 4 KiB -- plus the three header
// packets and each audio packet's first byte.  What it leaves to the device is everything that touches every byte: the
// checksums, and moving the audio bytes to where k_unpack wants them.  Plain C++, no HIP: the library and the one-lane
// test program (tests/c/demux_host.cpp) share it.
//
// Out of the walk come the per-stream statuses (VAMD_STATUS_BADPAGE / _BADHEADER: include/vorbis_amd.h has the list), the
// packet table of a PACKED arena in which a stream's audio packets lie back to back (so k_unpack's bit offsets), each
// packet's first byte (decode_plan_build's mode bits), the end granule, and the page table k_ogg_depage works from.  A
// stream the walk flags gets no pages, no packets and no blocks.  No byte outside [file_offset[s], file_offset[s+1]) is
// read, whatever the file claims: every length is held against what is left of the file before it is used.
#pragma once
#include <stdint.h>
#include <string.h>
#include <string>
#include <vector>
#include "k_demux.h"

#ifndef VAMD_STATUS_BADPAGE  // (include/vorbis_amd.h; the test program includes this header without it)
#define VAMD_STATUS_BADPAGE 32
#define VAMD_STATUS_BADHEADER 64
#endif
#ifndef VAMD_STATUS_PARTIAL  // (k_unpack.h)
#define VAMD_STATUS_PARTIAL 128
#endif

namespace vamd {

// what the identification header must say (the blob's), and the setup header packet to compare with (or none)
struct DemuxSetup {
  int channels, rate, bs[2];
  const uint8_t *setup_header;
  int64_t setup_header_bytes;
};

struct DemuxScan {
  std::vector<uint8_t> status;        // [nstreams]
  std::vector<int64_t> offset;        // [npackets + 1] into the packed arena
  std::vector<uint8_t> first;         // [npackets] the packet's first byte (0 for an empty one)
  std::vector<int64_t> stream_start;  // [nstreams + 1] into the packets
  std::vector<int64_t> end_granule;   // [nstreams] of the page that completes the last audio packet; -1: none
  std::vector<OggDepage> pages;       // the device's page table
  std::vector<int64_t> page_start;    // [nstreams + 1] into pages
};

// the identification header as far as the blob can be held against it (Vorbis I 4.2.2): type 1, "vorbis", version 0,
// channels, rate, three bitrates (not looked at), the two block sizes as exponents in one byte
inline bool demux_ident_ok(const uint8_t *p, int64_t n, const DemuxSetup &S) {
  if (n < 30 || p[0] != 1 || memcmp(p + 1, "vorbis", 6) != 0) return false;
  if (ogg_le32(p + 7) != 0 || p[11] != S.channels || ogg_le32(p + 12) != (uint32_t)S.rate) return false;
  return (1 << (p[28] & 15)) == S.bs[0] && (1 << (p[28] >> 4)) == S.bs[1];
}

// One file, f[0 .. n).  `base`: where f[0] lies in the upload; `arena`: where the stream's first audio byte goes.  Appends
// to `out` the stream's packets and pages -- none where the status is not 0.
inline uint8_t demux_scan_file(const uint8_t *f, int64_t n, int64_t base, int stream, const DemuxSetup &S, DemuxScan *out) {
  const size_t packets0 = out->first.size(), pages0 = out->pages.size();
  int64_t arena = out->offset.back(), pos = 0, granule = -1;
  int64_t npackets = 0, len = 0;  // packets completed; bytes of the open one so far
  bool open = false;
  uint32_t serial = 0;
  uint8_t st = 0;
  std::vector<uint8_t> header[3];
  for (int64_t page = 0; pos < n && !st; page++) {
    if (n - pos < OGG_HEADER) st = VAMD_STATUS_BADPAGE;                                    // the file ends inside a page header
    else if (memcmp(f + pos, "OggS", 4) != 0 || f[pos + 4] != 0) st = VAMD_STATUS_BADPAGE;  // capture pattern, version
    if (st) break;
    const int flags = f[pos + 5], nseg = f[pos + 26];
    int64_t gp = 0;
    for (int i = 0; i < 8; i++) gp |= (int64_t)((uint64_t)f[pos + 6 + i] << (8 * i));
    const uint32_t ser = ogg_le32(f + pos + 14), seq = ogg_le32(f + pos + 18);
    if (page == 0) serial = ser;
    if (ser != serial || seq != (uint32_t)page || (page > 0 && (flags & 2)) || (bool)(flags & 1) != open) st = VAMD_STATUS_BADPAGE;
    if (n - pos - OGG_HEADER < nseg) st = VAMD_STATUS_BADPAGE;  // ... inside a lacing table
    if (st) break;
    const uint8_t *lace = f + pos + OGG_HEADER;
    int64_t body = 0;
    for (int q = 0; q < nseg; q++) body += lace[q];
    if (n - pos - OGG_HEADER - nseg < body) {  // ... inside a body
      st = VAMD_STATUS_BADPAGE;
      break;
    }
    const uint8_t *data = lace + nseg;
    int64_t at = 0, skip = 0;
    bool done_audio = false;
    for (int q = 0; q < nseg; q++) {
      const int v = lace[q];
      if (npackets < 3) {
        header[npackets].insert(header[npackets].end(), data + at, data + at + v);
        skip += v;
      } else if (!open) {
        out->first.push_back(v ? data[at] : 0);
      }
      open = true, len += v, at += v;
      if (v < 255) {
        if (npackets >= 3) out->offset.push_back(out->offset.back() + len), done_audio = true;
        npackets++, open = false, len = 0;
      }
    }
    if (done_audio) granule = gp < -1 ? -1 : gp;  // (no position is a bad descriptor's, not a file's: none)
    OggDepage row;
    row.src = base + pos, row.dst = arena;
    row.nseg = nseg, row.body = (int32_t)body, row.skip = (int32_t)skip, row.stream = stream;
    out->pages.push_back(row);
    arena += body - skip;
    pos += OGG_HEADER + nseg + body;
  }
  if (!st && open) st = VAMD_STATUS_BADPAGE;  // the file ends inside a packet
  if (!st) {
    if (npackets < 3 || !demux_ident_ok(header[0].data(), (int64_t)header[0].size(), S)) st = VAMD_STATUS_BADHEADER;
    else if (ogg_comment_check(header[1].data(), (int64_t)header[1].size()) != OGG_COMMENT_OK) st = VAMD_STATUS_BADHEADER;
    else if (header[2].size() < 7 || header[2][0] != 5 || memcmp(header[2].data() + 1, "vorbis", 6) != 0) st = VAMD_STATUS_BADHEADER;
    else if (S.setup_header && ((int64_t)header[2].size() != S.setup_header_bytes ||
                                memcmp(header[2].data(), S.setup_header, header[2].size()) != 0))
      st = VAMD_STATUS_BADHEADER;
  }
  if (st) {  // (an open packet's first byte may lie behind the last offset: both lists go back to where they were)
    out->first.resize(packets0), out->offset.resize(packets0 + 1), out->pages.resize(pages0);
    granule = -1;
  }
  out->end_granule.push_back(granule);
  return st;
}

// The three header packets of a file's first logical stream (vamd_ogg_read_headers): the walk above as far as the third
// packet's end, pages of another serial number passed over.  -> false where the pages do not hold three packets: a broken
// page header, a file that ends first.  Every length is held against what is left of the file before it is used.
inline bool demux_read_headers(const uint8_t *f, int64_t n, std::vector<uint8_t> header[3]) {
  int64_t pos = 0;
  int npackets = 0;
  uint32_t serial = 0;
  for (int64_t page = 0; npackets < 3; page++) {
    if (n - pos < OGG_HEADER || memcmp(f + pos, "OggS", 4) != 0 || f[pos + 4] != 0) return false;
    const int nseg = f[pos + 26];
    const uint32_t ser = ogg_le32(f + pos + 14);
    if (page == 0) serial = ser;
    if (n - pos - OGG_HEADER < nseg) return false;
    const uint8_t *lace = f + pos + OGG_HEADER;
    int64_t body = 0, at = 0;
    for (int q = 0; q < nseg; q++) body += lace[q];
    if (n - pos - OGG_HEADER - nseg < body) return false;
    const uint8_t *data = lace + nseg;
    for (int q = 0; q < nseg && npackets < 3 && ser == serial; q++) {
      const int v = lace[q];
      header[npackets].insert(header[npackets].end(), data + at, data + at + v);
      at += v;
      if (v < 255) npackets++;
    }
    pos += OGG_HEADER + nseg + body;
  }
  return true;
}

// -> false with a reason for a bad descriptor: nothing of the files has been read then
inline bool demux_scan(int64_t nstreams, const uint8_t *bytes, const int64_t *file_offset, const DemuxSetup &S, DemuxScan *out, std::string *err) {
  *out = DemuxScan();
  if (nstreams < 0) return *err = "decode_ogg: negative stream count", false;
  if (nstreams > 0x7fffffff) return *err = "decode_ogg: more than 2^31 streams", false;
  if (!file_offset) return *err = "decode_ogg: null file_offset", false;
  if (file_offset[0] < 0) return *err = "decode_ogg: negative file offset", false;
  for (int64_t s = 0; s < nstreams; s++)
    if (file_offset[s + 1] < file_offset[s]) return *err = "decode_ogg: file offsets are not monotone", false;
  if (file_offset[nstreams] > ((int64_t)1 << 40)) return *err = "decode_ogg: more than 2^40 bytes of files", false;
  if (file_offset[nstreams] > file_offset[0] && !bytes) return *err = "decode_ogg: null bytes", false;
  if (S.setup_header_bytes < 0 || (S.setup_header_bytes > 0 && !S.setup_header)) return *err = "decode_ogg: setup_header_bytes without a setup header", false;
  out->offset.push_back(0), out->stream_start.push_back(0), out->page_start.push_back(0);
  for (int64_t s = 0; s < nstreams; s++) {
    const int64_t o = file_offset[s], n = file_offset[s + 1] - o;
    out->status.push_back(demux_scan_file(n ? bytes + o : nullptr, n, o - file_offset[0], (int)s, S, out));
    out->stream_start.push_back((int64_t)out->first.size());
    out->page_start.push_back((int64_t)out->pages.size());
  }
  return true;
}

}  // namespace vamd
