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
// Under the follow policy (vamd_decode_follow) the walk is demux_scan_file_links, below: links, foreign pages, and a granule
// and end-of-stream mark per packet in the end granule's place (tests/c/decode_links_host.cpp).
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
  // under the follow policy (demux_scan_file_links): the marks per packet, and the packets at which later links begin
  std::vector<int64_t> granule;       // [npackets] the page's granule position on the last packet it completes, else -1
  std::vector<uint8_t> eos;           // [npackets] that page's end-of-stream flag
  std::vector<int64_t> links;         // ascending, into the packets
};
inline uint8_t demux_scan_file_links(const uint8_t *f, int64_t n, int64_t base, int stream, const DemuxSetup &S, DemuxScan *out);

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

// ---- files as a reader takes them: links and foreign pages (vamd_decode_follow) ----------------------------------------------
// A page's header and lacing table held against what is left of the file -> false where the file ends first or the
// capture pattern or version is wrong.  Every page of a followed file goes through this, a foreign one included.
struct DemuxPage {
  int flags, nseg;
  int64_t granule, body, bytes;
  uint32_t serial, seq;
  const uint8_t *lace, *data;
};
inline bool demux_page_at(const uint8_t *f, int64_t n, int64_t pos, DemuxPage *pg) {
  if (n - pos < OGG_HEADER || memcmp(f + pos, "OggS", 4) != 0 || f[pos + 4] != 0) return false;
  pg->flags = f[pos + 5], pg->nseg = f[pos + 26];
  pg->granule = 0;
  for (int i = 0; i < 8; i++) pg->granule |= (int64_t)((uint64_t)f[pos + 6 + i] << (8 * i));
  pg->serial = ogg_le32(f + pos + 14), pg->seq = ogg_le32(f + pos + 18);
  if (n - pos - OGG_HEADER < pg->nseg) return false;
  pg->lace = f + pos + OGG_HEADER;
  pg->body = 0;
  for (int q = 0; q < pg->nseg; q++) pg->body += pg->lace[q];
  if (n - pos - OGG_HEADER - pg->nseg < pg->body) return false;
  pg->data = pg->lace + pg->nseg;
  pg->bytes = OGG_HEADER + pg->nseg + pg->body;
  return true;
}
// a begin-of-stream page whose first packet begins as a Vorbis identification header does
inline bool demux_page_is_vorbis(const DemuxPage &pg) { return pg.nseg > 0 && pg.lace[0] >= 7 && pg.data[0] == 1 && memcmp(pg.data + 1, "vorbis", 6) == 0; }

// One file under the follow policy.  The file is one or more LINKS.  A link opens with its begin-of-stream pages (the
// file's first page opens the first link with or without the flag, as the walk above takes it); its stream is the first
// of those whose first packet is a Vorbis identification header; a begin-of-stream page behind a page without the flag
// opens the next link, and the link in front ends there, with or without an end-of-stream page.  Pages of any other
// serial number are passed over: their headers are walked and their lengths held against the file, they get no page row
// and so no checksum.  Inside the link's stream the sequence numbers are consecutive from its first page's, the continued
// flag agrees with the open packet, and the link does not end inside a packet (BADPAGE); every link has a Vorbis stream
// whose three headers hold as a file's do above (BADHEADER).  Per audio packet out come, beside the above, the marks
// decode_plan_build_marked walks: the page's granule position on the last packet it completes (below -1: none), and the
// end-of-stream flag on that packet; and the packets at which the links behind the first begin.
struct DemuxLink {
  int64_t begin, end;
  uint32_t serial;  // the link's Vorbis stream, or its first page's where it has none
};
inline uint8_t demux_scan_file_links(const uint8_t *f, int64_t n, int64_t base, int stream, const DemuxSetup &S, DemuxScan *out) {
  const size_t packets0 = out->first.size(), pages0 = out->pages.size(), links0 = out->links.size();
  int64_t arena = out->offset.back(), pos = 0;
  uint8_t st = 0;
  bool bos_run = false, have = false, open = false, any = false;  // any: a link is open
  uint32_t serial = 0, next_seq = 0;
  int64_t npackets = 0, len = 0;
  std::vector<uint8_t> header[3];
  auto end_link = [&]() -> uint8_t {
    if (open) return VAMD_STATUS_BADPAGE;  // the link ends inside a packet
    if (!have || npackets < 3 || !demux_ident_ok(header[0].data(), (int64_t)header[0].size(), S)) return VAMD_STATUS_BADHEADER;
    if (ogg_comment_check(header[1].data(), (int64_t)header[1].size()) != OGG_COMMENT_OK) return VAMD_STATUS_BADHEADER;
    if (header[2].size() < 7 || header[2][0] != 5 || memcmp(header[2].data() + 1, "vorbis", 6) != 0) return VAMD_STATUS_BADHEADER;
    if (S.setup_header && ((int64_t)header[2].size() != S.setup_header_bytes || memcmp(header[2].data(), S.setup_header, header[2].size()) != 0))
      return VAMD_STATUS_BADHEADER;
    return 0;
  };
  while (pos < n && !st) {
    DemuxPage pg;
    if (!demux_page_at(f, n, pos, &pg)) {
      st = VAMD_STATUS_BADPAGE;
      break;
    }
    const bool bos = (pg.flags & 2) || pos == 0;
    if (bos && !bos_run) {  // the next link
      if (any && (st = end_link())) break;
      if (any) out->links.push_back((int64_t)out->first.size());
      any = true, bos_run = true, have = false, open = false, npackets = 0, len = 0;
      for (int k = 0; k < 3; k++) header[k].clear();
    }
    if (!bos) bos_run = false;
    if (bos && !have && demux_page_is_vorbis(pg)) have = true, serial = pg.serial, next_seq = pg.seq;
    else if (bos && have && pg.serial == serial) st = VAMD_STATUS_BADPAGE;  // the stream begins twice
    if (st) break;
    if (have && pg.serial == serial) {
      if (pg.seq != next_seq || (bool)(pg.flags & 1) != open) {
        st = VAMD_STATUS_BADPAGE;
        break;
      }
      next_seq++;
      int64_t at = 0, skip = 0, last = -1;
      for (int q = 0; q < pg.nseg; q++) {
        const int v = pg.lace[q];
        if (npackets < 3) {
          header[npackets].insert(header[npackets].end(), pg.data + at, pg.data + at + v);
          skip += v;
        } else if (!open) {
          out->first.push_back(v ? pg.data[at] : 0);
          out->granule.push_back(-1), out->eos.push_back(0);
        }
        open = true, len += v, at += v;
        if (v < 255) {
          if (npackets >= 3) out->offset.push_back(out->offset.back() + len), last = (int64_t)out->offset.size() - 2;
          npackets++, open = false, len = 0;
        }
      }
      if (last >= 0) out->granule[(size_t)last] = pg.granule < -1 ? -1 : pg.granule, out->eos[(size_t)last] = (pg.flags & 4) ? 1 : 0;
      OggDepage row;
      row.src = base + pos, row.dst = arena;
      row.nseg = pg.nseg, row.body = (int32_t)pg.body, row.skip = (int32_t)skip, row.stream = stream;
      out->pages.push_back(row);
      arena += pg.body - skip;
    }
    pos += pg.bytes;
  }
  if (!st) st = any ? end_link() : (uint8_t)VAMD_STATUS_BADHEADER;
  if (st) {
    out->first.resize(packets0), out->offset.resize(packets0 + 1), out->pages.resize(pages0), out->links.resize(links0);
  }
  out->granule.resize(out->first.size()), out->eos.resize(out->first.size());
  out->end_granule.push_back(-1);  // (the marks stand in its place)
  return st;
}

// A file's links (vamd_ogg_links): the page walk of demux_scan_file_links without its stream's rules -> false where a page
// header, a lacing table or a body does not hold against the file; the links begun up to there are listed then too, the
// last ending at the break.
inline bool demux_links(const uint8_t *f, int64_t n, std::vector<DemuxLink> *out) {
  out->clear();
  int64_t pos = 0;
  bool bos_run = false, have = false;
  while (pos < n) {
    DemuxPage pg;
    if (!demux_page_at(f, n, pos, &pg)) {
      if (!out->empty()) out->back().end = pos;
      return false;
    }
    const bool bos = (pg.flags & 2) || pos == 0;
    if (bos && !bos_run) {
      if (!out->empty()) out->back().end = pos;
      out->push_back({pos, n, pg.serial});
      bos_run = true, have = false;
    }
    if (!bos) bos_run = false;
    if (bos && !have && demux_page_is_vorbis(pg)) have = true, out->back().serial = pg.serial;
    pos += pg.bytes;
  }
  return true;
}

// The three header packets of a file's first logical stream (vamd_ogg_read_headers), or of its first stream of a given
// serial number (vamd_ogg_read_headers_serial): the walk above as far as the third
// packet's end, pages of another serial number passed over.  -> false where the pages do not hold three packets: a broken
// page header, a file that ends first.  Every length is held against what is left of the file before it is used.
inline bool demux_read_headers(const uint8_t *f, int64_t n, std::vector<uint8_t> header[3], const uint32_t *of_serial = nullptr) {
  int64_t pos = 0;
  int npackets = 0;
  uint32_t serial = of_serial ? *of_serial : 0;
  for (int64_t page = 0; npackets < 3; page++) {
    if (n - pos < OGG_HEADER || memcmp(f + pos, "OggS", 4) != 0 || f[pos + 4] != 0) return false;
    const int nseg = f[pos + 26];
    const uint32_t ser = ogg_le32(f + pos + 14);
    if (page == 0 && !of_serial) serial = ser;
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
inline bool demux_scan(int64_t nstreams, const uint8_t *bytes, const int64_t *file_offset, const DemuxSetup &S, DemuxScan *out, std::string *err,
                       bool follow = false) {
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
    out->status.push_back((follow ? demux_scan_file_links : demux_scan_file)(n ? bytes + o : nullptr, n, o - file_offset[0], (int)s, S, out));
    out->stream_start.push_back((int64_t)out->first.size());
    out->page_start.push_back((int64_t)out->pages.size());
  }
  return true;
}

}  // namespace vamd
