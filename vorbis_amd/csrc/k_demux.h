// k_demux.h -- Ogg pages back to audio packets, the device's half (the host's is vamd_demux.h): k_ogg_depage, a wave per
// page, over k_ogg.h's CRC (chunks per lane, the log-step join).  As with k_ogg.h the lanes' work is ONE body: the library
// compiles it for gfx950, the CPU suite compiles this very file with the host compiler and runs the lanes in turn
// (ogg_depage_host; tests/c/demux_host.cpp).
#pragma once
#include "k_ogg.h"

namespace vamd {

// A row of the page table the host's walk leaves.  The page lies at files[src ..]: 27 + nseg + body bytes.  Its first
// `skip` body bytes belong to the three header packets and go nowhere; the other body - skip go to arena[dst ..], the packed
// arena in which a stream's audio packets lie back to back (a page's audio bytes are one run there: lacing cuts packets
// into segments, it does not reorder them).
struct OggDepage {
  int64_t src, dst;
  int32_t nseg, body, skip, stream;
};
enum { OGG_DEPAGE_BADCRC = 32, OGG_DEPAGE_BADROW = 0x80 };  // a page's status byte: VAMD_STATUS_BADPAGE; a row outside the buffers (never seen)
// the row is trusted no further than the two buffers reach
VAMD_OGG_FN bool ogg_depage_inside(const OggDepage &pg, int64_t files_bytes, int64_t arena_bytes) {
  if (pg.nseg < 0 || pg.nseg > OGG_MAX_SEGS || pg.body < 0 || pg.body > OGG_MAX_SEGS * 255 || pg.skip < 0 || pg.skip > pg.body) return false;
  if (pg.src < 0 || pg.src > files_bytes || files_bytes - pg.src < OGG_HEADER + pg.nseg + pg.body) return false;
  return pg.dst >= 0 && pg.dst <= arena_bytes && arena_bytes - pg.dst >= pg.body - pg.skip;
}
VAMD_OGG_FN uint32_t ogg_load32(const uint8_t *aligned) {  // one aligned dword
  uint32_t w;
  memcpy(&w, __builtin_assume_aligned(aligned, 4), 4);
  return w;
}
VAMD_OGG_FN uint32_t ogg_alignbytes(uint32_t hi, uint32_t lo, unsigned sh) {  // bytes sh .. sh + 3 of lo | hi << 32 (v_alignbyte_b32)
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbyte(hi, lo, sh);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
#endif
}
// A lane's share of a page's checksum: bytes [lo, hi) of the page, the checksum field (bytes 22 .. 25) taken as zero.  The
// header's first 26 bytes and what lies in front of the first aligned dword go a byte at a time, the rest a dword at a time.
VAMD_OGG_FN uint32_t ogg_depage_crc(const uint32_t *table, const uint8_t *page, int64_t lo, int64_t hi) {
  uint32_t crc = 0;
  int64_t v = lo;
  for (; v < hi && (v < 26 || ((uintptr_t)(page + v) & 3)); v++) crc = ogg_crc_byte(table, crc, (uint64_t)(v - 22) < 4 ? 0u : page[v]);
  for (; v + 4 <= hi; v += 4) {
    const uint32_t w = ogg_load32(page + v);
    crc = ogg_crc_byte(table, crc, w & 0xffu);
    crc = ogg_crc_byte(table, crc, (w >> 8) & 0xffu);
    crc = ogg_crc_byte(table, crc, (w >> 16) & 0xffu);
    crc = ogg_crc_byte(table, crc, w >> 24);
  }
  for (; v < hi; v++) crc = ogg_crc_byte(table, crc, page[v]);
  return crc;
}
// A lane's share of a page's copy: n bytes from src to dst, both at any byte offset.  The dwords of the destination that
// the run covers whole are written as aligned dwords, each out of two aligned dwords of the source joined by alignbyte
// (the second holds at least one byte of the run, so no read goes past the dword the run's last byte lies in); the up to
// three bytes in front of and behind them share their dwords with the neighbouring pages' runs and are written as bytes,
// so no dword is read, changed and written back by two waves.
VAMD_OGG_FN void ogg_depage_copy(const uint8_t *src, uint8_t *dst, int64_t n, int lane, int lanes) {
  int64_t head = (int64_t)(-(uintptr_t)dst & 3);
  if (head > n) head = n;
  const int64_t words = (n - head) >> 2, tail0 = head + 4 * words;
  for (int64_t i = lane; i < head; i += lanes) dst[i] = src[i];
  for (int64_t i = tail0 + lane; i < n; i += lanes) dst[i] = src[i];
  const unsigned sh = (unsigned)((uintptr_t)(src + head) & 3);
  const uint8_t *wp = src + head - sh;
  uint32_t *wd = (uint32_t *)__builtin_assume_aligned(dst + head, 4);
  for (int64_t i = lane; i < words; i += lanes) wd[i] = ogg_alignbytes(sh ? ogg_load32(wp + 4 * i + 4) : 0u, ogg_load32(wp + 4 * i), sh);
}

// A row of the live Ogg decoder's two byte-carry tables (vamd_demux_live.h): the audio packet a stream's whole pages have
// left open lies in the slot's row of the carry, [slots][stride] bytes with stride a multiple of 4, so every row begins
// on a dword.  `len` bytes of it are, or go to, arena[at ..].
struct OggCarryRow {
  int64_t at;
  int32_t slot, len;
};
// the row is trusted no further than the two buffers reach
VAMD_OGG_FN bool ogg_carry_inside(const OggCarryRow &r, int64_t arena_bytes, int64_t slots, int64_t stride) {
  if (stride < 0 || (stride & 3) || r.slot < 0 || r.slot >= slots || r.len < 0 || r.len > stride) return false;
  return r.at >= 0 && r.at <= arena_bytes && arena_bytes - r.at >= r.len;
}
// A lane's share of a row, one body for both directions: in, the carried bytes to the front of the stream's region of the
// arena; out, the open packet's bytes at the end of that region back to the slot's row.  ogg_depage_copy's guarantee
// holds: a carry row begins on a dword and belongs to one wave, so its whole dwords and its last bytes are that wave's; in
// the arena the up to three bytes at either edge share their dwords with the neighbouring runs and are written as bytes.
VAMD_OGG_FN void ogg_packet_carry(bool out, const OggCarryRow &r, uint8_t *arena, uint8_t *carry, int64_t stride, int lane, int lanes) {
  uint8_t *row = carry + (int64_t)r.slot * stride;
  if (out) ogg_depage_copy(arena + r.at, row, r.len, lane, lanes);
  else ogg_depage_copy(row, arena + r.at, r.len, lane, lanes);
}

#if defined(__HIPCC__)
// The live Ogg decoder's byte carries, a wave per row, around k_ogg_depage on the context's stream:
//   k_ogg_packet_carry_in   carry[slot] -> arena[at ..]   the bytes of the packet the slot's earlier pages left open
//   k_ogg_depage                                          this call's whole pages behind them
//   k_ogg_packet_carry_out  arena[at ..] -> carry[slot]   the bytes of the packet still open behind this call's pages
// A packet open across a whole piece goes carry -> arena -> carry, its new bytes joined to the old ones in the arena.
// The three launches are on one stream, so each sees what the one before it wrote: carry_out reads bytes that carry_in and
// k_ogg_depage have written, and writes a row that carry_in (the only reader of the carry in a call) has already read.
// Inside one launch no two rows name the same slot or overlapping runs of the arena (the host's walk lays them out).
__global__ __launch_bounds__(64) void k_ogg_packet_carry_in(const OggCarryRow *__restrict__ rows, uint8_t *arena, int64_t arena_bytes, uint8_t *carry,
                                                            int64_t slots, int64_t stride) {
  const OggCarryRow r = rows[blockIdx.x];
  if (ogg_carry_inside(r, arena_bytes, slots, stride)) ogg_packet_carry(false, r, arena, carry, stride, threadIdx.x, 64);
}
__global__ __launch_bounds__(64) void k_ogg_packet_carry_out(const OggCarryRow *__restrict__ rows, uint8_t *arena, int64_t arena_bytes, uint8_t *carry,
                                                             int64_t slots, int64_t stride) {
  const OggCarryRow r = rows[blockIdx.x];
  if (ogg_carry_inside(r, arena_bytes, slots, stride)) ogg_packet_carry(true, r, arena, carry, stride, threadIdx.x, 64);
}

// A wave per row of the page table (vamd_demux.h), files as they lay in host memory: the page's checksum -- every lane its
// chunk (ogg_crc_range over header + lacing + body), the tree's six steps, the table in LDS -- against the stored field,
// BADCRC into the page's status byte where they differ; and the page's audio bytes to their place in the packed arena
// (ogg_depage_copy).  A page of header packets alone, or with no segment, is summed and copies nothing.  Pages are 27 to
// 65 307 bytes: a chunk is 16 bytes to 1021.
__global__ __launch_bounds__(64) void k_ogg_depage(const uint8_t *__restrict__ files, int64_t files_bytes, const OggDepage *__restrict__ pages,
                                                   uint8_t *__restrict__ arena, int64_t arena_bytes, uint8_t *__restrict__ page_status) {
  __shared__ uint32_t table[256];
  const int lane = threadIdx.x;
  const OggDepage pg = pages[blockIdx.x];
  if (!ogg_depage_inside(pg, files_bytes, arena_bytes)) {
    if (lane == 0) page_status[blockIdx.x] = OGG_DEPAGE_BADROW;
    return;
  }
  for (int e = lane; e < 256; e += 64) table[e] = ogg_crc_entry((uint32_t)e);
  __syncthreads();
  const uint8_t *page = files + pg.src;
  const int64_t hlen = OGG_HEADER + pg.nseg, len = hlen + pg.body;
  const int64_t c = ogg_crc_chunk(len, OGG_CRC_LANES, OGG_CRC_MIN_CHUNK);
  int64_t lo, hi;
  ogg_crc_range(len, OGG_CRC_LANES, c, lane, &lo, &hi);
  uint32_t crc = ogg_depage_crc(table, page, lo, hi);
  uint32_t m = ogg_crc_xpow8(c);
  for (int d = 1; d < OGG_CRC_LANES; d <<= 1) {
    const uint32_t right = (uint32_t)__shfl_down((int)crc, d, 64);
    crc = ogg_crc_join(crc, right, m);
    m = ogg_crc_mul(m, m);
  }
  if (lane == 0) page_status[blockIdx.x] = crc == ogg_le32(page + 22) ? 0 : OGG_DEPAGE_BADCRC;
  if (pg.body > pg.skip) ogg_depage_copy(page + hlen + pg.skip, arena + pg.dst, pg.body - pg.skip, lane, 64);
}
#endif  // __HIPCC__

#if !defined(__HIP_DEVICE_COMPILE__)
// k_ogg_depage's work on one page, the lanes in turn (tests/c/demux_host.cpp) -> the page's status byte
inline uint8_t ogg_depage_host(const uint8_t *files, int64_t files_bytes, const OggDepage &pg, uint8_t *arena, int64_t arena_bytes, int lanes) {
  if (!ogg_depage_inside(pg, files_bytes, arena_bytes)) return OGG_DEPAGE_BADROW;
  uint32_t table[256], part[64], next[64];
  for (int e = 0; e < 256; e++) table[e] = ogg_crc_entry((uint32_t)e);
  if (lanes > 64) lanes = 64;
  const uint8_t *page = files + pg.src;
  const int64_t hlen = OGG_HEADER + pg.nseg, len = hlen + pg.body;
  const int64_t c = ogg_crc_chunk(len, lanes, OGG_CRC_MIN_CHUNK);
  for (int l = 0; l < lanes; l++) {
    int64_t lo, hi;
    ogg_crc_range(len, lanes, c, l, &lo, &hi);
    part[l] = ogg_depage_crc(table, page, lo, hi);
  }
  uint32_t m = ogg_crc_xpow8(c);
  for (int d = 1; d < lanes; d <<= 1) {
    for (int l = 0; l < lanes; l++) next[l] = ogg_crc_join(part[l], l + d < lanes ? part[l + d] : part[l], m);
    memcpy(part, next, sizeof(part));
    m = ogg_crc_mul(m, m);
  }
  for (int l = 0; l < lanes && pg.body > pg.skip; l++) ogg_depage_copy(page + hlen + pg.skip, arena + pg.dst, pg.body - pg.skip, l, lanes);
  return part[0] == ogg_le32(page + 22) ? 0 : OGG_DEPAGE_BADCRC;
}
// k_ogg_packet_carry_in's (out = false) or _out's work on one row, the lanes in turn (tests/c/demux_live_host.cpp) -> false
// for a row outside the buffers, which is left alone
inline bool ogg_packet_carry_host(bool out, const OggCarryRow &r, uint8_t *arena, int64_t arena_bytes, uint8_t *carry, int64_t slots, int64_t stride,
                                  int lanes) {
  if (!ogg_carry_inside(r, arena_bytes, slots, stride)) return false;
  for (int l = 0; l < lanes; l++) ogg_packet_carry(out, r, arena, carry, stride, l, lanes);
  return true;
}
#endif

}  // namespace vamd
