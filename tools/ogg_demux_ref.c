/* tools/ogg_demux_ref.c -- what a caller of vamd_decode_streams has to run in front of it today (tools/decode_ogg_bench.py
 * compiles it -O2 and times it): one Ogg Vorbis file to its audio packets on the host, from doc/framing.html -- the page
 * walk, the byte-serial table CRC over every page, and every packet's bytes gathered into one contiguous buffer.  A plain
 * reader of well-formed single streams: anything else ends it with -1. */
#include <stdint.h>
#include <string.h>

static uint32_t table[256];

static void init(void) {
  for (uint32_t i = 0; i < 256; i++) {
    uint32_t r = i << 24;
    for (int k = 0; k < 8; k++) r = (r & 0x80000000u) ? (r << 1) ^ 0x04c11db7u : r << 1;
    table[i] = r;
  }
}

static uint32_t crc_run(uint32_t crc, const uint8_t *p, long n) {
  for (long i = 0; i < n; i++) crc = (crc << 8) ^ table[(crc >> 24) ^ p[i]];
  return crc;
}

/* -> the audio packets (the three headers skipped) back to back in out[], their sizes in sizes[], *end_granule the granule
 * position of the page that completes the last of them; returns their number, or -1 */
long ogg_demux_ref(const uint8_t *f, long n, uint8_t *out, long out_cap, long *sizes, long cap, long long *end_granule) {
  static const uint8_t zero[4] = {0, 0, 0, 0};
  long pos = 0, npackets = 0, at = 0, len = 0, seq = 0;
  int open = 0;
  uint32_t serial = 0;
  if (!table[1]) init();
  *end_granule = -1;
  while (pos < n) {
    if (n - pos < 27 || memcmp(f + pos, "OggS", 4) != 0 || f[pos + 4] != 0) return -1;
    const int nseg = f[pos + 26];
    if (n - pos - 27 < nseg) return -1;
    long body = 0;
    for (int q = 0; q < nseg; q++) body += f[pos + 27 + q];
    if (n - pos - 27 - nseg < body) return -1;
    uint32_t stored, ser, sq;
    long long gp;
    memcpy(&gp, f + pos + 6, 8), memcpy(&ser, f + pos + 14, 4), memcpy(&sq, f + pos + 18, 4), memcpy(&stored, f + pos + 22, 4);
    uint32_t crc = crc_run(0, f + pos, 22);
    crc = crc_run(crc, zero, 4);
    crc = crc_run(crc, f + pos + 26, 1 + nseg + body);
    if (crc != stored) return -1;
    if (seq == 0) serial = ser;
    if (ser != serial || sq != (uint32_t)seq || ((f[pos + 5] & 1) != 0) != open) return -1;
    const uint8_t *data = f + pos + 27 + nseg;
    int done = 0;
    for (int q = 0; q < nseg; q++) {
      const int v = f[pos + 27 + q];
      if (npackets >= 3) {
        if (at + v > out_cap) return -1;
        memcpy(out + at, data, (size_t)v);
        at += v;
      }
      data += v, len += v, open = 1;
      if (v < 255) {
        if (npackets >= 3) {
          if (npackets - 3 >= cap) return -1;
          sizes[npackets - 3] = len, done = 1;
        }
        npackets++, len = 0, open = 0;
      }
    }
    if (done) *end_granule = gp;
    pos += 27 + nseg + body, seq++;
  }
  return open || npackets < 3 ? -1 : npackets - 3;
}
