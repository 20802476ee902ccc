// k_feed_src.h -- the source side of a DEVICE-fed group of the feed (vamd_feed_wrote_device, include/vorbis_amd.h): samples
// that already lie in HBM as a caller's tensors -- one base pointer per stream, two strides in elements, four element types.
// Three parts, ONE body each for the library (gfx950) and for the CPU suite, which compiles this very file with the host
// compiler (tests/feed_source_host.py), as k_ogg.h is:
//   * the conversion of an element to the float the encoder sees (src_float) -- integer arithmetic on the bits only, so that
//     no mode register (denormal flushing, rounding) that a CPU test cannot see has a say in it;
//   * four frames of one channel row (src_quad): one vector load where the frames are consecutive and the quad's address is
//     aligned to its size, element loads otherwise -- and a whole stream's buffer from them (feed_ingest_dev_item: what a
//     thread of k_feed_ingest_dev does, k_feed.h);
//   * the range check the host makes before anything is enqueued (source_extent): a bad stride is an error code, never a fault.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define VAMD_HOSTDEV __host__ __device__ inline
#else
#define VAMD_HOSTDEV inline
#endif

namespace vamd {

// the element types (VAMD_SRC_*: their values); a 16-bit float travels as its bits
enum { SRC_S16 = 0, SRC_F32 = 1, SRC_F16 = 2, SRC_BF16 = 3, SRC_TYPES = 4 };
struct src_f16 {
  uint16_t bits;
};
struct src_bf16 {
  uint16_t bits;
};
VAMD_HOSTDEV int src_elem_bytes(int dtype) { return dtype == SRC_F32 ? 4 : 2; }

VAMD_HOSTDEV float src_from_bits(uint32_t u) {
  float f;
  memcpy(&f, &u, 4);
  return f;
}
VAMD_HOSTDEV uint32_t src_to_bits(float f) {
  uint32_t u;
  memcpy(&u, &f, 4);
  return u;
}

VAMD_HOSTDEV float src_float(int16_t x) { return (float)(int)x / 32768.f; }  // examples/encoder_example.c:197-202
VAMD_HOSTDEV float src_float(float x) { return x; }
VAMD_HOSTDEV float src_float(src_bf16 x) { return src_from_bits((uint32_t)x.bits << 16); }
// binary16 -> binary32, exact: every binary16 value is a binary32 value.  A subnormal m * 2^-24 is normalised by the place p
// of its leading one (2^(p - 24) * 1.xxx); Inf and NaN keep their class, a NaN its payload.
VAMD_HOSTDEV float src_float(src_f16 x) {
  const uint32_t h = x.bits, sign = (h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 0x3ffu;
  uint32_t u;
  if (e == 31u) u = sign | 0x7f800000u | (m << 13);
  else if (e) u = sign | ((e + 112u) << 23) | (m << 13);
  else if (!m) u = sign;
  else {
    const uint32_t p = 31u - (uint32_t)__builtin_clz(m);  // 0 .. 9
    u = sign | ((p + 103u) << 23) | ((m << (23u - p)) & 0x7fffffu);
  }
  return src_from_bits(u);
}
template <typename T>
VAMD_HOSTDEV constexpr bool src_has_non_finite() { return true; }
template <>
VAMD_HOSTDEV constexpr bool src_has_non_finite<int16_t>() { return false; }
VAMD_HOSTDEV bool src_non_finite(float x) { return (src_to_bits(x) & 0x7f800000u) == 0x7f800000u; }

// what one vector load brings: four elements of 4 or of 2 bytes
struct alignas(16) SrcVec16 {
  uint32_t w[4];
};
struct alignas(8) SrcVec8 {
  uint16_t h[4];
};
// ... and the one 16-byte store of a thread per channel (the stream buffers' quads are aligned to it)
struct alignas(16) SrcOut {
  float v[4];
};
VAMD_HOSTDEV void src_store4(float *d, float a, float b, float c, float e) { *(SrcOut *)d = SrcOut{{a, b, c, e}}; }
template <typename T>
VAMD_HOSTDEV T src_of_bits16(uint16_t b);
template <>
VAMD_HOSTDEV int16_t src_of_bits16<int16_t>(uint16_t b) { return (int16_t)b; }
template <>
VAMD_HOSTDEV src_f16 src_of_bits16<src_f16>(uint16_t b) { return src_f16{b}; }
template <>
VAMD_HOSTDEV src_bf16 src_of_bits16<src_bf16>(uint16_t b) { return src_bf16{b}; }

// whether four consecutive elements from p on may come in one load
template <typename T>
VAMD_HOSTDEV bool src_quad_aligned(const T *p) { return ((uintptr_t)p & (4 * sizeof(T) - 1)) == 0; }

template <typename T>
VAMD_HOSTDEV void src_quad_vec(const T *p, float v[4]) {  // (the 16-bit types)
  const SrcVec8 q = *(const SrcVec8 *)p;
  for (int k = 0; k < 4; k++) v[k] = src_float(src_of_bits16<T>(q.h[k]));
}
template <>
VAMD_HOSTDEV void src_quad_vec<float>(const float *p, float v[4]) {
  const SrcVec16 q = *(const SrcVec16 *)p;
  for (int k = 0; k < 4; k++) v[k] = src_from_bits(q.w[k]);
}

// frames f0 .. f0 + 3 of the channel row that begins at `row` (element (c, 0) of the stream), of which the first `live` exist
// (the others: 0.f, and nothing of them is read); fs: the frame stride in elements.  vec_ok false: element loads whatever
// the address (the CPU suite holds the two paths together).
template <typename T>
VAMD_HOSTDEV void src_quad(const T *row, int64_t f0, int64_t fs, int live, bool vec_ok, float v[4]) {
  const T *p = row + f0 * fs;
  if (vec_ok && live == 4 && fs == 1 && src_quad_aligned(p)) {
    src_quad_vec(p, v);
    return;
  }
  for (int k = 0; k < 4; k++) v[k] = k < live ? src_float(p[(int64_t)k * fs]) : 0.f;
}

// One thread's share of a whole-stream group's ingest (k_feed_ingest_dev), item t of nstreams * (head / 4 + quads + pad / 4):
// stream s = its base pointer base_of[s] and frames_of[s] <= frames frames, element (c, k) at base + c * cstride + k * fstride,
// -> pcm[s * ss + c * cs + head + k]; the room in front (head samples) and behind (the rest of the quads laid out for
// `frames`, and pad samples) zeroed, as k_feed_ingest leaves it; amp[s] = the ampmax chain's floor.
template <typename T>
VAMD_HOSTDEV void feed_ingest_dev_item(long t, int ch, long frames, int head, int pad, float *pcm, long ss, long cs, float *amp, float amp_floor,
                                       const long long *frames_of, const long long *base_of, int64_t cstride, int64_t fstride, bool vec_ok) {
  const long quads = (frames + 3) >> 2, hq = head >> 2, pq = pad >> 2, per = hq + quads + pq;
  const long s = t / per, q = t - s * per;
  float *row = pcm + s * ss;
  if (q < hq) {
    for (int c = 0; c < ch; c++) src_store4(row + (long)c * cs + 4 * q, 0.f, 0.f, 0.f, 0.f);
    if (q == 0) amp[s] = amp_floor;
  } else if (q < hq + quads) {
    const long mine = (long)frames_of[s], f0 = (q - hq) << 2;
    const int live = mine - f0 < 4 ? (mine > f0 ? (int)(mine - f0) : 0) : 4;
    const T *base = (const T *)(uintptr_t)base_of[s];
    for (int c = 0; c < ch; c++) {
      float v[4] = {0.f, 0.f, 0.f, 0.f};
      if (live) src_quad(base + (int64_t)c * cstride, (int64_t)f0, fstride, live, vec_ok, v);
      src_store4(row + (long)c * cs + head + f0, v[0], v[1], v[2], v[3]);
    }
  } else {
    const long f0 = (quads << 2) + ((q - hq - quads) << 2);
    for (int c = 0; c < ch; c++) src_store4(row + (long)c * cs + head + f0, 0.f, 0.f, 0.f, 0.f);
  }
}

// The elements a stream of `frames` frames in `ch` channels reads, relative to its base pointer: [*lo, *hi) is the minimum
// and the maximum of c * cstride + k * fstride over c < ch, k < frames, plus one (frames == 0: empty, lo == hi == 0).  Then, in
// bytes, against the allocation the base pointer lies in: `offset` bytes behind its start, `alloc_bytes` long.
// -> 0: every read lies inside; 1: the extent does not fit 64-bit arithmetic; 2: it begins before the allocation; 3: it ends
// behind it.  Pure host arithmetic, every product and sum checked.
inline int source_extent(int ch, int64_t frames, int64_t cstride, int64_t fstride, int elem_bytes, int64_t offset, int64_t alloc_bytes,
                         int64_t *lo, int64_t *hi) {
  int64_t a = 0, b = 0, l = 0, h = 0;
  if (lo) *lo = 0;
  if (hi) *hi = 0;
  if (ch < 1 || frames < 0 || elem_bytes < 1 || offset < 0 || alloc_bytes < 0) return 1;
  if (frames == 0) return offset <= alloc_bytes ? 0 : 3;
  if (__builtin_mul_overflow((int64_t)(ch - 1), cstride, &a) || __builtin_mul_overflow(frames - 1, fstride, &b)) return 1;
  if (__builtin_add_overflow(a < 0 ? a : 0, b < 0 ? b : 0, &l) || __builtin_add_overflow(a > 0 ? a : 0, b > 0 ? b : 0, &h) ||
      __builtin_add_overflow(h, (int64_t)1, &h))
    return 1;
  if (lo) *lo = l;
  if (hi) *hi = h;
  int64_t lb = 0, hb = 0;
  if (__builtin_mul_overflow(l, (int64_t)elem_bytes, &lb) || __builtin_mul_overflow(h, (int64_t)elem_bytes, &hb) ||
      __builtin_add_overflow(lb, offset, &lb) || __builtin_add_overflow(hb, offset, &hb))
    return 1;
  if (lb < 0) return 2;
  if (hb > alloc_bytes) return 3;
  return 0;
}

}  // namespace vamd
