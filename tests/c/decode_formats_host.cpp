// tests/c/decode_formats_host.cpp -- TEST BUILD ONLY (tests/test_decode_formats_cpu.py; built with -fsanitize=address,undefined).
// The output formats of vorbis_amd/csrc/k_synth.h ("the lap in the caller's format") compiled for one lane on the host
// (tests/emul/vamd_wave_host.h): the conversion helpers over a table, and lap_window_as / lap_row in every instantiation
// over one stream, every thread of the launch in turn.
//   decode_formats_host convert in out   in: float [n]     out: int16 s16[n] | uint16 f16[n] | uint16 bf16[n]
//   decode_formats_host lap job out      job: int32 ch, bs0, bs1, nblocks, ncases | int32 cases[ncases][4] = (start, frames,
//                                             offset, pad) | float win0[bs0/2], win1[bs1/2] | per block in stream order:
//                                             int32 W, float pcm[ch][bs[W]]
//                                        out: per dtype 0..3, per layout planar / interleaved, per case: the whole buffer,
//                                             GUARD + offset elements | the region | GUARD elements, every byte 0xA5 before
//                                             the run.  The region is ch rows of frames + pad elements (planar: the window
//                                             form, stride = frames + pad) or frames * ch elements (interleaved).
// <F32, planar> is the shipped lap_window, four frames a thread, as k_lap_window runs it.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "vamd_bind.h"
#include "k_synth.h"

using namespace vamd;

static const int GUARD = 16;

static std::vector<unsigned char> slurp(const char *path) {
  std::vector<unsigned char> v;
  FILE *f = fopen(path, "rb");
  if (!f) {
    printf("cannot open %s\n", path);
    exit(2);
  }
  unsigned char buf[65536];
  for (size_t k; (k = fread(buf, 1, sizeof(buf), f)) > 0;) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

struct Reader {
  const std::vector<unsigned char> &v;
  size_t at = 0;
  explicit Reader(const std::vector<unsigned char> &v_) : v(v_) {}
  template <class T>
  std::vector<T> take(size_t count) {
    if (at + count * sizeof(T) > v.size()) {
      printf("job file truncated\n");
      exit(2);
    }
    std::vector<T> o(count);
    if (count) memcpy(o.data(), v.data() + at, count * sizeof(T));
    at += count * sizeof(T);
    return o;
  }
  int i32() { return take<int32_t>(1)[0]; }
};

static void put(FILE *f, const void *p, size_t bytes) {
  if (bytes && fwrite(p, 1, bytes, f) != bytes) {
    printf("cannot write\n");
    exit(2);
  }
}

static int run_convert(const char *in, const char *outpath) {
  const std::vector<unsigned char> raw = slurp(in);
  Reader r(raw);
  const size_t n = raw.size() / 4;
  const std::vector<float> x = r.take<float>(n);
  std::vector<int16_t> s(n);
  std::vector<uint16_t> h(n), b(n);
  for (size_t k = 0; k < n; k++) s[k] = pcm_from<1>(x[k]), h[k] = pcm_from<2>(x[k]), b[k] = pcm_from<3>(x[k]);
  FILE *f = fopen(outpath, "wb");
  if (!f) return printf("cannot write %s\n", outpath), 2;
  put(f, s.data(), 2 * n), put(f, h.data(), 2 * n), put(f, b.data(), 2 * n);
  fclose(f);
  return 0;
}

struct Case {
  int start, frames, offset, pad;
};

// one case in one format: the buffer, exactly as large as the layout says (so a store past it is the sanitiser's), every
// thread the launch would have and two more
template <int D, bool IL>
static void run_case(const LapP &L, long long k0, long long k1, const Case &c, FILE *f) {
  typedef typename PcmElem<D>::T T;
  const long long stride = c.frames + c.pad, region = IL ? (long long)c.frames * L.ch : (long long)L.ch * stride;
  const size_t total = (size_t)(GUARD + c.offset + region + GUARD), bytes = (total * sizeof(T) + 15) & ~(size_t)15;
  T *buf = (T *)aligned_alloc(16, bytes);
  memset(buf, 0xA5, bytes);
  T *out = buf + GUARD + c.offset;
  const long long a = lap_centre(L, k0) + c.start;
  if (D == 0 && !IL) {
    for (long long q = 0; 4 * q < c.frames + 8; q++) lap_window(L, k0, k1, a, c.frames, stride, q, (float *)out);
  } else {
    const long long nq = lap_threads_as<D, IL>(c.frames, L.ch);
    for (long long q = 0; q < nq + 2; q++) lap_window_as<D, IL>(L, k0, k1, a, c.frames, stride, q, out);
  }
  put(f, buf, total * sizeof(T));
  free(buf);
}

template <int D>
static void run_dtype(const LapP &L, long long k0, long long k1, const std::vector<Case> &cases, FILE *f) {
  for (const Case &c : cases) run_case<D, false>(L, k0, k1, c, f);
  for (const Case &c : cases) run_case<D, true>(L, k0, k1, c, f);
}

static int run_lap(const char *job, const char *outpath) {
  const std::vector<unsigned char> raw = slurp(job);
  Reader r(raw);
  LapP L;
  memset(&L, 0, sizeof(L));
  L.ch = r.i32(), L.bs0 = r.i32(), L.bs1 = r.i32();
  const int nblocks = r.i32(), ncases = r.i32();
  const std::vector<int32_t> rows = r.take<int32_t>((size_t)ncases * 4);
  const std::vector<float> win0 = r.take<float>((size_t)L.bs0 / 2), win1 = r.take<float>((size_t)L.bs1 / 2);
  std::vector<int> order;
  std::vector<long long> src[2], start = {0, nblocks};
  std::vector<float> synth[2];
  long long at = 0;
  int prev = 0;
  for (int k = 0; k < nblocks; k++) {
    const int W = r.i32(), n = W ? L.bs1 : L.bs0;
    const std::vector<float> pcm = r.take<float>((size_t)L.ch * n);
    order.push_back((W << 30) | (int)(synth[W].size() / ((size_t)L.ch * n)));
    synth[W].insert(synth[W].end(), pcm.begin(), pcm.end());
    if (k) at += prev / 4 + n / 4;
    src[W].push_back(at - n / 2);
    prev = n;
  }
  synth[0].shrink_to_fit(), synth[1].shrink_to_fit();
  L.win0 = win0.data(), L.win1 = win1.data(), L.order = order.data(), L.stream_start = start.data(), L.src0 = src[0].data(), L.src1 = src[1].data();
  L.synth0 = synth[0].data(), L.synth1 = synth[1].data();
  std::vector<Case> cases;
  for (int k = 0; k < ncases; k++) {
    const Case c = {rows[4 * k], rows[4 * k + 1], rows[4 * k + 2], rows[4 * k + 3]};
    if (nblocks < 2 || c.start < 0 || c.frames < 0 || c.offset < 0 || c.pad < 0 || c.start + (long long)c.frames > at) return printf("lap: case %d outside the %lld frames\n", k, at), 2;
    cases.push_back(c);
  }
  FILE *f = fopen(outpath, "wb");
  if (!f) return printf("cannot write %s\n", outpath), 2;
  run_dtype<0>(L, 0, nblocks, cases, f);
  run_dtype<1>(L, 0, nblocks, cases, f);
  run_dtype<2>(L, 0, nblocks, cases, f);
  run_dtype<3>(L, 0, nblocks, cases, f);
  fclose(f);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 4 && !strcmp(argv[1], "convert")) return run_convert(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "lap")) return run_lap(argv[2], argv[3]);
  printf("usage: decode_formats_host convert in out | lap job out\n");
  return 2;
}
