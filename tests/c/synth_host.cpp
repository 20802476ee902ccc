// tests/c/synth_host.cpp -- TEST BUILD ONLY (tests/test_synth_cpu.py; built with -fsanitize=address,undefined).
// The bodies of vorbis_amd/csrc/k_synth.h -- mdct_backward_wave, synth_block, lap_find / lap_sample -- compiled for one
// lane on the host (tests/emul/vamd_wave_host.h) and run over jobs the test writes; the test holds the results against the
// reference decoder.  Every buffer has exactly the size the GPU launch gives it, so that a read or write beyond one is
// the sanitiser's to report.
//   synth_host mdct  job out          job: int32 n | float trig[n + n/4] | float in[n/2]                 out: float [n]
//   synth_host block setup job out    job: int32 nblocks | per block: int32 W, post_valid[ch], ilogmask[ch][n2],
//                                          res_class[submaps][VAMD_RES_CLASS_STRIDE], res_count[submaps][2],
//                                          uint16 res_entries[res_cap rounded up to even]            out: float [ch][n] each
//   synth_host lap   job out          job: int32 ch, bs0, bs1, nblocks, frames | float win0[bs0/2], win1[bs1/2] |
//                                          per block in stream order: int32 W, float pcm[ch][bs[W]]     out: float [ch][frames]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "vamd_bind.h"
#include "k_synth.h"

using namespace vamd;

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

static void spill(const char *path, const std::vector<float> &v) {
  FILE *f = fopen(path, "wb");
  if (!f || fwrite(v.data(), 4, v.size(), f) != v.size()) {
    printf("cannot write %s\n", path);
    exit(2);
  }
  fclose(f);
}

struct Reader {
  const std::vector<unsigned char> &v;
  size_t at = 0;
  explicit Reader(const std::vector<unsigned char> &v_) : v(v_) {}
  template <class T>
  std::vector<T> take(size_t count) {  // (a copy of its own: exactly `count` elements, aligned for its type)
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

// 16-byte aligned floats, as LDS and the setup image are
struct AlignedFloats {
  float *p;
  size_t n;
  explicit AlignedFloats(size_t count) : n(count) {
    p = (float *)aligned_alloc(16, (count * 4 + 15) & ~(size_t)15);  // (every count here is a whole number of quads)
    memset(p, 0, count * 4);
  }
  ~AlignedFloats() { free(p); }
};

static int run_mdct(const char *job, const char *outpath) {
  const std::vector<unsigned char> raw = slurp(job);
  Reader r(raw);
  const int n = r.i32();
  int log2n = 0;
  while ((1 << log2n) < n) log2n++;
  if (n < 64 || n > 8192 || (1 << log2n) != n) return printf("mdct: bad n\n"), 2;
  const std::vector<float> trig = r.take<float>((size_t)n + n / 4), in = r.take<float>((size_t)n / 2);
  AlignedFloats T(trig.size()), I(in.size()), W2(VAMD_SY_W2_FLOATS(n / 2));
  memcpy(T.p, trig.data(), trig.size() * 4);
  memcpy(I.p, in.data(), in.size() * 4);
  XformP P;
  memset(&P, 0, sizeof(P));
  P.n = n, P.log2n = log2n, P.mdct_scale = 4.f / n, P.trig = T.p, P.bitrev_std = 1;
  std::vector<float> out((size_t)n);
  PhaseClock pc;
  pc.start(nullptr);
  mdct_backward_wave(P, I.p, W2.p, out.data(), pc);
  spill(outpath, out);
  return 0;
}

static int run_block(const char *setup, const char *job, const char *outpath) {
  const std::vector<unsigned char> blob = slurp(setup), raw = slurp(job);
  std::vector<unsigned char> image;
  std::vector<uint32_t> doff;
  std::vector<PsyDerived> derived;
  std::string err;
  Bound B;
  if (build_image(blob.data(), blob.size(), &image, &doff, &derived, &err) != VAMD_OK) return printf("setup: %s\n", err.c_str()), 2;
  bind_params(image, doff, derived, image.data(), &B);
  Reader r(raw);
  const int nblocks = r.i32(), ch = B.channels;
  std::vector<float> all;
  for (int b = 0; b < nblocks; b++) {
    const int W = r.i32();
    if ((W != 0 && W != 1) || !B.res_cap[W]) return printf("block %d: size class %d has no covered residue\n", b, W), 2;
    const int n = B.bs[W], n2 = n / 2, S_ = B.chmap[W].submaps;
    const std::vector<int32_t> post_valid = r.take<int32_t>((size_t)ch), ilog32 = r.take<int32_t>((size_t)ch * n2),
                               res_class = r.take<int32_t>((size_t)S_ * VAMD_RES_CLASS_STRIDE), res_count = r.take<int32_t>((size_t)2 * S_);
    std::vector<uint16_t> res_entries = r.take<uint16_t>((size_t)((B.res_cap[W] + 1) & ~1));
    res_entries.resize((size_t)B.res_cap[W]);
    res_entries.shrink_to_fit();
    std::vector<ilog_t> ilog(ilog32.size());
    for (size_t k = 0; k < ilog.size(); k++) ilog[k] = (ilog_t)ilog32[k];
    SynthFloorP S;
    if (!synth_floor_ranges(B.floor[W][0], B.floor[W][1], S_, n2, &S)) return printf("block %d: a floor the decoder's way is not drawn\n", b), 2;
    AlignedFloats lds(synth_lds_words(ch, n2, 1, B.res_off_ints[W]));
    std::vector<float> out((size_t)ch * n);
    PhaseClock pc;
    pc.start(nullptr);
    synth_block(B.xf[W], B.res[W][0], B.res[W][1], B.chmap[W], B.couple[W], S, ch, B.res_off_ints[W], post_valid.data(), ilog.data(),
                res_class.data(), res_entries.data(), res_count.data(), lds.p, out.data(), pc);
    all.insert(all.end(), out.begin(), out.end());
  }
  spill(outpath, all);
  return 0;
}

static int run_lap(const char *job, const char *outpath) {
  const std::vector<unsigned char> raw = slurp(job);
  Reader r(raw);
  LapP L;
  memset(&L, 0, sizeof(L));
  L.ch = r.i32(), L.bs0 = r.i32(), L.bs1 = r.i32();
  const int nblocks = r.i32(), frames = r.i32();
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
    src[W].push_back(at - n / 2);  // (a block begins half its size before its centre)
    prev = n;
  }
  synth[0].shrink_to_fit(), synth[1].shrink_to_fit();
  L.win0 = win0.data(), L.win1 = win1.data(), L.order = order.data(), L.stream_start = start.data(), L.src0 = src[0].data(), L.src1 = src[1].data();
  L.synth0 = synth[0].data(), L.synth1 = synth[1].data();
  if (nblocks < 1 || frames < 0 || frames > at) return printf("lap: %d frames of %lld decoded\n", frames, at), 2;
  std::vector<float> out((size_t)L.ch * frames);
  const long long first = lap_centre(L, 0);
  for (long long t = 0; t < frames; t++) {
    const long long k = lap_find(L, start[0], start[1], first + t);
    for (int c = 0; c < L.ch; c++) out[(size_t)c * frames + t] = lap_sample(L, k, first + t, c);
  }
  spill(outpath, out);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 4 && !strcmp(argv[1], "mdct")) return run_mdct(argv[2], argv[3]);
  if (argc == 5 && !strcmp(argv[1], "block")) return run_block(argv[2], argv[3], argv[4]);
  if (argc == 4 && !strcmp(argv[1], "lap")) return run_lap(argv[2], argv[3]);
  printf("usage: synth_host mdct job out | block setup job out | lap job out\n");
  return 2;
}
