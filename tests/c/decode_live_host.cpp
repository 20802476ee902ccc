// tests/c/decode_live_host.cpp -- TEST BUILD ONLY (tests/test_decode_live_cpu.py; built with -fsanitize=address,undefined).
// The live decoder for one lane on the host: the shipped planning (vorbis_amd/csrc/vamd_decode_live_plan.h), unpack_packet
// (k_unpack.h), synth_block, the two carry bodies and lap_sample (k_synth.h), call after call on one decoder, as
// vamd_decode_live_wrote sequences them.  Every buffer has exactly the size the GPU launch gives it, so that a read or
// write beyond one is the sanitiser's to report; the half of a carried row that nothing may read holds NaNs.
//   decode_live_host setup job out
//     job: int32 max_streams, ncalls | per call: int32 nstreams, npackets, nullmask (bit 0 slot, 1 bytes, 2 offset,
//          3 stream_start, 4 close, 5 end_granule: the pointer is NULL), then five arrays, each int32 count + elements:
//          int64 slot, int64 offset, int64 stream_start, int64 close (0 / 1), int64 end_granule; then int32 nbytes and the
//          bytes, padded to 4
//     out: per call int32 ok; a refused call (a bad descriptor) has 0 and nothing else, and changes nothing; a call that ran
//          has 1, then per stream int32 status, int32 frames, float [ch][frames]
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "vamd_bind.h"
#include "k_synth.h"
#include "k_unpack.h"
#include "vamd_decode_live_plan.h"

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

struct Reader {
  const std::vector<unsigned char> &v;
  size_t at = 0;
  explicit Reader(const std::vector<unsigned char> &v_) : v(v_) {}
  void take(void *dst, size_t bytes) {
    if (at + bytes > v.size()) {
      printf("job file truncated\n");
      exit(2);
    }
    if (bytes) memcpy(dst, v.data() + at, bytes);
    at += bytes;
  }
  int i32() {
    int32_t x;
    take(&x, 4);
    return x;
  }
  std::vector<int64_t> i64s() {
    const int n = i32();
    if (n < 0) exit(2);
    std::vector<int64_t> o((size_t)n);
    take(o.data(), 8 * (size_t)n);
    return o;
  }
};

// 16-byte aligned floats, as device memory is; exactly `count` of them
struct AlignedFloats {
  float *p;
  explicit AlignedFloats(size_t count, float fill = 0.f) {
    p = (float *)aligned_alloc(16, ((count ? count : 4) * 4 + 15) & ~(size_t)15);
    for (size_t i = 0; i < count; i++) p[i] = fill;
  }
  ~AlignedFloats() { free(p); }
  AlignedFloats(const AlignedFloats &) = delete;
};

static void put(FILE *f, const void *p, size_t bytes) {
  if (bytes && fwrite(p, 1, bytes, f) != bytes) {
    printf("cannot write\n");
    exit(2);
  }
}

int main(int argc, char **argv) {
  if (argc != 4) return printf("usage: decode_live_host setup job out\n"), 2;
  const std::vector<unsigned char> blob = slurp(argv[1]), raw = slurp(argv[2]);
  std::vector<unsigned char> image, tab;
  std::vector<uint32_t> doff;
  std::vector<PsyDerived> derived;
  std::string err;
  Bound B;
  UnpackP U;
  if (build_image(blob.data(), blob.size(), &image, &doff, &derived, &err) != VAMD_OK) return printf("setup: %s\n", err.c_str()), 2;
  bind_params(image, doff, derived, image.data(), &B);
  if (!unpack_check_setup(image, &err)) return printf("%s\n", err.c_str()), 2;
  unpack_build_tables(image, &tab, &U);
  const int ch = B.channels;
  SynthFloorP F[2];
  for (int W = 0; W < U.modes; W++)
    if (!B.res_cap[W] || !synth_floor_ranges(B.floor[W][0], B.floor[W][1], B.chmap[W].submaps, B.bs[W] / 2, &F[W])) return printf("not synthesised\n"), 2;
  FILE *f = fopen(argv[3], "wb");
  if (!f) return printf("cannot write %s\n", argv[3]), 2;
  Reader r(raw);
  const int max_streams = r.i32(), ncalls = r.i32();
  if (max_streams < 1) return printf("max_streams\n"), 2;
  std::vector<LiveSlot> slots((size_t)max_streams);
  AlignedFloats carry((size_t)max_streams * ch * (B.bs[1] / 2));  // (vamd_decode_live_create zeroes it)
  for (int call = 0; call < ncalls; call++) {
    const int64_t ns = r.i32(), np = r.i32();
    const int nullmask = r.i32();
    const std::vector<int64_t> slot = r.i64s(), offset = r.i64s(), start = r.i64s(), close64 = r.i64s(), gran = r.i64s();
    std::vector<uint8_t> close(close64.begin(), close64.end());
    const int nbytes = r.i32();
    if (nbytes < 0) return 2;
    std::vector<unsigned char> bytes((size_t)nbytes);
    r.take(bytes.data(), bytes.size());
    r.at += (size_t)(-nbytes & 3);
    auto ptr = [&](int bit, const auto &v) { return (nullmask >> bit) & 1 ? nullptr : v.data(); };
    DecodeLivePlan L;
    int32_t ok = decode_live_plan_build(B.bs, U.modes, U.modebits, slots, ns, np, ptr(0, slot), ptr(1, bytes), ptr(2, offset), ptr(3, start), ptr(4, close),
                                        ptr(5, gran), &L, &err)
                     ? 1 : 0;
    put(f, &ok, 4);
    if (!ok) {
      printf("call %d refused: %s\n", call, err.c_str());
      continue;
    }
    const DecodePlan &P = L.P;
    // the arena as decode_run uploads it: the call's bytes from offset[0] on, in whole dwords
    const int64_t byte0 = np ? offset[0] : 0, arena = np ? offset[(size_t)np] - byte0 : 0;
    std::vector<uint32_t> words((size_t)((arena + 3) / 4), 0u);
    if (arena) memcpy(words.data(), bytes.data() + byte0, (size_t)arena);
    // k_synth's output per size class: the unpacked rows, the carried rows behind them
    const float nan = nanf("");
    AlignedFloats synth0((size_t)(P.nblocks[0] + P.extra[0]) * ch * B.bs[0], nan), synth1((size_t)(P.nblocks[1] + P.extra[1]) * ch * B.bs[1], nan);
    std::vector<uint8_t> status = P.status;
    for (int64_t s = 0; s < ns; s++)
      for (int64_t k = L.unpack_start[(size_t)s]; k < L.unpack_start[(size_t)s + 1]; k++) {
        const int W = (L.unpack[(size_t)k] >> 30) & 1, i = L.unpack[(size_t)k] & 0x3fffffff;
        const int n = B.bs[W], n2 = n / 2, S = B.chmap[W].submaps;
        std::vector<int32_t> post_valid((size_t)ch, 0), res_class((size_t)S * VAMD_RES_CLASS_STRIDE, 0), res_count((size_t)2 * S, 0);
        std::vector<uint32_t> ilog_words((size_t)ch * n2 / 4, 0);
        std::vector<uint16_t> res_entries((size_t)B.res_cap[W], 0);
        std::vector<int> fit(VAMD_POSIT);
        PhaseClock pc;
        pc.start(nullptr);
        const int64_t p = P.packet[(size_t)k];
        status[(size_t)s] |= (uint8_t)unpack_packet(B, U, words.data(), (long long)words.size(), 8 * (offset[(size_t)p] - byte0), 8 * (offset[(size_t)p + 1] - byte0), W,
                                                    post_valid.data(), (ilog_t *)ilog_words.data(), res_class.data(), res_entries.data(), res_count.data(),
                                                    fit.data(), 1, pc);
        AlignedFloats lds(synth_lds_words(ch, n2, 1, B.res_off_ints[W]));
        synth_block(B.xf[W], B.res[W][0], B.res[W][1], B.chmap[W], B.couple[W], F[W], ch, B.res_off_ints[W], post_valid.data(), (ilog_t *)ilog_words.data(),
                    res_class.data(), res_entries.data(), res_count.data(), lds.p, (W ? synth1.p : synth0.p) + (size_t)i * ch * n, pc);
      }
    CarryP C;
    C.ch = ch, C.bs0 = B.bs[0], C.bs1 = B.bs[1], C.carry = carry.p, C.synth0 = synth0.p, C.synth1 = synth1.p;
    for (const CarryRow &row : L.in)  // k_decode_carry_in, then k_decode_carry_out: the launch order
      for (int c = 0; c < ch; c++) decode_carry_in(C, row, c);
    for (const CarryRow &row : L.out)
      for (int c = 0; c < ch; c++) decode_carry_out(C, row, c);
    LapP Lp;
    memset(&Lp, 0, sizeof(Lp));
    Lp.ch = ch, Lp.bs0 = B.bs[0], Lp.bs1 = B.bs[1];
    Lp.win0 = B.xf[0].win_short, Lp.win1 = B.xf[0].win_long;
    Lp.order = P.order.data(), Lp.stream_start = (const long long *)P.lap_start.data();
    Lp.src0 = (const long long *)P.src[0].data(), Lp.src1 = (const long long *)P.src[1].data();
    Lp.synth0 = synth0.p, Lp.synth1 = synth1.p;
    for (int64_t s = 0; s < ns; s++) {
      const int32_t st = status[(size_t)s], frames = st ? 0 : (int32_t)P.frames[(size_t)s];
      put(f, &st, 4);
      put(f, &frames, 4);
      std::vector<float> out((size_t)ch * frames);
      const long long k0 = P.lap_start[(size_t)s], k1 = P.lap_start[(size_t)s + 1];
      if (frames > 0) {  // k_lap's walk of a stream
        if (k1 - k0 < 2) return printf("call %d stream %lld: frames without two blocks\n", call, (long long)s), 2;
        const long long first = lap_centre(Lp, k0), span = lap_centre(Lp, k1 - 1) - first;
        if (frames > span) return printf("call %d stream %lld: more frames than the centres span\n", call, (long long)s), 2;
        for (long long t = 0; t < frames; t++) {
          const long long k = lap_find(Lp, k0, k1, first + t);
          for (int c = 0; c < ch; c++) out[(size_t)c * frames + t] = lap_sample(Lp, k, first + t, c);
        }
      }
      put(f, out.data(), 4 * out.size());
    }
    decode_live_commit(&slots, L, ns, slot.data(), ptr(4, close), status.data());
  }
  fclose(f);
  return 0;
}
