// tests/c/unpack_partial_host.cpp -- TEST BUILD ONLY (tests/test_unpack_partial_cpu.py; built with -fsanitize=address,undefined).
// The packet decoder under the keep policy (vamd_decode_partial), one lane on the host from the shipped headers: k_unpack.h's
// second instantiation of the walk (unpack_packet_partial) with the planning of vamd_decode_plan.h, and behind it k_synth.h's
// bounded residue add -- what k_unpack_partial and k_synth_bounded / k_synth_values_bounded run.  With keep = 0 it runs the
// default pair instead (unpack_packet, synth_block), so that one program shows both policies on the same input.  Every
// buffer has exactly the size the GPU launch gives it, so that a read or write beyond one is the sanitiser's to report.
//   SETUP is `blob <setup blob>` or `headers <identification packet> <setup packet>` (vamd_headers.h: the value lists too)
//   unpack_partial_host blocks  SETUP job out   job: int32 keep | int32 nblocks | per block: int32 bytes, the packet (padded
//                                               to 4); the block's size class is the one its own head names
//                                               out, per block: int32 [12] = status, W, the place the reader FIRST failed at
//                                               (UNPACK_AT_*, 0: nowhere), that place's channel or submap, its stage,
//                                               res_count[submaps][2] (four ints), 1 where vb->pcm follows, 0, 0;
//                                               then float vb->pcm [ch][n] where status & ~VAMD_STATUS_PARTIAL is 0
//   unpack_partial_host ends    SETUP job out   job as `blocks` (keep is not read: the keep policy's walk); out, per block and
//                                               submap (two): int32 count, then int32 [count] the bit of the packet behind
//                                               which the reader stood when it had read each entry, in reading order
//   unpack_partial_host streams SETUP job out   job: int32 keep | int32 nstreams | per stream: int32 npackets, int64
//                                               end_granule, per packet: int32 bytes, the packet (padded to 4)
//                                               out, per stream: int32 status, int32 frames, float [ch][frames]
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "vamd_headers.h"
#include "vamd_decode_plan.h"

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
  long long i64() {
    int64_t x;
    take(&x, 8);
    return x;
  }
  std::vector<unsigned char> packet() {
    const int n = i32();
    if (n < 0) exit(2);
    std::vector<unsigned char> p((size_t)n);
    take(p.data(), (size_t)n);
    at += (size_t)(-n & 3);
    return p;
  }
};

struct AlignedFloats {
  float *p;
  explicit AlignedFloats(size_t count) {
    p = (float *)aligned_alloc(16, (count * 4 + 15) & ~(size_t)15);
    memset(p, 0, count * 4);
  }
  ~AlignedFloats() { free(p); }
};

static void put(FILE *f, const void *p, size_t bytes) {
  if (bytes && fwrite(p, 1, bytes, f) != bytes) {
    printf("cannot write\n");
    exit(2);
  }
}

// a setup from a blob or from a stream's headers; argv[*at] names which, *at moves past it
struct Setup {
  std::vector<unsigned char> image, tab;
  std::vector<int> value_off;
  std::vector<float> values;  // (the value lists in a buffer of exactly their size)
  bool table = false;
  Bound B;
  UnpackP U;
  ValueP V = {nullptr, nullptr};
  Setup(int argc, char **argv, int *at) {
    std::string err;
    std::vector<uint32_t> doff;
    std::vector<PsyDerived> derived;
    if (*at + 1 < argc && !strcmp(argv[*at], "blob")) {
      const std::vector<unsigned char> blob = slurp(argv[*at + 1]);
      if (build_image(blob.data(), blob.size(), &image, &doff, &derived, &err) != VAMD_OK) {
        printf("setup: %s\n", err.c_str());
        exit(2);
      }
      *at += 2;
    } else if (*at + 2 < argc && !strcmp(argv[*at], "headers")) {
      const std::vector<unsigned char> id = slurp(argv[*at + 1]), setup = slurp(argv[*at + 2]);
      HeaderImage H;
      const int r = headers_to_image(id.data(), id.size(), setup.data(), setup.size(), &H, &err);
      if (r) {
        printf("headers_to_image: %d %s\n", r, err.c_str());
        exit(2);
      }
      image = H.image, doff = H.derived_off, derived = H.derived;
      value_off.assign(H.value_off.begin(), H.value_off.end());
      values = H.values;
      table = H.table_books > 0;
      *at += 3;
    } else {
      printf("setup: blob <file> | headers <identification> <setup>\n");
      exit(2);
    }
    bind_params(image, doff, derived, image.data(), &B);
    if (!unpack_check_setup(image, &err)) {
      printf("%s\n", err.c_str());
      exit(2);
    }
    unpack_build_tables(image, &tab, &U);
    V.book_off = value_off.data(), V.values = values.data();
  }
};

// where the reader first failed, and where it stood behind every entry it read
struct FirstStop {
  int place = 0, index = 0, stage = 0;
  std::vector<long long> ends[VAMD_MAX_SUBMAPS];
  void stop(int p, int i, int s) {
    if (!place) place = p, index = i, stage = s;
  }
  void entry(int sm, long long pos) {
    if (sm >= 0 && sm < VAMD_MAX_SUBMAPS) ends[sm].push_back(pos);
  }
};

// one block's rows, each exactly as long as the launch's
struct Rows {
  std::vector<int32_t> post_valid, res_class, res_count;
  std::vector<uint32_t> ilog_words;  // (4-byte aligned bytes)
  std::vector<uint16_t> res_entries;
  int W;
  Rows(const Bound &B, int W_) : W(W_) {
    const int ch = B.channels, n2 = B.bs[W] / 2, S = B.chmap[W].submaps;
    post_valid.assign((size_t)ch, 0);
    ilog_words.assign((size_t)ch * n2 / 4, 0);
    // (the device's rows are reused from call to call: what a walk leaves unwritten there is whatever was there)
    res_class.assign((size_t)S * VAMD_RES_CLASS_STRIDE, 0x5a5a5a5a);
    res_count.assign((size_t)2 * S, 0x5a5a5a5a);
    res_entries.assign((size_t)B.res_cap[W], 0x5a5a);
  }
  ilog_t *ilog() { return (ilog_t *)ilog_words.data(); }
};

static std::vector<uint32_t> as_words(const std::vector<unsigned char> &bytes) {
  std::vector<uint32_t> w((bytes.size() + 3) / 4, 0u);
  if (!bytes.empty()) memcpy(w.data(), bytes.data(), bytes.size());
  return w;
}

// the packet at bytes [o0, o1) of a buffer of whole dwords, under either policy
static int unpack(const Setup &S, int keep, const std::vector<uint32_t> &words, long long o0, long long o1, Rows &r, FirstStop *where) {
  std::vector<int> fit(VAMD_POSIT);
  PhaseClock pc;
  pc.start(nullptr);
  if (keep)
    return unpack_packet_partial(S.B, S.U, words.data(), (long long)words.size(), 8 * o0, 8 * o1, r.W, r.post_valid.data(), r.ilog(), r.res_class.data(),
                                 r.res_entries.data(), r.res_count.data(), fit.data(), 1, pc, *where);
  return unpack_packet(S.B, S.U, words.data(), (long long)words.size(), 8 * o0, 8 * o1, r.W, r.post_valid.data(), r.ilog(), r.res_class.data(),
                       r.res_entries.data(), r.res_count.data(), fit.data(), 1, pc);
}

// the kernel the launch would take: k_synth / k_synth_values by the setup, their bounded forms under the keep policy
static bool synth(const Setup &S, int keep, Rows &r, float *out) {
  const Bound &B = S.B;
  const int W = r.W, ch = B.channels, n2 = B.bs[W] / 2;
  SynthFloorP F;
  if (!B.res_cap[W] || !synth_floor_ranges(B.floor[W][0], B.floor[W][1], B.chmap[W].submaps, n2, &F)) return false;
  AlignedFloats lds(synth_lds_words(ch, n2, 1, B.res_off_ints[W]));
  PhaseClock pc;
  pc.start(nullptr);
#define SYNTH(TABLE, BOUNDED)                                                                                                                          \
  synth_block<TABLE, BOUNDED>(B.xf[W], B.res[W][0], B.res[W][1], B.chmap[W], B.couple[W], F, ch, B.res_off_ints[W], r.post_valid.data(), r.ilog(), \
                              r.res_class.data(), r.res_entries.data(), r.res_count.data(), lds.p, out, pc, S.V)
  if (S.table && keep) SYNTH(true, true);
  else if (S.table) SYNTH(true, false);
  else if (keep) SYNTH(false, true);
  else SYNTH(false, false);
#undef SYNTH
  return true;
}

static int run_blocks(const Setup &S, const char *job, const char *outpath) {
  const Bound &B = S.B;
  const std::vector<unsigned char> raw = slurp(job);
  Reader r(raw);
  FILE *f = fopen(outpath, "wb");
  if (!f) return printf("cannot write %s\n", outpath), 2;
  const int keep = r.i32(), nblocks = r.i32();
  for (int b = 0; b < nblocks; b++) {
    const std::vector<unsigned char> p = r.packet();
    const int cls = decode_packet_class(p.data(), (int64_t)p.size(), S.U.modes, S.U.modebits);
    const int W = cls < 0 ? 0 : cls;  // (a head the plan refuses: the walk refuses it too)
    Rows rows(B, W);
    FirstStop where;
    const int status = unpack(S, keep, as_words(p), 0, (long long)p.size(), rows, &where);
    const bool kept = !(status & ~VAMD_STATUS_PARTIAL);
    int32_t rec[12] = {status, W, where.place, where.index, where.stage, 0, 0, 0, 0, kept ? 1 : 0, 0, 0};
    for (int k = 0; k < 2 * B.chmap[W].submaps && k < 4; k++) rec[5 + k] = rows.res_count[(size_t)k];
    put(f, rec, sizeof(rec));
    if (kept) {
      std::vector<float> pcm((size_t)B.channels * B.bs[W], 0.f);
      if (!synth(S, keep, rows, pcm.data())) return printf("block %d: not synthesised\n", b), 2;
      put(f, pcm.data(), 4 * pcm.size());
    }
  }
  fclose(f);
  return 0;
}

static int run_ends(const Setup &S, const char *job, const char *outpath) {
  const std::vector<unsigned char> raw = slurp(job);
  Reader r(raw);
  FILE *f = fopen(outpath, "wb");
  if (!f) return printf("cannot write %s\n", outpath), 2;
  r.i32();
  const int nblocks = r.i32();
  for (int b = 0; b < nblocks; b++) {
    const std::vector<unsigned char> p = r.packet();
    const int cls = decode_packet_class(p.data(), (int64_t)p.size(), S.U.modes, S.U.modebits);
    Rows rows(S.B, cls < 0 ? 0 : cls);
    FirstStop where;
    unpack(S, 1, as_words(p), 0, (long long)p.size(), rows, &where);
    for (int sm = 0; sm < 2; sm++) {
      std::vector<int32_t> out(1, sm < VAMD_MAX_SUBMAPS ? (int32_t)where.ends[sm].size() : 0);
      for (int k = 0; k < out[0]; k++) out.push_back((int32_t)where.ends[sm][(size_t)k]);
      put(f, out.data(), 4 * out.size());
    }
  }
  fclose(f);
  return 0;
}

static int run_streams(const Setup &S, const char *job, const char *outpath) {
  const Bound &B = S.B;
  const std::vector<unsigned char> raw = slurp(job);
  Reader r(raw);
  const int keep = r.i32(), nstreams = r.i32();
  // the descriptor as a caller of vamd_decode_streams holds it: the packets back to back
  std::vector<unsigned char> bytes;
  std::vector<int64_t> offset = {0}, start = {0}, granule;
  for (int s = 0; s < nstreams; s++) {
    const int np = r.i32();
    granule.push_back(r.i64());
    for (int k = 0; k < np; k++) {
      const std::vector<unsigned char> p = r.packet();
      bytes.insert(bytes.end(), p.begin(), p.end());
      offset.push_back((int64_t)bytes.size());
    }
    start.push_back((int64_t)offset.size() - 1);
  }
  DecodePlan P;
  std::string err;
  if (!decode_plan_build(B.bs, S.U.modes, S.U.modebits, nstreams, (int64_t)offset.size() - 1, bytes.data(), offset.data(), start.data(), granule.data(), &P,
                         &err))
    return printf("%s\n", err.c_str()), 2;
  const std::vector<uint32_t> words = as_words(bytes);
  const int ch = B.channels;
  std::vector<float> pcm[2];
  for (int W = 0; W < 2; W++) pcm[W].assign((size_t)P.nblocks[W] * ch * B.bs[W], 0.f);
  std::vector<uint8_t> status = P.status;
  for (int s = 0; s < nstreams; s++)
    for (int64_t k = P.lap_start[(size_t)s]; k < P.lap_start[(size_t)s + 1]; k++) {
      const int W = (P.order[(size_t)k] >> 30) & 1, i = P.order[(size_t)k] & 0x3fffffff;
      Rows rows(B, W);
      FirstStop where;
      const int64_t p = P.packet[(size_t)k];
      status[(size_t)s] |= (uint8_t)unpack(S, keep, words, offset[(size_t)p], offset[(size_t)p + 1], rows, &where);
      if (!synth(S, keep, rows, pcm[W].data() + (size_t)i * ch * B.bs[W])) return printf("not synthesised\n"), 2;
    }
  LapP L;
  memset(&L, 0, sizeof(L));
  L.ch = ch, L.bs0 = B.bs[0], L.bs1 = B.bs[1];
  L.win0 = B.xf[0].win_short, L.win1 = B.xf[0].win_long;
  L.order = P.order.data(), L.stream_start = (const long long *)P.lap_start.data();
  L.src0 = (const long long *)P.src[0].data(), L.src1 = (const long long *)P.src[1].data();
  L.synth0 = pcm[0].data(), L.synth1 = pcm[1].data();
  FILE *f = fopen(outpath, "wb");
  if (!f) return printf("cannot write %s\n", outpath), 2;
  for (int s = 0; s < nstreams; s++) {
    // (the host's rule: a stream whose only flag is VAMD_STATUS_PARTIAL has its planned frames)
    const int32_t st = status[(size_t)s], frames = (st & ~VAMD_STATUS_PARTIAL) ? 0 : (int32_t)P.frames[(size_t)s];
    put(f, &st, 4);
    put(f, &frames, 4);
    std::vector<float> out((size_t)ch * frames);
    const long long k0 = P.lap_start[(size_t)s], k1 = P.lap_start[(size_t)s + 1];
    for (long long t = 0; t < frames; t++) {  // (frames > 0: at least two blocks, the first centre at 0)
      const long long k = lap_find(L, k0, k1, t);
      for (int c = 0; c < ch; c++) out[(size_t)c * frames + t] = lap_sample(L, k, t, c);
    }
    put(f, out.data(), 4 * out.size());
  }
  fclose(f);
  return 0;
}

int main(int argc, char **argv) {
  if (argc >= 2 && (!strcmp(argv[1], "blocks") || !strcmp(argv[1], "streams") || !strcmp(argv[1], "ends"))) {
    int at = 2;
    Setup S(argc, argv, &at);
    if (argc == at + 2 && !strcmp(argv[1], "ends")) return run_ends(S, argv[at], argv[at + 1]);
    if (argc == at + 2) return !strcmp(argv[1], "blocks") ? run_blocks(S, argv[at], argv[at + 1]) : run_streams(S, argv[at], argv[at + 1]);
  }
  printf("usage: unpack_partial_host blocks|ends|streams (blob <setup> | headers <identification> <setup>) job out\n");
  return 2;
}
