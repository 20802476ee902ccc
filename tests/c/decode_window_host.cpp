// tests/c/decode_window_host.cpp -- TEST BUILD ONLY (tests/test_decode_window_cpu.py; built with -fsanitize=address,undefined).
// The window decoder for one lane on the host: the shipped scan, seek index, window plan and staging layout
// (vorbis_amd/csrc/vamd_demux.h, vamd_decode_window_plan.h), the staging gather, k_ogg_depage's body with the lanes in
// turn (k_demux.h), unpack_packet (k_unpack.h), synth_block and the window's lap body lap_window (k_synth.h), call after
// call on one index, as vamd_decode_ogg_window / vamd_decode_window sequence them.  Every buffer has exactly the size the
// library gives it, so that a read or write beyond one is the sanitiser's to report.
//   decode_window_host ogg setup job out
//     job: int32 nstreams, int32 setup_header_bytes, the setup header (padded to 4), per stream: int64 bytes, the file
//          (padded to 4); int32 ncalls, then the calls
//     out: per stream int32 status, int64 frames (the index's); then the calls' results
//   decode_window_host packets setup job out
//     job: int32 nstreams, npackets, then int64 arrays (int32 count + elements) offset, stream_start, end_granule (count 0:
//          NULL), int32 nbytes and the bytes (padded to 4); int32 ncalls, then the calls
//     out: the calls' results
//   a call: int32 nullmask (bit 0 stream, 1 start, 2 count, 3 bytes, 4 file_offset: the pointer is NULL), int32 nwindows,
//          int64 arrays stream, start, count, file_offset (count 0: the index's own), int32 nfiles (0: the index's files
//          again; else per stream int64 bytes + the file, padded to 4)
//   a result: int32 ok; a refused call has 0 and nothing else; one that ran has 1, int64 nblocks[2], int64 bytes staged,
//          int64 page rows, then per window int32 status, int32 frames, float [ch][frames]
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "vamd_bind.h"
#include "k_synth.h"
#include "k_unpack.h"
#include "vamd_decode_window_plan.h"

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
  int64_t i64() {
    int64_t x;
    take(&x, 8);
    return x;
  }
  std::vector<int64_t> i64s() {
    const int n = i32();
    if (n < 0) exit(2);
    std::vector<int64_t> o((size_t)n);
    take(o.data(), 8 * (size_t)n);
    return o;
  }
  void bytes(unsigned char *dst, int64_t n) {
    take(dst, (size_t)n);
    at += (size_t)(-n & 3);
  }
};

// exactly n bytes, freed with the scope
struct Exact {
  unsigned char *p;
  explicit Exact(size_t n) : p((unsigned char *)malloc(n ? n : 1)) {}
  ~Exact() { free(p); }
  Exact(const Exact &) = delete;
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

struct Setup {
  std::vector<unsigned char> image, tab;
  Bound B;
  UnpackP U;
  SynthFloorP F[2];
};

// per stream int64 bytes + the file -> the files back to back in a buffer of exactly their sum, and their offsets
static Exact *read_files(Reader &r, int ns, std::vector<int64_t> *off) {
  off->assign(1, 0);
  const size_t files_at = r.at;
  for (int s = 0; s < ns; s++) {
    const int64_t n = r.i64();
    if (n < 0) exit(2);
    off->push_back(off->back() + n);
    r.at += (size_t)((n + 3) & ~(int64_t)3);
  }
  Exact *files = new Exact((size_t)off->back());
  r.at = files_at;
  for (int s = 0; s < ns; s++) {
    r.i64();
    r.bytes(files->p + (*off)[(size_t)s], (*off)[(size_t)s + 1] - (*off)[(size_t)s]);
  }
  return files;
}

// From the arena on: k_unpack, k_synth and k_lap_window over the windows' plan, the blocks and the threads in turn.
// words: the arena in whole dwords; block k's packet is its bytes [begin[k], begin[k] + offs[k+1] - offs[k]).
static void run_windows(const Setup &S, const WindowPlan &WP, const std::vector<uint32_t> &words, const int64_t *begin, const int64_t *offs,
                        std::vector<uint8_t> status, int64_t staged, int64_t rows, FILE *f) {
  const Bound &B = S.B;
  const DecodePlan &P = WP.P;
  const int ch = B.channels;
  const int64_t nw = (int64_t)P.frames.size();
  const float nan = nanf("");
  AlignedFloats synth0((size_t)P.nblocks[0] * ch * B.bs[0], nan), synth1((size_t)P.nblocks[1] * ch * B.bs[1], nan);
  for (int64_t w = 0; w < nw; w++)
    for (int64_t k = P.lap_start[(size_t)w]; k < P.lap_start[(size_t)w + 1]; k++) {
      const int W = (P.order[(size_t)k] >> 30) & 1, i = P.order[(size_t)k] & 0x3fffffff;
      const int n = B.bs[W], n2 = n / 2, SM = B.chmap[W].submaps;
      std::vector<int32_t> post_valid((size_t)ch, 0), res_class((size_t)SM * VAMD_RES_CLASS_STRIDE, 0), res_count((size_t)2 * SM, 0);
      std::vector<uint32_t> ilog_words((size_t)ch * n2 / 4, 0);
      std::vector<uint16_t> res_entries((size_t)B.res_cap[W], 0);
      std::vector<int> fit(VAMD_POSIT);
      PhaseClock pc;
      pc.start(nullptr);
      const int64_t p = P.packet[(size_t)k], at = begin ? begin[p] : offs[p];
      status[(size_t)w] |= (uint8_t)unpack_packet(B, S.U, words.data(), (long long)words.size(), 8 * at, 8 * (at + offs[p + 1] - offs[p]), W, post_valid.data(),
                                                  (ilog_t *)ilog_words.data(), res_class.data(), res_entries.data(), res_count.data(), fit.data(), 1, pc);
      AlignedFloats lds(synth_lds_words(ch, n2, 1, B.res_off_ints[W]));
      synth_block(B.xf[W], B.res[W][0], B.res[W][1], B.chmap[W], B.couple[W], S.F[W], ch, B.res_off_ints[W], post_valid.data(), (ilog_t *)ilog_words.data(),
                  res_class.data(), res_entries.data(), res_count.data(), lds.p, (W ? synth1.p : synth0.p) + (size_t)i * ch * n, pc);
    }
  LapP L;
  memset(&L, 0, sizeof(L));
  L.ch = ch, L.bs0 = B.bs[0], L.bs1 = B.bs[1];
  L.win0 = B.xf[0].win_short, L.win1 = B.xf[0].win_long;
  L.order = P.order.data(), L.stream_start = (const long long *)P.lap_start.data();
  L.src0 = (const long long *)P.src[0].data(), L.src1 = (const long long *)P.src[1].data();
  L.synth0 = synth0.p, L.synth1 = synth1.p;
  const int32_t ok = 1;
  const int64_t nb[2] = {P.nblocks[0], P.nblocks[1]};
  put(f, &ok, 4), put(f, nb, 16), put(f, &staged, 8), put(f, &rows, 8);
  for (int64_t w = 0; w < nw; w++) {
    const int32_t st = status[(size_t)w], frames = (int32_t)P.frames[(size_t)w];
    put(f, &st, 4), put(f, &frames, 4);
    AlignedFloats out((size_t)ch * frames, nan);  // (exactly the window's floats: k_lap_window writes no other)
    for (long long q = 0; 4 * q < frames; q++)
      lap_window(L, P.lap_start[(size_t)w], P.lap_start[(size_t)w + 1], WP.first[(size_t)w], frames, frames, q, out.p);
    put(f, out.p, 4 * (size_t)ch * frames);
  }
}

static void refuse(FILE *f, int call, const std::string &err) {
  const int32_t ok = 0;
  put(f, &ok, 4);
  printf("call %d refused: %s\n", call, err.c_str());
}

struct Call {
  int nullmask, nw;
  std::vector<int64_t> stream, start, count, file_offset;
  explicit Call(Reader &r) {
    nullmask = r.i32(), nw = r.i32();
    stream = r.i64s(), start = r.i64s(), count = r.i64s(), file_offset = r.i64s();
  }
  const int64_t *ptr(int bit, const std::vector<int64_t> &v) const { return (nullmask >> bit) & 1 ? nullptr : v.data(); }
};

static int run_ogg(const Setup &S, Reader &r, FILE *f) {
  const Bound &B = S.B;
  const int ns = r.i32(), hb = r.i32();
  if (ns < 0 || hb < 0) return printf("job: counts\n"), 2;
  Exact header((size_t)hb);
  r.bytes(header.p, hb);
  std::vector<int64_t> off;
  Exact *files = read_files(r, ns, &off);
  DemuxSetup DS;
  DS.channels = B.channels, DS.rate = B.rate, DS.bs[0] = B.bs[0], DS.bs[1] = B.bs[1];
  DS.setup_header = hb ? header.p : nullptr, DS.setup_header_bytes = hb;
  OggIndex I;
  std::string err;
  if (!ogg_index_build(B.bs, S.U.modes, S.U.modebits, ns, files->p, off.data(), DS, &I, &err)) return printf("%s\n", err.c_str()), 2;
  for (int s = 0; s < ns; s++) {
    const int32_t st = I.whole.status[(size_t)s];
    put(f, &st, 4), put(f, &I.whole.frames[(size_t)s], 8);
  }
  const int ncalls = r.i32();
  for (int call = 0; call < ncalls; call++) {
    Call c(r);
    const int nfiles = r.i32();
    std::vector<int64_t> other_off;
    Exact *other = nfiles ? read_files(r, nfiles, &other_off) : nullptr;
    // the files handed again: a copy of exactly their bytes, made for this call and gone after it
    const std::vector<int64_t> &foff = !c.file_offset.empty() ? c.file_offset : other ? other_off : off;
    const Exact *src = other ? other : files;
    const int64_t total = other ? other_off.back() : off.back();
    Exact again((size_t)total);
    if (total) memcpy(again.p, src->p, (size_t)total);
    delete other;
    const uint8_t *bytes = (c.nullmask >> 3) & 1 ? nullptr : again.p;
    WindowPlan WP;
    OggWindowStage G;
    if ((int64_t)foff.size() != ns + 1 && !((c.nullmask >> 4) & 1)) return printf("job: file_offset\n"), 2;
    if (!ogg_window_files_check(I, bytes, c.ptr(4, foff), &err) ||
        !window_plan_build(I.whole, B.bs, c.nw, c.ptr(0, c.stream), c.ptr(1, c.start), c.ptr(2, c.count), &WP, &err) ||
        !ogg_window_stage(I, WP, c.stream.data(), &G, &err)) {
      refuse(f, call, err);
      continue;
    }
    // the staging buffer exactly its bytes; the upload rounded up to a dword + 16; the arena in whole dwords, bounded to its bytes
    Exact stage((size_t)G.stage_bytes);
    ogg_window_gather(G, bytes, foff.data(), stage.p);
    std::vector<uint32_t> upload((size_t)(G.stage_bytes + 3) / 4 + 4, 0xa5a5a5a5u);
    if (G.stage_bytes) memcpy(upload.data(), stage.p, (size_t)G.stage_bytes);
    std::vector<uint32_t> words((size_t)((G.arena_bytes + 3) / 4), 0xeeeeeeeeu), words1((size_t)((G.arena_bytes + 3) / 4), 0xeeeeeeeeu);
    std::vector<uint8_t> status = WP.P.status;
    for (const OggDepage &pg : G.pages) {
      const uint8_t a = ogg_depage_host((const uint8_t *)upload.data(), G.stage_bytes, pg, (uint8_t *)words.data(), G.arena_bytes, 64);
      const uint8_t b = ogg_depage_host((const uint8_t *)upload.data(), G.stage_bytes, pg, (uint8_t *)words1.data(), G.arena_bytes, 1);
      if (a != b) return printf("a page's status differs between 64 lanes and one\n"), 1;
      if (a & OGG_DEPAGE_BADROW) return printf("a page row outside its buffers\n"), 1;
      status[(size_t)pg.stream] |= a;
    }
    if (words != words1) return printf("the arena differs between 64 lanes and one\n"), 1;
    run_windows(S, WP, words, G.begin.data(), G.offs.data(), status, G.stage_bytes, (int64_t)G.pages.size(), f);
  }
  delete files;
  return 0;
}

static int run_packets(const Setup &S, Reader &r, FILE *f) {
  const Bound &B = S.B;
  const int64_t ns = r.i32(), np = r.i32();
  const std::vector<int64_t> offset = r.i64s(), start = r.i64s(), gran = r.i64s();
  const int nbytes = r.i32();
  if (nbytes < 0) return 2;
  Exact bytes((size_t)nbytes);
  r.bytes(bytes.p, nbytes);
  const int ncalls = r.i32();
  std::string err;
  for (int call = 0; call < ncalls; call++) {
    Call c(r);
    if (r.i32()) return printf("job: files in a packet call\n"), 2;
    DecodePlan whole;
    WindowPlan WP;
    if (!decode_plan_build(B.bs, S.U.modes, S.U.modebits, ns, np, (c.nullmask >> 3) & 1 ? nullptr : bytes.p, offset.data(), start.data(),
                           gran.empty() ? nullptr : gran.data(), &whole, &err) ||
        !window_plan_build(whole, B.bs, c.nw, c.ptr(0, c.stream), c.ptr(1, c.start), c.ptr(2, c.count), &WP, &err)) {
      refuse(f, call, err);
      continue;
    }
    std::vector<int64_t> offs;
    window_packet_layout(WP, offset.data(), &offs);
    Exact stage((size_t)offs.back());
    window_packet_gather(WP, bytes.p, offset.data(), offs, stage.p);
    std::vector<uint32_t> words((size_t)((offs.back() + 3) / 4), 0u);
    if (offs.back()) memcpy(words.data(), stage.p, (size_t)offs.back());
    run_windows(S, WP, words, nullptr, offs.data(), WP.P.status, offs.back(), 0, f);
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 5 || (strcmp(argv[1], "ogg") && strcmp(argv[1], "packets"))) return printf("usage: decode_window_host ogg|packets setup job out\n"), 2;
  const std::vector<unsigned char> blob = slurp(argv[2]), raw = slurp(argv[3]);
  Setup S;
  std::vector<uint32_t> doff;
  std::vector<PsyDerived> derived;
  std::string err;
  if (build_image(blob.data(), blob.size(), &S.image, &doff, &derived, &err) != VAMD_OK) return printf("setup: %s\n", err.c_str()), 2;
  bind_params(S.image, doff, derived, S.image.data(), &S.B);
  if (!unpack_check_setup(S.image, &err)) return printf("%s\n", err.c_str()), 2;
  unpack_build_tables(S.image, &S.tab, &S.U);
  for (int W = 0; W < S.U.modes; W++)
    if (!S.B.res_cap[W] || !synth_floor_ranges(S.B.floor[W][0], S.B.floor[W][1], S.B.chmap[W].submaps, S.B.bs[W] / 2, &S.F[W])) return printf("not synthesised\n"), 2;
  FILE *f = fopen(argv[4], "wb");
  if (!f) return printf("cannot write %s\n", argv[4]), 2;
  Reader r(raw);
  const int rc = !strcmp(argv[1], "ogg") ? run_ogg(S, r, f) : run_packets(S, r, f);
  fclose(f);
  return rc;
}
