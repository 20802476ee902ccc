// tests/c/decode_links_host.cpp -- TEST BUILD ONLY (tests/test_decode_links_cpu.py; built with -fsanitize=address,undefined).
// The reader's bookkeeping for one lane on the host: the shipped scan with and without the follow policy and the plan from
// per-packet marks (vorbis_amd/csrc/vamd_demux.h, vamd_decode_plan.h), k_ogg_depage's body with the lanes in turn
// (k_demux.h), unpack_packet (k_unpack.h), synth_block and the segments' lap body lap_segment (k_synth.h), as
// vamd_decode_ogg / vamd_decode_streams_marked sequence them.  Every buffer has exactly the size the library gives it, so
// that a read or write beyond one is the sanitiser's to report.
//   decode_links_host ogg setup job out
//     job: int32 follow, int32 nstreams, int32 setup_header_bytes, the setup header (padded to 4), per stream: int64 bytes,
//          the file (padded to 4)
//     out: per stream a result; with follow 0 the walk alone runs and no result has floats
//   decode_links_host packets setup job out
//     job: int32 nstreams, npackets, int32 decode, then int64 arrays (int32 count + elements) offset, stream_start, granule,
//          eos (count 0: NULL), int32 nbytes and the bytes (padded to 4)
//     out: int32 ok (0: the descriptor was refused, nothing follows), then per stream a result
//   decode_links_host links setup job out
//     job: int32 cap, int64 bytes, the file
//     out: int32 return code, int64 nlinks, then min(cap, nlinks) x int64 begin, end, serial
//   a result: int32 status, int64 frames, int32 nsegments, per segment int64 k0, k1, first, count, out_at; then, where the
//          status is 0 and the job decodes, float [ch][frames]
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "vamd_bind.h"
#include "k_synth.h"
#include "k_unpack.h"
#include "vamd_decode_plan.h"
#include "vamd_demux.h"

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

// From the arena on: k_unpack and k_synth over the plan's blocks in turn, then per stream its result -- with `decode` the
// rows of kept frames through k_lap_segments' body, a thread at a time, into exactly the stream's floats.
static void run_plan(const Setup &S, const DecodePlan &P, const std::vector<uint32_t> &words, const int64_t *offs, std::vector<uint8_t> status, bool decode,
                     FILE *f) {
  const Bound &B = S.B;
  const int ch = B.channels;
  const int64_t ns = (int64_t)P.frames.size();
  const float nan = nanf("");
  AlignedFloats synth0(decode ? (size_t)P.nblocks[0] * ch * B.bs[0] : 0, nan), synth1(decode ? (size_t)P.nblocks[1] * ch * B.bs[1] : 0, nan);
  for (int64_t s = 0; decode && s < ns; s++)
    for (int64_t k = P.lap_start[(size_t)s]; k < P.lap_start[(size_t)s + 1]; k++) {
      const int W = (P.order[(size_t)k] >> 30) & 1, i = P.order[(size_t)k] & 0x3fffffff;
      const int n = B.bs[W], n2 = n / 2, SM = B.chmap[W].submaps;
      std::vector<int32_t> post_valid((size_t)ch, 0), res_class((size_t)SM * VAMD_RES_CLASS_STRIDE, 0), res_count((size_t)2 * SM, 0);
      std::vector<uint32_t> ilog_words((size_t)ch * n2 / 4, 0);
      std::vector<uint16_t> res_entries((size_t)B.res_cap[W], 0);
      std::vector<int> fit(VAMD_POSIT);
      PhaseClock pc;
      pc.start(nullptr);
      const int64_t p = P.packet[(size_t)k];
      status[(size_t)s] |= (uint8_t)unpack_packet(B, S.U, words.data(), (long long)words.size(), 8 * offs[p], 8 * offs[p + 1], W, post_valid.data(),
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
  size_t g = 0;
  for (int64_t s = 0; s < ns; s++) {
    const int32_t st = status[(size_t)s];
    const int64_t frames = P.frames[(size_t)s];
    size_t g1 = g;
    while (g1 < P.segments.size() && P.segments[g1].stream == s) g1++;
    const int32_t nseg = (int32_t)(g1 - g);
    put(f, &st, 4), put(f, &frames, 8), put(f, &nseg, 4);
    for (size_t i = g; i < g1; i++) {
      const DecodePlan::Segment &e = P.segments[i];
      const int64_t row[5] = {e.k0, e.k1, e.first, e.count, e.out_at};
      put(f, row, sizeof(row));
    }
    if (decode && !st) {
      AlignedFloats out((size_t)ch * frames, nan);  // (exactly the stream's floats: k_lap_segments writes no other)
      for (size_t i = g; i < g1; i++) {
        const DecodePlan::Segment &e = P.segments[i];
        const LapSegment row = {e.k0, e.k1, e.first, e.count, frames, e.out_at};
        for (long long q = 0; 4 * q < row.count; q++) lap_segment(L, row, q, out.p);
      }
      put(f, out.p, 4 * (size_t)ch * frames);
    }
    g = g1;
  }
  if (g != P.segments.size()) {
    printf("segments out of stream order\n");
    exit(1);
  }
}

static int run_ogg(const Setup &S, Reader &r, FILE *f) {
  const Bound &B = S.B;
  const int follow = r.i32(), ns = r.i32(), hb = r.i32();
  if (ns < 0 || hb < 0) return printf("job: counts\n"), 2;
  Exact header((size_t)hb);
  r.bytes(header.p, hb);
  // the files back to back in a buffer of exactly their sum
  std::vector<int64_t> off(1, 0);
  const size_t files_at = r.at;
  for (int s = 0; s < ns; s++) {
    const int64_t n = r.i64();
    if (n < 0) return 2;
    off.push_back(off.back() + n);
    r.at += (size_t)((n + 3) & ~(int64_t)3);
  }
  Exact files((size_t)off.back());
  r.at = files_at;
  for (int s = 0; s < ns; s++) {
    r.i64();
    r.bytes(files.p + off[(size_t)s], off[(size_t)s + 1] - off[(size_t)s]);
  }
  DemuxSetup DS;
  DS.channels = B.channels, DS.rate = B.rate, DS.bs[0] = B.bs[0], DS.bs[1] = B.bs[1];
  DS.setup_header = hb ? header.p : nullptr, DS.setup_header_bytes = hb;
  DemuxScan X;
  DecodePlan P;
  std::string err;
  if (!demux_scan(ns, files.p, off.data(), DS, &X, &err, follow != 0)) return printf("%s\n", err.c_str()), 2;
  const int64_t np = (int64_t)X.first.size();
  if (follow) {
    if (!decode_plan_build_marked(B.bs, S.U.modes, S.U.modebits, ns, np, nullptr, X.offset.data(), X.stream_start.data(), X.granule.data(), X.eos.data(), &P,
                                  &err, X.first.data(), X.links.data(), (int64_t)X.links.size()))
      return printf("%s\n", err.c_str()), 2;
  } else if (!decode_plan_build(B.bs, S.U.modes, S.U.modebits, ns, np, nullptr, X.offset.data(), X.stream_start.data(), X.end_granule.data(), &P, &err,
                                X.first.data())) {
    return printf("%s\n", err.c_str()), 2;
  }
  std::vector<uint8_t> status = P.status;
  for (int s = 0; s < ns; s++) status[(size_t)s] |= X.status[(size_t)s];
  // the upload rounded up to a dword + 16; the arena in whole dwords, bounded to its bytes
  const int64_t total = off.back(), arena = X.offset.back();
  std::vector<uint32_t> upload((size_t)(total + 3) / 4 + 4, 0xa5a5a5a5u);
  if (total) memcpy(upload.data(), files.p, (size_t)total);
  std::vector<uint32_t> words((size_t)((arena + 3) / 4), 0xeeeeeeeeu), words1((size_t)((arena + 3) / 4), 0xeeeeeeeeu);
  for (const OggDepage &pg : X.pages) {
    const uint8_t a = ogg_depage_host((const uint8_t *)upload.data(), total, pg, (uint8_t *)words.data(), arena, 64);
    const uint8_t b = ogg_depage_host((const uint8_t *)upload.data(), total, pg, (uint8_t *)words1.data(), arena, 1);
    if (a != b) return printf("a page's status differs between 64 lanes and one\n"), 1;
    if (a & OGG_DEPAGE_BADROW) return printf("a page row outside its buffers\n"), 1;
    status[(size_t)pg.stream] |= a;
  }
  if (words != words1) return printf("the arena differs between 64 lanes and one\n"), 1;
  run_plan(S, P, words, X.offset.data(), status, follow != 0, f);
  return 0;
}

static int run_packets(const Setup &S, Reader &r, FILE *f) {
  const Bound &B = S.B;
  const int64_t ns = r.i32(), np = r.i32();
  const int decode = r.i32();
  const std::vector<int64_t> offset = r.i64s(), start = r.i64s(), gran = r.i64s(), eos64 = r.i64s();
  std::vector<uint8_t> eos(eos64.begin(), eos64.end());
  const int nbytes = r.i32();
  if (nbytes < 0) return 2;
  Exact bytes((size_t)nbytes);
  r.bytes(bytes.p, nbytes);
  DecodePlan P;
  std::string err;
  int32_t ok = 1;
  if (!decode_plan_build_marked(B.bs, S.U.modes, S.U.modebits, ns, np, bytes.p, offset.data(), start.data(), gran.data(), eos.empty() ? nullptr : eos.data(), &P,
                                &err)) {
    ok = 0;
    put(f, &ok, 4);
    printf("refused: %s\n", err.c_str());
    return 0;
  }
  put(f, &ok, 4);
  std::vector<uint32_t> words((size_t)((nbytes + 3) / 4), 0u);
  if (nbytes) memcpy(words.data(), bytes.p, (size_t)nbytes);
  run_plan(S, P, words, offset.data(), P.status, decode != 0, f);
  return 0;
}

// vamd_ogg_links' body (vamd_decode.h) over demux_links, the file in a buffer of exactly its size
static int run_links(Reader &r, FILE *f) {
  const int64_t cap = r.i32(), n = r.i64();
  if (cap < 0 || n < 0) return 2;
  Exact file((size_t)n);
  r.bytes(file.p, n);
  std::vector<DemuxLink> links;
  const bool whole = demux_links(file.p, n, &links);
  const int64_t nlinks = (int64_t)links.size();
  const int32_t rc = !whole ? -133 : nlinks > cap ? -131 : 0;  // VAMD_EBADHEADER, VAMD_EINVAL
  put(f, &rc, 4), put(f, &nlinks, 8);
  for (int64_t k = 0; k < nlinks && k < cap; k++) {
    const int64_t row[3] = {links[(size_t)k].begin, links[(size_t)k].end, (int64_t)links[(size_t)k].serial};
    put(f, row, sizeof(row));
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 5 || (strcmp(argv[1], "ogg") && strcmp(argv[1], "packets") && strcmp(argv[1], "links")))
    return printf("usage: decode_links_host ogg|packets|links setup job out\n"), 2;
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
  const int rc = !strcmp(argv[1], "ogg") ? run_ogg(S, r, f) : !strcmp(argv[1], "packets") ? run_packets(S, r, f) : run_links(r, f);
  fclose(f);
  return rc;
}
