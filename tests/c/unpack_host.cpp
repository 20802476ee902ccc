// tests/c/unpack_host.cpp -- TEST BUILD ONLY (tests/test_unpack_cpu.py; built with -fsanitize=address,undefined).
// The packet decoder's front half, vorbis_amd/csrc/k_unpack.h, compiled for one lane on the host with the planning of
// vamd_decode_plan.h, and behind it the shipped back half (k_synth.h): packets in, rows and samples out.  Every buffer has
// exactly the size the GPU launch gives it, so that a read or write beyond one is the sanitiser's to report.
//   unpack_host blocks  setup job out   job: int32 nblocks | per block: int32 W, int32 bytes, the packet (padded to 4)
//                                       out, per block, all int32: status, post_valid[ch], ilogmask[ch][n2],
//                                            res_class[submaps][VAMD_RES_CLASS_STRIDE], res_count[submaps][2],
//                                            res_entries[res_cap]; then float vb->pcm [ch][n] (synth_block over those rows)
//   unpack_host streams setup job out   job: int32 nstreams | per stream: int32 npackets, int64 end_granule, per packet:
//                                            int32 bytes, the packet (padded to 4)
//                                       out, per stream: int32 status, int32 frames, float [ch][frames]
//   unpack_host fuzz    setup job       job: as `streams`, the first stream is used.  Every packet cut at every byte length;
//                                            seeded single-bit flips; random bytes.  Exit 0 when every cut packet carries
//                                            VAMD_STATUS_TRUNCATED and every other outcome is a status or rows inside the
//                                            bounds synth_block's walk relies on (checked here, then walked).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "vamd_bind.h"
#include "k_synth.h"
#include "k_unpack.h"
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

struct Setup {
  std::vector<unsigned char> image, tab;
  Bound B;
  UnpackP U;
  explicit Setup(const char *path) {
    const std::vector<unsigned char> blob = slurp(path);
    std::vector<uint32_t> doff;
    std::vector<PsyDerived> derived;
    std::string err;
    if (build_image(blob.data(), blob.size(), &image, &doff, &derived, &err) != VAMD_OK) {
      printf("setup: %s\n", err.c_str());
      exit(2);
    }
    bind_params(image, doff, derived, image.data(), &B);
    if (!unpack_check_setup(image, &err)) {
      printf("%s\n", err.c_str());
      exit(2);
    }
    unpack_build_tables(image, &tab, &U);
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
    res_class.assign((size_t)S * VAMD_RES_CLASS_STRIDE, 0);
    res_count.assign((size_t)2 * S, 0);
    res_entries.assign((size_t)B.res_cap[W], 0);
  }
  ilog_t *ilog() { return (ilog_t *)ilog_words.data(); }
};

// the packet at bytes [o0, o1) of a buffer of whole dwords
static int unpack(const Setup &S, const std::vector<uint32_t> &words, long long o0, long long o1, Rows &r) {
  std::vector<int> fit(VAMD_POSIT);
  PhaseClock pc;
  pc.start(nullptr);
  return unpack_packet(S.B, S.U, words.data(), (long long)words.size(), 8 * o0, 8 * o1, r.W, r.post_valid.data(), r.ilog(), r.res_class.data(),
                       r.res_entries.data(), r.res_count.data(), fit.data(), 1, pc);
}

static std::vector<uint32_t> as_words(const std::vector<unsigned char> &bytes) {
  std::vector<uint32_t> w((bytes.size() + 3) / 4, 0u);
  if (!bytes.empty()) memcpy(w.data(), bytes.data(), bytes.size());
  return w;
}

static bool synth(const Setup &S, Rows &r, std::vector<float> *out) {
  const Bound &B = S.B;
  const int W = r.W, ch = B.channels, n = B.bs[W], n2 = n / 2;
  SynthFloorP F;
  if (!B.res_cap[W] || !synth_floor_ranges(B.floor[W][0], B.floor[W][1], B.chmap[W].submaps, n2, &F)) return false;
  AlignedFloats lds(synth_lds_words(ch, n2, 1, B.res_off_ints[W]));
  out->assign((size_t)ch * n, 0.f);
  PhaseClock pc;
  pc.start(nullptr);
  synth_block(B.xf[W], B.res[W][0], B.res[W][1], B.chmap[W], B.couple[W], F, ch, B.res_off_ints[W], r.post_valid.data(), r.ilog(), r.res_class.data(),
              r.res_entries.data(), r.res_count.data(), lds.p, out->data(), pc);
  return true;
}

static void put(FILE *f, const void *p, size_t bytes) {
  if (bytes && fwrite(p, 1, bytes, f) != bytes) {
    printf("cannot write\n");
    exit(2);
  }
}

static int run_blocks(const char *setup, const char *job, const char *outpath) {
  Setup S(setup);
  const std::vector<unsigned char> raw = slurp(job);
  Reader r(raw);
  FILE *f = fopen(outpath, "wb");
  if (!f) return printf("cannot write %s\n", outpath), 2;
  const int nblocks = r.i32();
  for (int b = 0; b < nblocks; b++) {
    const int W = r.i32();
    if (W != 0 && W != 1) return printf("block %d: size class\n", b), 2;
    const std::vector<unsigned char> p = r.packet();
    Rows rows(S.B, W);
    const int32_t status = unpack(S, as_words(p), 0, (long long)p.size(), rows);
    put(f, &status, 4);
    put(f, rows.post_valid.data(), 4 * rows.post_valid.size());
    std::vector<int32_t> wide((size_t)S.B.channels * (S.B.bs[W] / 2));
    for (size_t k = 0; k < wide.size(); k++) wide[k] = rows.ilog()[k];
    put(f, wide.data(), 4 * wide.size());
    put(f, rows.res_class.data(), 4 * rows.res_class.size());
    put(f, rows.res_count.data(), 4 * rows.res_count.size());
    wide.assign(rows.res_entries.begin(), rows.res_entries.end());
    put(f, wide.data(), 4 * wide.size());
    std::vector<float> pcm;
    if (!synth(S, rows, &pcm)) return printf("block %d: not synthesised\n", b), 2;
    put(f, pcm.data(), 4 * pcm.size());
  }
  fclose(f);
  return 0;
}

struct Stream {
  std::vector<std::vector<unsigned char>> packets;
  long long end_granule;
};
static std::vector<Stream> read_streams(Reader &r) {
  std::vector<Stream> out((size_t)r.i32());
  for (Stream &s : out) {
    const int np = r.i32();
    s.end_granule = r.i64();
    for (int k = 0; k < np; k++) s.packets.push_back(r.packet());
  }
  return out;
}

static int run_streams(const char *setup, const char *job, const char *outpath) {
  Setup S(setup);
  const Bound &B = S.B;
  const std::vector<unsigned char> raw = slurp(job);
  Reader r(raw);
  const std::vector<Stream> streams = read_streams(r);
  // the descriptor as a caller of vamd_decode_streams holds it: the packets back to back
  std::vector<unsigned char> bytes;
  std::vector<int64_t> offset = {0}, start = {0}, granule;
  for (const Stream &s : streams) {
    for (const auto &p : s.packets) {
      bytes.insert(bytes.end(), p.begin(), p.end());
      offset.push_back((int64_t)bytes.size());
    }
    start.push_back((int64_t)offset.size() - 1);
    granule.push_back(s.end_granule);
  }
  DecodePlan P;
  std::string err;
  if (!decode_plan_build(B.bs, S.U.modes, S.U.modebits, (int64_t)streams.size(), (int64_t)offset.size() - 1, bytes.data(), offset.data(), start.data(),
                         granule.data(), &P, &err))
    return printf("%s\n", err.c_str()), 2;
  const std::vector<uint32_t> words = as_words(bytes);
  const int ch = B.channels;
  std::vector<float> pcm[2];
  for (int W = 0; W < 2; W++) pcm[W].assign((size_t)P.nblocks[W] * ch * B.bs[W], 0.f);
  std::vector<uint8_t> status = P.status;
  for (size_t s = 0; s < streams.size(); s++)
    for (int64_t k = P.lap_start[s]; k < P.lap_start[s + 1]; k++) {
      const int W = (P.order[(size_t)k] >> 30) & 1, i = P.order[(size_t)k] & 0x3fffffff;
      Rows rows(B, W);
      const int64_t p = P.packet[(size_t)k];
      status[s] |= (uint8_t)unpack(S, words, offset[(size_t)p], offset[(size_t)p + 1], rows);
      std::vector<float> out;
      if (!synth(S, rows, &out)) return printf("not synthesised\n"), 2;
      memcpy(pcm[W].data() + (size_t)i * ch * B.bs[W], out.data(), 4 * out.size());
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
  for (size_t s = 0; s < streams.size(); s++) {
    const int32_t st = status[s], frames = st ? 0 : (int32_t)P.frames[s];
    put(f, &st, 4);
    put(f, &frames, 4);
    std::vector<float> out((size_t)ch * frames);
    const long long k0 = P.lap_start[s], k1 = P.lap_start[s + 1];
    for (long long t = 0; t < frames; t++) {  // (frames > 0: at least two blocks, the first centre at 0)
      const long long k = lap_find(L, k0, k1, t);
      for (int c = 0; c < ch; c++) out[(size_t)c * frames + t] = lap_sample(L, k, t, c);
    }
    put(f, out.data(), 4 * out.size());
  }
  fclose(f);
  return 0;
}

// the bounds synth_block's walk relies on, for rows of a packet that decoded
static bool rows_in_bounds(const Setup &S, Rows &r) {
  const Bound &B = S.B;
  const vamd_setup_header *h = (const vamd_setup_header *)S.image.data();
  const vamd_book_tab *books = (const vamd_book_tab *)(S.image.data() + h->off_books);
  for (int c = 0; c < B.channels; c++)
    if (r.post_valid[(size_t)c] != 0 && r.post_valid[(size_t)c] != 1) return false;
  for (int sm = 0; sm < B.chmap[r.W].submaps; sm++) {
    const ResP &R = B.res[r.W][sm];
    const vamd_residue_tab &t = *R.tab;
    const int slots = r.res_count[2 * (size_t)sm], total = r.res_count[2 * (size_t)sm + 1];
    if (slots < 0 || slots > R.slots || (R.partvals > 0 && slots % R.partvals) || total < 0 || total > R.cap) return false;
    long long e = 0;
    for (int s = 0; s < t.stages; s++)
      for (int q = 0; q < slots; q++) {
        const int c = r.res_class[(size_t)R.cls_base + q];
        if (c < 0 || c >= t.partitions) return false;
        if (!((t.secondstages[c] >> s) & 1) || t.partbooks[c][s] < 0) continue;
        const vamd_book_tab &bk = books[t.partbooks[c][s]];
        for (int v = 0; v < t.grouping / bk.dim; v++, e++)
          if (e < R.cap && r.res_entries[(size_t)R.ent_base + e] >= bk.entries) return false;
      }
    if (e != total) return false;
  }
  return true;
}

static int run_fuzz(const char *setup, const char *job) {
  Setup S(setup);
  const std::vector<unsigned char> raw = slurp(job);
  Reader r(raw);
  const std::vector<Stream> streams = read_streams(r);
  if (streams.empty() || streams[0].packets.empty()) return printf("fuzz: no packets\n"), 2;
  const std::vector<std::vector<unsigned char>> &pk = streams[0].packets;
  long cut = 0, flagged = 0, decoded = 0, walked = 0;
  auto one = [&](const std::vector<unsigned char> &p, int W, int want) {  // -> false: the run has failed
    Rows rows(S.B, W);
    const int st = unpack(S, as_words(p), 0, (long long)p.size(), rows);
    if (want && st != want) return printf("fuzz: a cut packet (%zu bytes) has status %d\n", p.size(), st), false;
    if (st) {
      flagged++;
      if (st & ~(VAMD_STATUS_NOTAUDIO | VAMD_STATUS_BADCODE | VAMD_STATUS_TRUNCATED)) return printf("fuzz: status %d\n", st), false;
      for (int v : rows.post_valid)
        if (v) return printf("fuzz: a flagged packet with a floor\n"), false;
      for (int v : rows.res_count)
        if (v) return printf("fuzz: a flagged packet with a residue\n"), false;
    } else {
      decoded++;
      if (!rows_in_bounds(S, rows)) return printf("fuzz: rows out of bounds (%zu bytes)\n", p.size()), false;
    }
    if ((flagged + decoded) % 16 == 0) {  // the walk itself, on a share of them (a long block is milliseconds here)
      std::vector<float> out;
      if (!synth(S, rows, &out)) return printf("fuzz: not synthesised\n"), false;
      walked++;
    }
    return true;
  };
  auto class_of = [&](const std::vector<unsigned char> &p) {
    const int W = decode_packet_class(p.data(), (int64_t)p.size(), S.U.modes, S.U.modebits);
    return W < 0 ? 0 : W;
  };
  for (const auto &p : pk) {  // every packet at every shorter length
    const int W = class_of(p);
    for (size_t len = 0; len < p.size(); len++, cut++)
      if (!one(std::vector<unsigned char>(p.begin(), p.begin() + (long)len), W, VAMD_STATUS_TRUNCATED)) return 1;
  }
  uint64_t seed = 0x9e3779b97f4a7c15ull;  // fixed: the same cases every run
  auto rnd = [&]() {
    seed ^= seed << 13, seed ^= seed >> 7, seed ^= seed << 17;
    return seed;
  };
  for (int k = 0; k < 3000; k++) {  // single-bit flips, under either size class's rows
    std::vector<unsigned char> p = pk[(size_t)(rnd() % pk.size())];
    const size_t bit = (size_t)(rnd() % (8 * p.size()));
    p[bit >> 3] ^= (unsigned char)(1u << (bit & 7));
    if (!one(p, class_of(p), 0)) return 1;
  }
  for (int k = 0; k < 1000; k++) {  // random bytes
    std::vector<unsigned char> p((size_t)(rnd() % 400));
    for (auto &b : p) b = (unsigned char)rnd();
    if (!p.empty() && (k & 1)) p[0] &= 0xfe;  // (half of them pass for audio)
    if (!one(p, (int)(rnd() & 1) && S.B.bs[0] != S.B.bs[1] ? 1 : 0, 0)) return 1;
  }
  printf("fuzz: %ld cut, %ld flagged, %ld decoded, %ld walked\n", cut, flagged, decoded, walked);
  return 0;
}

// what the test needs of the setup to read `blocks`' output: per size class one line
//   W submaps res_cap | the channels' submaps | per submap: the floor's range, the residue rows' first entry
static int run_info(const char *setup) {
  Setup S(setup);
  const Bound &B = S.B;
  for (int W = 0; W < S.U.modes; W++) {
    printf("%d %d %d |", W, B.chmap[W].submaps, B.res_cap[W]);
    for (int c = 0; c < B.channels; c++) printf(" %d", B.chmap[W].sub[c]);
    printf(" |");
    for (int sm = 0; sm < B.chmap[W].submaps; sm++) printf(" %d %d", B.floor[W][sm].look_n, B.res[W][sm].ent_base);
    printf("\n");
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 3 && !strcmp(argv[1], "info")) return run_info(argv[2]);
  if (argc == 5 && !strcmp(argv[1], "blocks")) return run_blocks(argv[2], argv[3], argv[4]);
  if (argc == 5 && !strcmp(argv[1], "streams")) return run_streams(argv[2], argv[3], argv[4]);
  if (argc == 4 && !strcmp(argv[1], "fuzz")) return run_fuzz(argv[2], argv[3]);
  printf("usage: unpack_host blocks setup job out | streams setup job out | fuzz setup job\n");
  return 2;
}
