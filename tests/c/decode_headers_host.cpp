// tests/c/decode_headers_host.cpp -- TEST BUILD ONLY (tests/test_decode_headers_cpu.py; built with -fsanitize=address,undefined).
// vorbis_amd/csrc/vamd_headers.h on the host: a stream's header packets to a decode image, and that image under the one-lane
// build of the decoder (vamd_decode_plan.h, k_unpack.h, k_synth.h with the table form of the residue add where the setup
// has a book that is no lattice book).  Every buffer has exactly the size the GPU launch gives it.
//   decode_headers_host image   id setup blob      the image's decode-side fields against the reference packer's blob
//   decode_headers_host window  n out              the derived rising half window of a block of n samples: float [n/2]
//   decode_headers_host streams id setup job out   job / out as unpack_host's `streams`; two lines of text on stdout first:
//                                                  "books <lattice> <table>" and "lds <bytes W0> <bytes W1> off <ints W0> <ints W1>"
//                                                  (k_synth's LDS per size class, Bound::res_off_ints)
//   decode_headers_host codes   job out            job: int32 ncases | per case: the identification packet, the setup packet
//                                                  (int32 bytes, the bytes padded to 4); out: int32 [ncases] return codes,
//                                                  then per VAMD_EIMPL case its text, a line each, on stdout
//   decode_headers_host ogg     file out           out: int32 code, int64 len[3], the three packets back to back
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "vamd_headers.h"
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
  long long i64() {
    int64_t x;
    take(&x, 8);
    return x;
  }
  // (a packet in a buffer of exactly its size: a read past its end is the sanitiser's to report)
  std::vector<unsigned char> packet() {
    const int n = i32();
    if (n < 0) exit(2);
    std::vector<unsigned char> p((size_t)n);
    take(p.data(), (size_t)n);
    at += (size_t)(-n & 3);
    return p;
  }
};

static void put(FILE *f, const void *p, size_t bytes) {
  if (bytes && fwrite(p, 1, bytes, f) != bytes) {
    printf("cannot write\n");
    exit(2);
  }
}

static int bad;
static void differ(const char *what, int W, int sm) {
  printf("differs: %s (W %d, submap %d)\n", what, W, sm);
  bad++;
}
#define SAME(a, b, what) \
  if (memcmp(&(a), &(b), sizeof(a)) != 0) differ(what, W, sm)

static int run_image(const char *idp, const char *setupp, const char *blobp) {
  const std::vector<unsigned char> id = slurp(idp), setup = slurp(setupp), blob = slurp(blobp);
  HeaderImage H;
  std::string err;
  const int r = headers_to_image(id.data(), id.size(), setup.data(), setup.size(), &H, &err);
  if (r) return printf("headers_to_image: %d %s\n", r, err.c_str()), 1;
  vamd_setup_header a, b;
  if (blob.size() < sizeof(b)) return printf("blob truncated\n"), 2;
  memcpy(&a, H.image.data(), sizeof(a));
  memcpy(&b, blob.data(), sizeof(b));
  int W = -1, sm = -1;
  SAME(a.magic, b.magic, "magic");
  SAME(a.version, b.version, "version");
  SAME(a.channels, b.channels, "channels");
  SAME(a.rate, b.rate, "rate");
  SAME(a.blocksizes, b.blocksizes, "blocksizes");
  SAME(a.modebits, b.modebits, "modebits");
  SAME(a.modes, b.modes, "modes");
  SAME(a.nbooks, b.nbooks, "nbooks");
  for (W = 0; W < 2; W++) {
    const vamd_xform_tab &x = a.xform[W], &y = b.xform[W];
    const int n = y.n;
    SAME(x.n, y.n, "xform n");
    SAME(x.log2n, y.log2n, "xform log2n");
    SAME(x.mdct_scale, y.mdct_scale, "xform mdct_scale");
    if (x.n != y.n) continue;
    if (memcmp(H.image.data() + x.off_mdct_trig, blob.data() + y.off_mdct_trig, 4 * (size_t)(n + n / 4))) differ("the trig table", W, -1);
    if (memcmp(H.image.data() + x.off_mdct_bitrev, blob.data() + y.off_mdct_bitrev, 4 * (size_t)(n / 4))) differ("the bit-reverse table", W, -1);
    if (memcmp(H.image.data() + x.off_window, blob.data() + y.off_window, 4 * (size_t)(n / 2))) differ("the window", W, -1);
    const vamd_mode_tab &m = a.mode[W], &k = b.mode[W];
    SAME(m.submaps, k.submaps, "submaps");
    SAME(m.coupling_steps, k.coupling_steps, "coupling_steps");
    SAME(m.coupling_mag, k.coupling_mag, "coupling_mag");
    SAME(m.coupling_ang, k.coupling_ang, "coupling_ang");
    SAME(m.chmuxlist, k.chmuxlist, "chmuxlist");
    for (sm = 0; sm < k.submaps && sm < VAMD_MAX_SUBMAPS; sm++) {
      const vamd_floor1_tab &f = m.floor[sm], &g = k.floor[sm];
      SAME(f.posts, g.posts, "floor posts");
      SAME(f.quant_q, g.quant_q, "floor quant_q");
      SAME(f.mult, g.mult, "floor mult");
      {  // the range as a decoder holds it: 1 << ilog(look_n - 1), what synth_floor_ranges maps the encoder's to
        int bits = 0;
        for (unsigned v = g.look_n > 0 ? (unsigned)(g.look_n - 1) : 0; v; v >>= 1) bits++;
        const int dec_n = 1 << bits;
        if (f.look_n != dec_n) differ("floor look_n", W, sm);
        // (the encoder's post 1 lies at its look_n, the decoder's at dec_n: the rest of the posts are the same places)
        if (f.postlist[0] != g.postlist[0] || f.postlist[1] != dec_n) differ("floor postlist[0..1]", W, sm);
        if (memcmp(f.postlist + 2, g.postlist + 2, 4 * (size_t)(g.posts - 2))) differ("floor postlist", W, sm);
        if (dec_n == g.look_n) {
          SAME(f.sorted_index, g.sorted_index, "floor sorted_index");
        }
      }
      SAME(f.forward_index, g.forward_index, "floor forward_index");
      SAME(f.reverse_index, g.reverse_index, "floor reverse_index");
      SAME(f.hineighbor, g.hineighbor, "floor hineighbor");
      SAME(f.loneighbor, g.loneighbor, "floor loneighbor");
      SAME(f.partitions, g.partitions, "floor partitions");
      SAME(f.partitionclass, g.partitionclass, "floor partitionclass");
      // (the classes the partitions name; the packer copies all sixteen, the header holds those up to the highest in use)
      for (int i = 0; i < g.partitions; i++) {
        const int c = g.partitionclass[i];
        if (f.class_dim[c] != g.class_dim[c] || f.class_subs[c] != g.class_subs[c] || (g.class_subs[c] && f.class_book[c] != g.class_book[c]))
          differ("floor class", W, sm);
        for (int q = 0; q < (1 << g.class_subs[c]); q++)
          if (f.class_subbook[c][q] != g.class_subbook[c][q]) differ("floor class_subbook", W, sm);
      }
      const vamd_residue_tab &t = a.res[W][sm], &u = b.res[W][sm];
      SAME(t.type, u.type, "residue type");
      SAME(t.begin, u.begin, "residue begin");
      {  // the decoder's clamp of the coded range to the block
        int bundle = 0;
        for (int c = 0; c < b.channels; c++) bundle += k.chmuxlist[c] == sm;
        const int span = (u.type == 2 ? bundle : 1) * (n / 2);
        if (t.end != (u.end < span ? u.end : span)) differ("residue end", W, sm);
      }
      SAME(t.grouping, u.grouping, "residue grouping");
      SAME(t.partitions, u.partitions, "residue partitions");
      SAME(t.stages, u.stages, "residue stages");
      SAME(t.groupbook, u.groupbook, "residue groupbook");
      SAME(t.groupbook_dim, u.groupbook_dim, "residue groupbook_dim");
      if (memcmp(t.secondstages, u.secondstages, 4 * (size_t)u.partitions)) differ("residue secondstages", W, sm);
      if (memcmp(t.partbooks, u.partbooks, sizeof(t.partbooks[0]) * (size_t)u.partitions)) differ("residue partbooks", W, sm);
    }
    sm = -1;
  }
  W = sm = -1;
  if (a.nbooks == b.nbooks) {
    const vamd_book_tab *p = (const vamd_book_tab *)(H.image.data() + a.off_books), *q = (const vamd_book_tab *)(blob.data() + b.off_books);
    for (int i = 0; i < a.nbooks; i++) {
      if (p[i].dim != q[i].dim || p[i].entries != q[i].entries || p[i].minval != q[i].minval || p[i].delta != q[i].delta ||
          p[i].quantvals != q[i].quantvals) {
        printf("book %d: ", i), differ("the book's fields", -1, -1);
        continue;
      }
      if (memcmp(H.image.data() + p[i].off_lengths, blob.data() + q[i].off_lengths, (size_t)q[i].entries)) printf("book %d: ", i), differ("lengths", -1, -1);
      // (a codeword of an unused entry is nobody's to read)
      const uint32_t *x = (const uint32_t *)(H.image.data() + p[i].off_codes), *y = (const uint32_t *)(blob.data() + q[i].off_codes);
      const signed char *len = (const signed char *)(blob.data() + q[i].off_lengths);
      for (int e = 0; e < q[i].entries; e++)
        if (len[e] > 0 && x[e] != y[e]) {
          printf("book %d: ", i), differ("codes", -1, -1);
          break;
        }
    }
  }
  if (H.table_books) printf("%d residue books are not recognised as lattice books\n", H.table_books), bad++;
  if (!H.lattice_books) printf("no residue book\n"), bad++;
  printf("image: %d lattice books, %zu bytes: %s\n", H.lattice_books, H.image.size(), bad ? "FAILED" : "ok");
  return bad ? 1 : 0;
}

static int run_window(const char *ns, const char *outpath) {
  const int n = atoi(ns);
  if (n < 64 || n > 8192 || (n & (n - 1))) return printf("window: n\n"), 2;
  std::vector<float> w;
  header_window(n, &w);
  FILE *f = fopen(outpath, "wb");
  if (!f) return printf("cannot write %s\n", outpath), 2;
  put(f, w.data(), 4 * w.size());
  fclose(f);
  return 0;
}

struct AlignedFloats {
  float *p;
  explicit AlignedFloats(size_t count) {
    p = (float *)aligned_alloc(16, (count * 4 + 15) & ~(size_t)15);
    memset(p, 0, count * 4);
  }
  ~AlignedFloats() { free(p); }
};

static std::vector<uint32_t> as_words(const std::vector<unsigned char> &bytes) {
  std::vector<uint32_t> w((bytes.size() + 3) / 4, 0u);
  if (!bytes.empty()) memcpy(w.data(), bytes.data(), bytes.size());
  return w;
}

static int run_streams(const char *idp, const char *setupp, const char *job, const char *outpath) {
  const std::vector<unsigned char> id = slurp(idp), setup = slurp(setupp);
  HeaderImage H;
  std::string err;
  int r = headers_to_image(id.data(), id.size(), setup.data(), setup.size(), &H, &err);
  if (r) return printf("headers_to_image: %d %s\n", r, err.c_str()), 1;
  printf("books %d %d\n", H.lattice_books, H.table_books);
  Bound B;
  bind_params(H.image, H.derived_off, H.derived, H.image.data(), &B);
  // k_synth's LDS per size class as the library's launch asks for it (vamd_batch.h: synth_lds_bytes), and the offsets row behind it
  printf("lds %zu %zu off %d %d\n", 4 * synth_lds_words(B.channels, B.bs[0] / 2, B.channels, B.res_off_ints[0]),
         4 * synth_lds_words(B.channels, B.bs[1] / 2, B.channels, B.res_off_ints[1]), B.res_off_ints[0], B.res_off_ints[1]);
  std::vector<unsigned char> tab;
  UnpackP U;
  unpack_build_tables(H.image, &tab, &U);
  // (the value lists in a buffer of exactly their size)
  std::vector<float> values(H.values);
  ValueP V = {H.value_off.data(), values.data()};
  const std::vector<unsigned char> raw = slurp(job);
  Reader rd(raw);
  const int nstreams = rd.i32();
  std::vector<unsigned char> bytes;
  std::vector<int64_t> offset = {0}, start = {0}, granule;
  for (int s = 0; s < nstreams; s++) {
    const int np = rd.i32();
    granule.push_back(rd.i64());
    for (int k = 0; k < np; k++) {
      const std::vector<unsigned char> p = rd.packet();
      bytes.insert(bytes.end(), p.begin(), p.end());
      offset.push_back((int64_t)bytes.size());
    }
    start.push_back((int64_t)offset.size() - 1);
  }
  DecodePlan P;
  if (!decode_plan_build(B.bs, U.modes, U.modebits, nstreams, (int64_t)offset.size() - 1, bytes.data(), offset.data(), start.data(), granule.data(), &P, &err))
    return printf("%s\n", err.c_str()), 2;
  const std::vector<uint32_t> words = as_words(bytes);
  const int ch = B.channels;
  std::vector<float> pcm[2];
  for (int W = 0; W < 2; W++) pcm[W].assign((size_t)P.nblocks[W] * ch * B.bs[W], 0.f);
  std::vector<uint8_t> status = P.status;
  for (int s = 0; s < nstreams; s++)
    for (int64_t k = P.lap_start[(size_t)s]; k < P.lap_start[(size_t)s + 1]; k++) {
      const int W = (P.order[(size_t)k] >> 30) & 1, i = P.order[(size_t)k] & 0x3fffffff;
      const int n = B.bs[W], n2 = n / 2, S = B.chmap[W].submaps;
      std::vector<int32_t> post_valid((size_t)ch, 0), res_class((size_t)S * VAMD_RES_CLASS_STRIDE, 0), res_count((size_t)2 * S, 0);
      std::vector<uint32_t> ilog((size_t)ch * n2 / 4, 0);
      std::vector<uint16_t> res_entries((size_t)B.res_cap[W], 0);
      std::vector<int> fit(VAMD_POSIT);
      PhaseClock pc;
      pc.start(nullptr);
      const int64_t p = P.packet[(size_t)k];
      status[(size_t)s] |= (uint8_t)unpack_packet(B, U, words.data(), (long long)words.size(), 8 * offset[(size_t)p], 8 * offset[(size_t)p + 1], W, post_valid.data(),
                                                 (ilog_t *)ilog.data(), res_class.data(), res_entries.data(), res_count.data(), fit.data(), 1, pc);
      SynthFloorP F;
      if (!synth_floor_ranges(B.floor[W][0], B.floor[W][1], S, n2, &F)) return printf("not synthesised\n"), 2;
      AlignedFloats lds(synth_lds_words(ch, n2, 1, B.res_off_ints[W]));
      float *out = pcm[W].data() + (size_t)i * ch * n;
      if (H.table_books)
        synth_block<true>(B.xf[W], B.res[W][0], B.res[W][1], B.chmap[W], B.couple[W], F, ch, B.res_off_ints[W], post_valid.data(), (const ilog_t *)ilog.data(),
                          res_class.data(), res_entries.data(), res_count.data(), lds.p, out, pc, V);
      else
        synth_block(B.xf[W], B.res[W][0], B.res[W][1], B.chmap[W], B.couple[W], F, ch, B.res_off_ints[W], post_valid.data(), (const ilog_t *)ilog.data(),
                    res_class.data(), res_entries.data(), res_count.data(), lds.p, out, pc);
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
    const int32_t st = status[(size_t)s], frames = st ? 0 : (int32_t)P.frames[(size_t)s];
    put(f, &st, 4);
    put(f, &frames, 4);
    std::vector<float> out((size_t)ch * frames);
    const long long k0 = P.lap_start[(size_t)s], k1 = P.lap_start[(size_t)s + 1];
    for (long long t = 0; t < frames; t++) {
      const long long k = lap_find(L, k0, k1, t);
      for (int c = 0; c < ch; c++) out[(size_t)c * frames + t] = lap_sample(L, k, t, c);
    }
    put(f, out.data(), 4 * out.size());
  }
  fclose(f);
  return 0;
}

static int run_codes(const char *job, const char *outpath) {
  const std::vector<unsigned char> raw = slurp(job);
  Reader rd(raw);
  const int ncases = rd.i32();
  std::vector<int32_t> codes;
  for (int k = 0; k < ncases; k++) {
    const std::vector<unsigned char> id = rd.packet(), setup = rd.packet();
    HeaderImage H;
    std::string err;
    // (an empty vector's data() may be null: the parser is handed a packet of no bytes, not no packet)
    static const unsigned char none = 0;
    const int r = headers_to_image(id.empty() ? &none : id.data(), id.size(), setup.empty() ? &none : setup.data(), setup.size(), &H, &err);
    codes.push_back(r);
    if (r == VAMD_EIMPL) printf("%d %s\n", k, err.c_str());
  }
  FILE *f = fopen(outpath, "wb");
  if (!f) return printf("cannot write %s\n", outpath), 2;
  put(f, codes.data(), 4 * codes.size());
  fclose(f);
  return 0;
}

// vamd_ogg_read_headers' body (vamd_decode.h) over demux_read_headers, the file in a buffer of exactly its size
static int run_ogg(const char *file, const char *outpath) {
  const std::vector<unsigned char> f = slurp(file);
  std::vector<uint8_t> copy(f.begin(), f.end()), header[3];
  const int32_t code = demux_read_headers(copy.data(), (int64_t)copy.size(), header) ? 0 : VAMD_EBADHEADER;
  FILE *o = fopen(outpath, "wb");
  if (!o) return printf("cannot write %s\n", outpath), 2;
  put(o, &code, 4);
  for (int k = 0; k < 3; k++) {
    const int64_t n = code ? 0 : (int64_t)header[k].size();
    put(o, &n, 8);
  }
  for (int k = 0; k < 3 && !code; k++) put(o, header[k].data(), header[k].size());
  fclose(o);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 5 && !strcmp(argv[1], "image")) return run_image(argv[2], argv[3], argv[4]);
  if (argc == 4 && !strcmp(argv[1], "window")) return run_window(argv[2], argv[3]);
  if (argc == 6 && !strcmp(argv[1], "streams")) return run_streams(argv[2], argv[3], argv[4], argv[5]);
  if (argc == 4 && !strcmp(argv[1], "codes")) return run_codes(argv[2], argv[3]);
  if (argc == 4 && !strcmp(argv[1], "ogg")) return run_ogg(argv[2], argv[3]);
  printf("usage: decode_headers_host image id setup blob | window n out | streams id setup job out | codes job out | ogg file out\n");
  return 2;
}
