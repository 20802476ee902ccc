// tests/c/demux_host.cpp -- TEST BUILD ONLY (tests/test_demux_cpu.py; built with -fsanitize=address,undefined).
// The Ogg decode entry's way from files to packets on the host: the shipped scan (vorbis_amd/csrc/vamd_demux.h), the block
// plan over its packet table (vamd_decode_plan.h, the first bytes handed over as the library hands them), and k_ogg_depage's
// body (k_demux.h) with its lanes in turn -- 64 of them as the GPU has, and one -- over the page table.  Every buffer has
// exactly the size the library gives it: the group's files back to back with nothing behind them for the scan, and each
// file once more ALONE in a buffer of its own length (a read outside the file is the sanitiser's to report; the status
// must not depend on the neighbours); the upload rounded up to a dword + 16 and the arena exactly its bytes for the depage.
//   demux_host scan setup job out   job: int32 nstreams, int32 setup_header_bytes, the setup header (padded to 4), per stream:
//                                        int64 bytes, the file (padded to 4)
//                                   out, per stream: int32 status (the scan's | its pages'), int64 end granule, int32 frames
//                                        (the plan's), int32 npackets, int32 sizes[npackets], the packets (padded to 4)
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include "vamd_bind.h"
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
  template <class T>
  T get() {
    T x;
    take(&x, sizeof(T));
    return x;
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
};

static void put(FILE *f, const void *p, size_t bytes) {
  if (bytes && fwrite(p, 1, bytes, f) != bytes) {
    printf("cannot write\n");
    exit(2);
  }
}

static int run_scan(const char *setup, const char *job, const char *outpath) {
  const std::vector<unsigned char> blob = slurp(setup);
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

  const std::vector<unsigned char> raw = slurp(job);
  Reader r(raw);
  const int ns = r.get<int32_t>(), hb = r.get<int32_t>();
  if (ns < 0 || hb < 0) return printf("job: counts\n"), 2;
  Exact header((size_t)hb);
  r.bytes(header.p, hb);
  std::vector<int64_t> off = {0};
  const size_t files_at = r.at;
  for (int s = 0; s < ns; s++) {  // (a first pass for the sizes: the group's buffer is exactly their sum)
    const int64_t n = r.get<int64_t>();
    if (n < 0) return printf("job: a file's size\n"), 2;
    off.push_back(off.back() + n);
    r.at += (size_t)((n + 3) & ~(int64_t)3);
  }
  const int64_t total = off.back();
  Exact files((size_t)total);
  r.at = files_at;
  for (int s = 0; s < ns; s++) {
    r.get<int64_t>();
    r.bytes(files.p + off[(size_t)s], off[(size_t)s + 1] - off[(size_t)s]);
  }
  DemuxSetup S;
  S.channels = B.channels, S.rate = B.rate, S.bs[0] = B.bs[0], S.bs[1] = B.bs[1];
  S.setup_header = hb ? header.p : nullptr, S.setup_header_bytes = hb;
  DemuxScan X;
  if (!demux_scan(ns, files.p, off.data(), S, &X, &err)) return printf("%s\n", err.c_str()), 2;
  // each file alone: the same status, the same packets, the same pages
  for (int s = 0; s < ns; s++) {
    const int64_t n = off[(size_t)s + 1] - off[(size_t)s];
    Exact one((size_t)n);
    if (n) memcpy(one.p, files.p + off[(size_t)s], (size_t)n);
    DemuxScan Y;
    Y.offset.push_back(0);
    const uint8_t st = demux_scan_file(n ? one.p : nullptr, n, 0, 0, S, &Y);
    const size_t p0 = (size_t)X.stream_start[(size_t)s], p1 = (size_t)X.stream_start[(size_t)s + 1];
    bool same = st == X.status[(size_t)s] && Y.first.size() == p1 - p0 && Y.end_granule[0] == X.end_granule[(size_t)s] &&
                Y.pages.size() == (size_t)(X.page_start[(size_t)s + 1] - X.page_start[(size_t)s]);
    for (size_t p = p0; same && p < p1; p++)
      same = Y.first[p - p0] == X.first[p] && Y.offset[p - p0 + 1] - Y.offset[p - p0] == X.offset[p + 1] - X.offset[p];
    if (!same) return printf("stream %d: the scan of the file alone differs from its scan in the group\n", s), 1;
  }
  DecodePlan P;
  if (!decode_plan_build(B.bs, U.modes, U.modebits, ns, (int64_t)X.first.size(), nullptr, X.offset.data(), X.stream_start.data(), X.end_granule.data(), &P,
                         &err, X.first.data()))
    return printf("%s\n", err.c_str()), 2;
  // the depage: the upload as the library sizes it, the arena exactly its bytes
  std::vector<uint32_t> upload((size_t)(total + 3) / 4 + 4, 0xa5a5a5a5u);
  if (total) memcpy(upload.data(), files.p, (size_t)total);
  const int64_t nbytes = X.offset.back();
  Exact arena((size_t)nbytes), arena1((size_t)nbytes);
  memset(arena.p, 0xee, (size_t)nbytes), memset(arena1.p, 0x11, (size_t)nbytes);
  std::vector<uint8_t> status = X.status;
  for (const OggDepage &pg : X.pages) {
    const uint8_t a = ogg_depage_host((const uint8_t *)upload.data(), total, pg, arena.p, nbytes, 64);
    const uint8_t b = ogg_depage_host((const uint8_t *)upload.data(), total, pg, arena1.p, nbytes, 1);
    if (a != b) return printf("a page's status differs between 64 lanes and one\n"), 1;
    status[(size_t)pg.stream] |= a;
  }
  if (nbytes && memcmp(arena.p, arena1.p, (size_t)nbytes) != 0) return printf("the arena differs between 64 lanes and one\n"), 1;
  FILE *f = fopen(outpath, "wb");
  if (!f) return printf("cannot write %s\n", outpath), 2;
  for (int s = 0; s < ns; s++) {
    const int32_t st = status[(size_t)s] | P.status[(size_t)s], frames = (int32_t)P.frames[(size_t)s];
    const int64_t p0 = X.stream_start[(size_t)s], p1 = X.stream_start[(size_t)s + 1], end = X.end_granule[(size_t)s];
    const int32_t np = (int32_t)(p1 - p0);
    put(f, &st, 4), put(f, &end, 8), put(f, &frames, 4), put(f, &np, 4);
    for (int64_t p = p0; p < p1; p++) {
      const int32_t n = (int32_t)(X.offset[(size_t)p + 1] - X.offset[(size_t)p]);
      put(f, &n, 4);
    }
    const int64_t b0 = X.offset[(size_t)p0], b1 = X.offset[(size_t)p1];
    put(f, arena.p + b0, (size_t)(b1 - b0));
    const char pad[4] = {0, 0, 0, 0};
    put(f, pad, (size_t)(-(b1 - b0) & 3));
  }
  fclose(f);
  return 0;
}

int main(int argc, char **argv) {
  if (argc == 5 && !strcmp(argv[1], "scan")) return run_scan(argv[2], argv[3], argv[4]);
  printf("usage: demux_host scan setup job out\n");
  return 2;
}
