// tests/c/demux_live_host.cpp -- TEST BUILD ONLY (tests/test_demux_live_cpu.py; built with -fsanitize=address,undefined).
// The live Ogg decoder for one lane on the host, call after call on one decoder as vamd_decode_ogg_live_wrote sequences
// them: the shipped walk (vorbis_amd/csrc/vamd_demux_live.h), the live block plan over its packet table with the first
// bytes handed over (vamd_decode_live_plan.h), the bodies of k_ogg_packet_carry_in, k_ogg_depage and k_ogg_packet_carry_out
// (k_demux.h) with 64 lanes in turn and once more with one, then unpack_packet, synth_block, the two lap carries and
// lap_sample as tests/c/decode_live_host.cpp runs them.  Every buffer has exactly the size the launch gives it -- the
// pieces exactly their bytes, the upload rounded up to a dword + 16, the arena its dwords + 16, the byte carry exactly
// [max_streams][stride] -- so that a read or write beyond one is the sanitiser's to report.
// A packet's unpack + synth is kept by its bytes as they came out of the arena (that stage is tests/test_decode_live_cpu.py's
// to test, and thousands of cut lists decode the same packets); the carries, the plan and the lap run every time.
//   demux_live_host setup job out
//     job: int32 max_streams, hb, the setup header (padded to 4), int64 max_packet_bytes, max_header_bytes, int32 nrefs, nruns
//          per ref (what a stream must come to, from the independent reader and the reference decoder): int32 np,
//            int32 sizes[np], the packets (padded to 4), int64 end granule, int32 frames, float [ch][frames]
//          per run (a fresh decoder): int32 compact, ncalls, nexp, per expectation int32 slot, ref
//            per call: int32 nstreams, nullmask (bit 0 slot, 1 bytes, 2 piece_offset, 3 close: the pointer is NULL), three
//            arrays, each int32 count + int64 elements: slot, piece_offset, close; int32 nbytes and the bytes (padded to 4)
//     out: a full run (compact = 0): per call int32 ok; a refused call has 0 and nothing else, and changes nothing; a call
//            that ran has 1, then per stream int32 status, frames, int64 end granule (what cut the last block in this call,
//            else -1), int32 carry_in, carry_out (the byte-carry rows' lengths, 0: none), int32 np, sizes[np], the packets
//            as they lie in the arena (padded to 4), float [ch][frames]
//          a compact run: int32 refused calls, int32 largest carry_out row, per expectation int32 verdict: bit 0 a status,
//            1 the packets differ, 2 the end granule differs, 3 the samples differ
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <string>
#include <vector>
#include "vamd_bind.h"
#include "k_synth.h"
#include "k_unpack.h"
#include "vamd_decode_live_plan.h"
#include "vamd_demux_live.h"

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

// exactly n bytes (16-byte aligned, as device memory is), freed with the scope
struct Exact {
  unsigned char *p;
  size_t n;
  explicit Exact(size_t n_, int fill = 0) : n(n_) {
    p = (unsigned char *)malloc(n ? n : 1);
    if (n) memset(p, fill, n);
  }
  ~Exact() { free(p); }
  Exact(const Exact &) = delete;
};

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
static void put32(FILE *f, int32_t v) { put(f, &v, 4); }

struct Ref {
  std::vector<std::string> packets;
  int64_t end = -1;
  int32_t frames = 0;
  std::vector<float> pcm;
};
struct Got {  // what a slot's stream has come to in a compact run
  std::vector<std::string> packets;
  int64_t end = -1;
  std::vector<std::vector<float>> pcm;  // per channel
  int status = 0;
};
struct Block {
  uint8_t status;
  std::vector<float> v;
};

int main(int argc, char **argv) {
  if (argc != 4) return printf("usage: demux_live_host setup job out\n"), 2;
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
  const int max_streams = r.i32(), hb = r.i32();
  if (max_streams < 1 || hb < 0) return printf("job: counts\n"), 2;
  Exact header((size_t)hb);
  r.bytes(header.p, hb);
  const int64_t max_packet_bytes = r.i64(), max_header_bytes = r.i64();
  const int64_t stride = (max_packet_bytes + 3) & ~(int64_t)3;
  const int nrefs = r.i32(), nruns = r.i32();
  std::vector<Ref> refs((size_t)nrefs);
  for (Ref &R : refs) {
    const int np = r.i32();
    std::vector<int32_t> sizes((size_t)np);
    r.take(sizes.data(), 4 * sizes.size());
    int64_t sum = 0;
    for (int32_t v : sizes) sum += v;
    std::vector<unsigned char> all((size_t)sum);
    r.bytes(all.data(), sum);
    int64_t at = 0;
    for (int32_t v : sizes) R.packets.emplace_back((const char *)all.data() + at, (size_t)v), at += v;
    R.end = r.i64(), R.frames = r.i32();
    R.pcm.resize((size_t)ch * R.frames);
    r.take(R.pcm.data(), 4 * R.pcm.size());
  }
  DemuxSetup S;
  S.channels = B.channels, S.rate = B.rate, S.bs[0] = B.bs[0], S.bs[1] = B.bs[1];
  S.setup_header = hb ? header.p : nullptr, S.setup_header_bytes = hb;
  std::map<std::string, Block> memo;
  const float nan = nanf("");
  for (int run = 0; run < nruns; run++) {
    const int compact = r.i32(), ncalls = r.i32(), nexp = r.i32();
    std::vector<int> exp_slot, exp_ref;
    for (int e = 0; e < nexp; e++) exp_slot.push_back(r.i32()), exp_ref.push_back(r.i32());
    std::vector<LiveSlot> slots((size_t)max_streams);
    std::vector<DemuxLiveSlot> demux((size_t)max_streams);
    AlignedFloats carry((size_t)max_streams * ch * (B.bs[1] / 2));
    Exact bcarry((size_t)max_streams * (size_t)stride, 0xcc), bcarry1((size_t)max_streams * (size_t)stride, 0x33);
    std::vector<Got> got((size_t)max_streams);
    int32_t refused = 0, largest = 0;
    for (int call = 0; call < ncalls; call++) {
      const int64_t ns = r.i32();
      const int nullmask = r.i32();
      const std::vector<int64_t> slot = r.i64s(), off = r.i64s(), close64 = r.i64s();
      std::vector<uint8_t> close(close64.begin(), close64.end());
      const int nbytes = r.i32();
      if (nbytes < 0) return 2;
      Exact bytes((size_t)nbytes);
      r.bytes(bytes.p, nbytes);
      auto ptr = [&](int bit, const auto &v) { return (nullmask >> bit) & 1 ? nullptr : v.data(); };
      const uint8_t *closep = ptr(3, close);
      DemuxLiveCall X;
      DecodeLivePlan L;
      bool ok = demux_live_scan(demux, ns, ptr(0, slot), (nullmask >> 1) & 1 ? nullptr : bytes.p, ptr(2, off), closep, S, max_packet_bytes, max_header_bytes,
                                &X, &err);
      if (ok)
        ok = decode_live_plan_build(B.bs, U.modes, U.modebits, slots, ns, (int64_t)X.X.first.size(), slot.data(), nullptr, X.X.offset.data(),
                                    X.X.stream_start.data(), X.close.data(), X.X.end_granule.data(), &L, &err, X.X.first.data());
      if (!ok) {
        if (!compact) put32(f, 0), printf("run %d call %d refused: %s\n", run, call, err.c_str());
        refused++;
        continue;
      }
      const DecodePlan &P = L.P;
      std::vector<uint8_t> status(P.status);
      for (int64_t s = 0; s < ns; s++) status[(size_t)s] |= X.X.status[(size_t)s];
      // the upload and the arena as decode_run sizes them; the three launches, 64 lanes and one
      const int64_t up = (int64_t)X.upload.size(), nbytes_arena = X.arena_bytes;
      Exact upload((size_t)((up + 3) & ~(int64_t)3) + 16, 0xa5);
      if (up) memcpy(upload.p, X.upload.data(), (size_t)up);
      const size_t arena_size = (size_t)((nbytes_arena + 3) / 4) * 4 + 16;
      Exact arena(arena_size, 0xee), arena1(arena_size, 0xee);
      for (const OggCarryRow &row : X.in)
        if (!ogg_packet_carry_host(false, row, arena.p, nbytes_arena, bcarry.p, max_streams, stride, 64) ||
            !ogg_packet_carry_host(false, row, arena1.p, nbytes_arena, bcarry1.p, max_streams, stride, 1))
          return printf("a carry-in row outside its buffers\n"), 1;
      for (const OggDepage &pg : X.X.pages) {
        const uint8_t a = ogg_depage_host(upload.p, up, pg, arena.p, nbytes_arena, 64), b = ogg_depage_host(upload.p, up, pg, arena1.p, nbytes_arena, 1);
        if (a != b) return printf("a page's status differs between 64 lanes and one\n"), 1;
        if (a == OGG_DEPAGE_BADROW) return printf("a page row outside its buffers\n"), 1;
        status[(size_t)pg.stream] |= a;
      }
      for (const OggCarryRow &row : X.out)
        if (!ogg_packet_carry_host(true, row, arena.p, nbytes_arena, bcarry.p, max_streams, stride, 64) ||
            !ogg_packet_carry_host(true, row, arena1.p, nbytes_arena, bcarry1.p, max_streams, stride, 1))
          return printf("a carry-out row outside its buffers\n"), 1;
      if (memcmp(arena.p, arena1.p, arena_size) != 0) return printf("the arena differs between 64 lanes and one\n"), 1;
      for (const OggCarryRow &row : X.out)
        if (memcmp(bcarry.p + row.slot * stride, bcarry1.p + row.slot * stride, (size_t)row.len) != 0) return printf("the carry differs between 64 lanes and one\n"), 1;
      std::vector<int32_t> cin((size_t)max_streams, 0), cout((size_t)max_streams, 0);
      for (const OggCarryRow &row : X.in) cin[(size_t)row.slot] = row.len;
      for (const OggCarryRow &row : X.out) cout[(size_t)row.slot] = row.len, largest = std::max(largest, row.len);
      // k_unpack + k_synth per planned packet, out of the arena at the places the plan's upload gives them
      AlignedFloats synth0((size_t)(P.nblocks[0] + P.extra[0]) * ch * B.bs[0], nan), synth1((size_t)(P.nblocks[1] + P.extra[1]) * ch * B.bs[1], nan);
      const uint32_t *words = (const uint32_t *)arena.p;
      const long long nwords = (long long)((nbytes_arena + 3) / 4);
      for (int64_t s = 0; s < ns; s++)
        for (int64_t k = L.unpack_start[(size_t)s]; k < L.unpack_start[(size_t)s + 1]; k++) {
          const int W = (L.unpack[(size_t)k] >> 30) & 1, i = L.unpack[(size_t)k] & 0x3fffffff;
          const int n = B.bs[W], n2 = n / 2, Sm = B.chmap[W].submaps;
          const int64_t p = P.packet[(size_t)k], at = X.begin[(size_t)p], len = X.X.offset[(size_t)p + 1] - X.X.offset[(size_t)p];
          std::string key(1, (char)W);
          key.append((const char *)arena.p + at, (size_t)len);
          auto it = memo.find(key);
          if (it == memo.end()) {
            std::vector<int32_t> post_valid((size_t)ch, 0), res_class((size_t)Sm * VAMD_RES_CLASS_STRIDE, 0), res_count((size_t)2 * Sm, 0);
            std::vector<uint32_t> ilog_words((size_t)ch * n2 / 4, 0);
            std::vector<uint16_t> res_entries((size_t)B.res_cap[W], 0);
            std::vector<int> fit(VAMD_POSIT);
            PhaseClock pc;
            pc.start(nullptr);
            Block blk;
            blk.v.assign((size_t)ch * n, nan);
            blk.status = (uint8_t)unpack_packet(B, U, words, nwords, 8 * at, 8 * (at + len), W, post_valid.data(), (ilog_t *)ilog_words.data(), res_class.data(),
                                                res_entries.data(), res_count.data(), fit.data(), 1, pc);
            AlignedFloats lds(synth_lds_words(ch, n2, 1, B.res_off_ints[W])), one((size_t)ch * n, nan);
            synth_block(B.xf[W], B.res[W][0], B.res[W][1], B.chmap[W], B.couple[W], F[W], ch, B.res_off_ints[W], post_valid.data(), (ilog_t *)ilog_words.data(),
                        res_class.data(), res_entries.data(), res_count.data(), lds.p, one.p, pc);
            memcpy(blk.v.data(), one.p, 4 * blk.v.size());
            it = memo.emplace(key, std::move(blk)).first;
          }
          status[(size_t)s] |= it->second.status;
          memcpy((W ? synth1.p : synth0.p) + (size_t)i * ch * n, it->second.v.data(), 4 * it->second.v.size());
        }
      CarryP C;
      C.ch = ch, C.bs0 = B.bs[0], C.bs1 = B.bs[1], C.carry = carry.p, C.synth0 = synth0.p, C.synth1 = synth1.p;
      for (const CarryRow &row : L.in)
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
      if (!compact) put32(f, 1);
      for (int64_t s = 0; s < ns; s++) {
        const int32_t st = status[(size_t)s], frames = st ? 0 : (int32_t)P.frames[(size_t)s];
        std::vector<float> out((size_t)ch * frames);
        const long long k0 = P.lap_start[(size_t)s], k1 = P.lap_start[(size_t)s + 1];
        if (frames > 0) {  // k_lap's walk of a stream
          if (k1 - k0 < 2) return printf("run %d call %d stream %lld: frames without two blocks\n", run, call, (long long)s), 2;
          const long long first = lap_centre(Lp, k0), span = lap_centre(Lp, k1 - 1) - first;
          if (frames > span) return printf("run %d call %d stream %lld: more frames than the centres span\n", run, call, (long long)s), 2;
          for (long long t = 0; t < frames; t++) {
            const long long k = lap_find(Lp, k0, k1, first + t);
            for (int c = 0; c < ch; c++) out[(size_t)c * frames + t] = lap_sample(Lp, k, first + t, c);
          }
        }
        const int64_t p0 = X.X.stream_start[(size_t)s], p1 = X.X.stream_start[(size_t)s + 1], end = X.X.end_granule[(size_t)s];
        if (compact) {
          Got &G = got[(size_t)slot[(size_t)s]];
          G.status |= st;
          G.pcm.resize((size_t)ch);
          for (int64_t p = p0; p < p1 && !st; p++) G.packets.emplace_back((const char *)arena.p + X.begin[(size_t)p], (size_t)(X.X.offset[(size_t)p + 1] - X.X.offset[(size_t)p]));
          if (end >= 0) G.end = end;
          for (int c = 0; c < ch; c++) G.pcm[(size_t)c].insert(G.pcm[(size_t)c].end(), out.begin() + (size_t)c * frames, out.begin() + (size_t)(c + 1) * frames);
          continue;
        }
        put32(f, st), put32(f, frames), put(f, &end, 8);
        put32(f, cin[(size_t)slot[(size_t)s]]), put32(f, cout[(size_t)slot[(size_t)s]]);
        put32(f, (int32_t)(p1 - p0));
        int64_t sum = 0;
        for (int64_t p = p0; p < p1; p++) put32(f, (int32_t)(X.X.offset[(size_t)p + 1] - X.X.offset[(size_t)p]));
        for (int64_t p = p0; p < p1; p++) {
          const int64_t len = X.X.offset[(size_t)p + 1] - X.X.offset[(size_t)p];
          put(f, arena.p + X.begin[(size_t)p], (size_t)len), sum += len;
        }
        const char pad[4] = {0, 0, 0, 0};
        put(f, pad, (size_t)(-sum & 3));
        put(f, out.data(), 4 * out.size());
      }
      decode_live_commit(&slots, L, ns, slot.data(), X.close.data(), status.data());
      demux_live_commit(&demux, &X, ns, slot.data(), closep, status.data());
    }
    if (compact) {
      put32(f, refused), put32(f, largest);
      for (int e = 0; e < nexp; e++) {
        const Got &G = got[(size_t)exp_slot[(size_t)e]];
        const Ref &R = refs[(size_t)exp_ref[(size_t)e]];
        int32_t verdict = (G.status ? 1 : 0) | (G.packets != R.packets ? 2 : 0) | (G.end != R.end ? 4 : 0);
        bool same = G.pcm.size() == (size_t)ch || R.frames == 0;
        for (int c = 0; same && c < ch && R.frames; c++)
          same = G.pcm[(size_t)c].size() == (size_t)R.frames && memcmp(G.pcm[(size_t)c].data(), R.pcm.data() + (size_t)c * R.frames, 4 * (size_t)R.frames) == 0;
        if (R.frames == 0)
          for (const auto &row : G.pcm) same = same && row.empty();
        put32(f, verdict | (same ? 0 : 8));
      }
    }
  }
  fclose(f);
  return 0;
}
