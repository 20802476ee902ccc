"""The live feed's walk (k_blockout.h: plan_stream from a carried WalkState, walk_rebase) and the lane's host mirror of a
stream (vamd_feed_host.h: live_piece, live_planned) compiled with the host compiler, for the tests: the shipped headers
themselves, built -ffp-contract=off as the library is.  With the host-compiled stream ends and detector of tests/emul it
chains one stream's live sequence as run_group_live and vamd_live_plan do: the bookkeeping is the mirror's, not restated."""
import ctypes as C

import numpy as np

from tests import hostbuild


_SHIM = r"""
#include <vector>
#include "k_blockout.h"
#include "vamd_feed_host.h"
using namespace vamd;
// one walk over flags[0, nsteps) (mark_at, as k_plan_live applies it), from state[5] = centerW, cursor, curmark, W, lW
// (fresh: a new stream's); the state it ends in is written back.  Returns the number of blocks.
extern "C" int live_walk(const unsigned char *flags, long nsteps, long nsamples, long eof, int bs0, int bs1, long long *state,
                         int fresh, int maxblocks, int *kind, int *begin, long long *pending) {
  BlockoutP B;
  B.bs[0] = bs0, B.bs[1] = bs1;
  blockout_set_step(B, 64);
  B.nsamples = nsamples, B.nsteps = nsteps, B.eof = eof, B.maxblocks = maxblocks;
  const long last = blockout_steps(B);
  std::vector<unsigned char> marks((size_t)nsteps + 4, 0);
  for (long p = 0; p < nsteps + 4; p++) marks[(size_t)p] = (unsigned char)mark_at(flags, last, p);
  WalkState st = walk_fresh(B);
  if (!fresh) st.centerW = state[0], st.cursor = state[1], st.curmark = state[2], st.W = (int)state[3], st.lW = (int)state[4];
  std::vector<PlannedBlock> out((size_t)maxblocks);
  int n0 = 0, n1 = 0;
  long pc = 0;
  const int n = plan_stream(B, marks.data(), out.data(), &n0, &n1, &pc, &st);
  for (int k = 0; k < n; k++) kind[k] = out[(size_t)k].kind, begin[k] = out[(size_t)k].begin;
  state[0] = st.centerW, state[1] = st.cursor, state[2] = st.curmark, state[3] = st.W, state[4] = st.lW;
  *pending = pc;
  return n;
}
extern "C" long live_rebase(int bs0, int bs1, long centerW) {
  BlockoutP B;
  B.bs[0] = bs0, B.bs[1] = bs1;
  blockout_set_step(B, 64);
  return walk_rebase(B, centerW);
}
// the lane's mirror of one stream (vamd_feed_host.h), as run_group_live drives it
extern "C" void *mirror_new() { return new LiveStream(); }
extern "C" void mirror_free(void *m) { delete (LiveStream *)m; }
// the step before the plan -> out[9] = keep, shift, origin, have, kept, c1, c2, n_head, fresh; returns 0, or 1 for the error
extern "C" int mirror_piece(void *m, int bs1, int write_frames, long cs, long long n, int close, long long *out) {
  const LiveShape G(bs1, write_frames, cs);
  LiveIn in;
  vamd_live_geo g;
  int64_t quads = 0;
  if (live_piece(G, *(LiveStream *)m, 0, n, close != 0, in, g, &quads)) return 1;
  out[0] = in.keep, out[1] = in.shift, out[2] = in.origin, out[3] = g.have, out[4] = g.kept, out[5] = g.c1, out[6] = g.c2;
  out[7] = g.n_head, out[8] = in.fresh;
  return 0;
}
// the step after the plan; returns 0, or 1 for the error
extern "C" int mirror_planned(void *m, int closed, long long shift, long retain) {
  return live_planned(*(LiveStream *)m, closed != 0, shift, retain) ? 1 : 0;
}
"""


def build():
    return hostbuild.shim("live", _SHIM)


class LiveWalk:
    def __init__(self, lib, bs):
        self.L = C.CDLL(lib)
        self.L.live_walk.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int,
                                     C.c_void_p, C.c_void_p, C.POINTER(C.c_longlong)]
        self.L.live_rebase.argtypes = [C.c_int, C.c_int, C.c_long]
        self.L.live_rebase.restype = C.c_long
        self.L.mirror_new.restype = C.c_void_p
        self.L.mirror_free.argtypes = [C.c_void_p]
        self.L.mirror_piece.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_long, C.c_longlong, C.c_int, C.c_void_p]
        self.L.mirror_planned.argtypes = [C.c_void_p, C.c_int, C.c_longlong, C.c_long]
        self.bs = bs

    def walk(self, flags, nsamples, state, fresh, eof=0, maxblocks=8192):
        flags = np.ascontiguousarray(flags, np.uint8)
        kind = np.zeros(maxblocks, np.int32)
        begin = np.zeros(maxblocks, np.int32)
        pc = C.c_longlong(0)
        n = self.L.live_walk(flags.ctypes.data, len(flags), nsamples, eof, self.bs[0], self.bs[1], state.ctypes.data, int(fresh),
                             maxblocks, kind.ctypes.data, begin.ctypes.data, C.byref(pc))
        return kind[:n], begin[:n], int(pc.value)

    def rebase(self, centerW):
        return int(self.L.live_rebase(self.bs[0], self.bs[1], centerW))


class Mirror:
    """The shipped host mirror of one live stream (vamd_feed_host.h) in a buffer of cs samples per channel."""
    FIELDS = ("keep", "shift", "origin", "have", "kept", "c1", "c2", "n_head", "fresh")

    def __init__(self, lw, write_frames, cs):
        self.L, self.bs1, self.write_frames, self.cs = lw.L, lw.bs[1], write_frames, cs
        self.m = C.c_void_p(self.L.mirror_new())

    def __del__(self):
        self.L.mirror_free(self.m)

    def piece(self, n, close):
        out = np.zeros(len(self.FIELDS), np.int64)
        assert self.L.mirror_piece(self.m, self.bs1, self.write_frames, self.cs, n, int(close), out.ctypes.data) == 0, \
            "the mirror refuses the piece: it exceeds the buffer"
        return dict(zip(self.FIELDS, (int(v) for v in out)))

    def planned(self, closed, shift, retain):
        assert self.L.mirror_planned(self.m, int(closed), shift, retain) == 0, "the mirror refuses the walk's rebase"


def live_stream(em, lw, pcm, cuts, write_frames):
    """One stream's live sequence on the host, pcm [ch][frames] in pieces `cuts` (the last one closes it): the stream ends
    (tests/emul), the detector over each piece's new steps from its carried state, the resumed walk and the rebase.  What
    the buffer holds, which steps the detector takes, when the head is extrapolated and where the next buffer begins are
    the shipped mirror's answers (Mirror), as on the lane.
    -> its blocks as dicts: kind, begin (absolute), granulepos, eos, pcm [ch][n]."""
    import vorbis_amd
    ch = pcm.shape[0]
    bs1, head, pad, step = lw.bs[1], lw.bs[1] // 2, 3 * lw.bs[1], 64
    cap = head + pcm.shape[1] + pad + 4096
    buf = np.zeros((ch, cap), np.float32)
    mirror = Mirror(lw, write_frames, cap)
    total = 0
    flags = np.zeros(0, np.uint8)
    env = vorbis_amd.EnvelopeState()
    state = np.zeros(5, np.int64)
    fresh = True
    blocks = []
    fp = C.POINTER(C.c_float)

    def detect(first, n):
        return em.envelope_search(np.ascontiguousarray(buf[:, first * step:first * step + (n - 1) * step + 128]), n, env) \
            if n else np.zeros(0, np.uint8)

    for i, n in enumerate(cuts):
        close = i == len(cuts) - 1
        p = mirror.piece(n, close)
        if p["fresh"] and not n:  # (the stream is not there yet: nothing of it is planned)
            continue
        sh, keep, have, origin = p["shift"], p["keep"], p["have"], p["origin"]
        if sh:  # the rebase the last walk asked for, as the ingest and the flag rows carry it out
            buf[:, :cap - sh] = buf[:, sh:].copy()
            buf[:, cap - sh:] = 0
            flags = flags[sh // step:]
        buf[:, keep:keep + n] = pcm[:, total:total + n]
        total += n
        if p["n_head"]:
            for c in range(ch):
                em.L.emul_lpc_head(buf[c].ctypes.data_as(fp), head, p["n_head"])
        flags = np.concatenate([flags, detect(p["kept"], p["c1"])])
        if close:
            _, _, pending = lw.walk(flags, have, state.copy(), fresh)
            for c in range(ch):
                em.L.emul_lpc_tail(buf[c].ctypes.data_as(fp), have, pending - bs1 // 2, bs1, pad)
            f2 = detect(p["kept"] + p["c1"], p["c2"])
            kind, begin, _ = lw.walk(np.concatenate([flags, f2]), have + pad, state, fresh, eof=have)
        else:
            kind, begin, _ = lw.walk(flags, have, state, fresh)
        fresh = False
        for k, b in zip(kind, begin):
            n = lw.bs[int(k) & 1]
            centre = int(b) + n // 2
            blocks.append({"kind": int(k), "begin": origin + int(b), "eos": 0, "pcm": buf[:, int(b):int(b) + n].copy(),
                           "granulepos": (min(centre, have) if close else centre) - head + origin})
        if close:
            mirror.planned(True, 0, cap)
            if blocks:
                blocks[-1]["eos"] = 1
            break
        sh = lw.rebase(int(state[0]))
        assert sh % step == 0 and state[1] >= sh, "the walk's cursor lies in front of the rebased buffer"
        state[:3] -= sh
        mirror.planned(False, sh, cap)
    return blocks
