"""The stream walk's mark window (k_blockout.h: MarkWindow, plan_window_min, plan_stream over either mark source) compiled
with the host compiler, for the tests: the shipped header itself, as tests/live_host.py builds it.  The build's
VAMD_WINDOW_CHECK counts the reads that fall outside the window instead of aborting, and the window's buffer has a margin on
both sides so that such a read stays inside the test's own memory."""
import ctypes as C

import numpy as np

from tests import hostbuild


_SHIM = r"""
#include <vector>
static long g_outside = 0;
#define VAMD_WINDOW_CHECK(ok) do { if (!(ok)) g_outside++; } while (0)
#include "k_blockout.h"
using namespace vamd;
static BlockoutP params(long nsteps, long nsamples, long eof, int bs0, int bs1, int maxblocks) {
  BlockoutP B;
  B.bs[0] = bs0, B.bs[1] = bs1;
  blockout_set_step(B, 64);
  B.nsamples = nsamples, B.nsteps = nsteps, B.eof = eof, B.maxblocks = maxblocks;
  return B;
}
// res: blocks, short ones, long ones, pending, centerW, cursor, curmark, W, lW, refills, window in use, reads outside it
static void results(long long *res, int n, int n0, int n1, long pc, const WalkState &st) {
  res[0] = n, res[1] = n0, res[2] = n1, res[3] = pc, res[4] = st.centerW, res[5] = st.cursor, res[6] = st.curmark, res[7] = st.W, res[8] = st.lW;
}
extern "C" long pw_min(int bs0, int bs1) { return plan_window_min(params(0, 0, 0, bs0, bs1, 0)); }
// the one-shot walk over a whole mark array (what k_plan_live and the emulation do)
extern "C" void pw_walk_array(const unsigned char *flags, long nsteps, long nsamples, long eof, int bs0, int bs1, int maxblocks,
                              int *kind, int *begin, long long *res) {
  const BlockoutP B = params(nsteps, nsamples, eof, bs0, bs1, maxblocks);
  const long last = blockout_steps(B);
  std::vector<unsigned char> marks((size_t)nsteps + 4, 0);
  for (long p = 0; p < nsteps + 4; p++) marks[(size_t)p] = (unsigned char)mark_at(flags, last, p);
  std::vector<PlannedBlock> out((size_t)maxblocks);
  WalkState st = walk_fresh(B);
  int n0 = 0, n1 = 0;
  long pc = 0;
  const int n = plan_stream(B, marks.data(), out.data(), &n0, &n1, &pc, &st);
  for (int k = 0; k < n; k++) kind[k] = out[(size_t)k].kind, begin[k] = out[(size_t)k].begin;
  results(res, n, n0, n1, pc, st);
}
// the walk through a window of `window` marks (k_plan_streams): flags of the steps [0, split) in f1, of the rest in f2.
// raw: the window as given, not raised to plan_window_min.  dry: nothing emitted (k_plan_streams' dry run).
extern "C" void pw_walk_window(const unsigned char *f1, long split, const unsigned char *f2, long nsteps, long nsamples, long eof,
                               int bs0, int bs1, int maxblocks, long window, int raw, int dry, int *kind, int *begin, long long *res) {
  const BlockoutP B = params(nsteps, nsamples, eof, bs0, bs1, maxblocks);
  const long size = raw ? window : plan_window_clamp(B, window), margin = 8192;
  std::vector<unsigned char> buf((size_t)(size + 2 * margin), 0);
  std::vector<PlannedBlock> out((size_t)maxblocks);
  g_outside = 0;
  MarkWindow marks;
  marks.open(buf.data() + margin, size, f1, split, f2, blockout_steps(B));
  WalkState st = walk_fresh(B);
  int n0 = 0, n1 = 0;
  long pc = 0;
  const int n = plan_stream(B, marks, dry ? nullptr : out.data(), &n0, &n1, &pc, &st);
  if (!dry)
    for (int k = 0; k < n; k++) kind[k] = out[(size_t)k].kind, begin[k] = out[(size_t)k].begin;
  results(res, n, n0, n1, pc, st);
  res[9] = marks.refills, res[10] = size, res[11] = g_outside;
}
"""


def build():
    return hostbuild.shim("plan_window", _SHIM)


class Walk:
    """A walk's outcome: kind[], begin[] (None for a dry run), and `res` -- see the shim."""
    FIELDS = ("blocks", "short", "long", "pending", "centerW", "cursor", "curmark", "W", "lW")

    def __init__(self, kind, begin, res):
        self.kind, self.begin = kind, begin
        self.res = dict(zip(self.FIELDS, (int(v) for v in res[:9])))
        self.refills, self.window, self.outside = int(res[9]), int(res[10]), int(res[11])


class PlanWindow:
    def __init__(self, lib, bs):
        self.L = C.CDLL(lib)
        vp, ll = C.c_void_p, C.c_long
        self.L.pw_min.argtypes = [C.c_int, C.c_int]
        self.L.pw_min.restype = C.c_long
        self.L.pw_walk_array.argtypes = [vp, ll, ll, ll, C.c_int, C.c_int, C.c_int, vp, vp, vp]
        self.L.pw_walk_array.restype = None
        self.L.pw_walk_window.argtypes = [vp, ll, vp, ll, ll, ll, C.c_int, C.c_int, C.c_int, ll, C.c_int, C.c_int, vp, vp, vp]
        self.L.pw_walk_window.restype = None
        self.bs = bs
        self.minimum = int(self.L.pw_min(bs[0], bs[1]))

    def array(self, flags, nsamples, eof=0, maxblocks=16384):
        flags = np.ascontiguousarray(flags, np.uint8)
        kind, begin, res = np.zeros(maxblocks, np.int32), np.zeros(maxblocks, np.int32), np.zeros(12, np.int64)
        self.L.pw_walk_array(flags.ctypes.data, len(flags), nsamples, eof, self.bs[0], self.bs[1], maxblocks, kind.ctypes.data,
                             begin.ctypes.data, res.ctypes.data)
        n = int(res[0])
        return Walk(kind[:n], begin[:n], res)

    def window(self, flags, nsamples, window, eof=0, split=None, raw=False, dry=False, maxblocks=16384):
        flags = np.ascontiguousarray(flags, np.uint8)
        split = len(flags) if split is None else split
        # two arrays of their own, each with nothing of the other behind or in front of it
        f1, f2 = np.ascontiguousarray(flags[:split].copy()), np.ascontiguousarray(flags[split:].copy())
        f1, f2 = (np.concatenate([f, np.zeros(1, np.uint8)]) for f in (f1, f2))
        kind, begin, res = np.zeros(maxblocks, np.int32), np.zeros(maxblocks, np.int32), np.zeros(12, np.int64)
        self.L.pw_walk_window(f1.ctypes.data, split, f2.ctypes.data, len(flags), nsamples, eof, self.bs[0], self.bs[1], maxblocks,
                              window, int(raw), int(dry), kind.ctypes.data, begin.ctypes.data, res.ctypes.data)
        n = int(res[0])
        return Walk(None if dry else kind[:n], None if dry else begin[:n], res)
