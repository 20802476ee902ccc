"""Groups of hundreds of streams for the feed's tests (tests/test_feed_many_streams.py on the GPU,
tests/test_feed_many_cases_cpu.py without one): `count` streams made from D distinct ones dealt round, as
decode_cases.short_streams does for the decoder, so that the reference runs D times however large the group is.

D = 23: odd and no divisor of 64 or 1024, so neighbours always differ and a stride of 64 (a wave) or 1024 (k_feed_scan's
and k_lap's workgroup) never lands on a copy of the same stream.  A stream's expectation is the reference's for that
stream alone (tests/test_feed.py::test_streams_of_unequal_length_in_one_group holds the feed to that contract).

What each group exists for -- the switch it takes the feed across -- is computed here twice: conditions_of() from the
reference's records alone (the CPU test: an edit of the signals cannot make the GPU ids vacuous unnoticed), and by every
GPU id from its own inputs and results."""
import numpy as np

from tests import checker, ref_host
from tests.decode_cases import END_COUNTS_9000
from tests.feed_cases import planar
from tests.signals import MANAGED_RATES, gated, s16_streams
from tests.soak_lib import MANAGED
from tests.synth_host import SHORT_LENGTHS

D = 23
KINDS = ("noise", "gated", "sine", "clicks", "silence")
SETUP = "44k_stereo_q4"
HEAD, PAD, SEARCHSTEP, VE_WIN = 1024, 6144, 64, 4   # blocksizes[1] / 2, 3 * blocksizes[1], the detector's step and window
# The switches the groups are sized for; the tests assert them as literals, each mirroring one source line:
#   65 536      vamd_plan.h, envelope_search_batch: `big = nstreams * nsteps > 65536` (k_env_amp_tiled, k_env_bits_tiled)
#   1024        k_feed.h, k_feed_scan: __launch_bounds__(1024), per = ceil(ns / 1024); k_synth.h, k_lap: 1024 rows, strided beyond
#   8192 x 256  vamd_feed_ingest.h, launch_ingest: `if (blocks > 256L * 32) blocks = 256L * 32`, workgroups of 256 threads
#   2048        vamd_knobs.h: res_team_max = pack_pair_max = 2048 units; feed_slice = 2048 blocks
BATCH_UNITS = 2048

# the eight of SHORT_LENGTHS, the end counts of decode_cases (not multiples of four among them), and what lies between
SHORT = tuple(SHORT_LENGTHS) + tuple(sorted(set(END_COUNTS_9000))) + (100, 700, 1500, 2500, 3071, 3072, 4097, 5000, 6001, 8190)
# under one detector window: two packets each, whatever the signal
TINY = (1, 2, 3, 5, 8, 13, 20, 21, 33, 34, 47, 55, 63, 64, 65, 77, 89, 96, 100, 111, 120, 127, 128)
# the benchmark's shape in miniature: up to about 46 000 frames
LONG = (46001, 44100, 41003, 39999, 37002, 35001, 33333, 31001, 29002, 27003, 25001, 23002, 21003, 19001, 17002, 15003, 13001, 11002,
        9003, 7001, 5002, 3073, 1)
LONG_KINDS = ("gated", "clicks", "noise", "gated", "clicks", "sine", "gated", "clicks", "gated", "clicks", "silence", "gated", "clicks",
              "noise", "gated", "clicks", "gated", "sine", "clicks", "gated", "clicks", "gated", "noise")
# one length for all: silence once (two silent streams of one length would be the same stream), gated in its other places
UNIFORM_KINDS = ("noise", "gated", "sine", "clicks", "silence", "noise", "gated", "sine", "clicks", "gated", "noise", "gated", "sine",
                 "clicks", "gated", "noise", "gated", "sine", "clicks", "gated", "noise", "gated", "sine")
UNIFORM = 4099             # not a multiple of 4; (1024 + 4099) / 64 - 4 = 76 steps: 76 % 32 = 12, the last detector tile ragged
assert len(SHORT) == len(set(SHORT)) == D and len(TINY) == len(set(TINY)) == D and len(LONG) == len(set(LONG)) == D == len(LONG_KINDS)
assert D % 2 == 1 and 64 % D and 1024 % D

_groups, _cache = {}, {}


def steps_of(frames):
    """-> (steps of the first detector pass, steps of the second) of a whole stream: vamd_plan.h, plan_streams"""
    s1 = max((HEAD + frames) // SEARCHSTEP - VE_WIN, 0)
    return s1, max((HEAD + frames + PAD) // SEARCHSTEP - VE_WIN, s1) - s1


def ingest_items(ns, frames):
    """vamd_feed_ingest.h, run_group: ns * (head / 4 + ceil(frames / 4) + pad / 4), frames the group's longest"""
    return ns * (HEAD // 4 + (frames + 3) // 4 + PAD // 4)


class Many:
    """distinct: the D (or, joined, more) distinct streams [frames, ch] int16; index[s]: which of them stream s is"""

    def __init__(self, name, distinct, index, key):
        self.name, self.distinct, self.index, self.key = name, distinct, [int(i) for i in index], key
        self.ch, self.rate, self.q = checker.SETUPS[name]
        self.count = len(self.index)
        self.frames = [len(self.distinct[d]) for d in self.index]

    def parts(self, dtype=np.int16):
        """per stream [frames, ch]: the 16-bit samples, or the float32 an application makes of them (x / 32768)"""
        if dtype == np.int16:
            return [self.distinct[d] for d in self.index]
        f = self._once("f32", lambda d: np.ascontiguousarray(planar(self.distinct[d]).T))
        return [f[d] for d in self.index]

    def _once(self, what, make):
        k = (self.key, what)
        if k not in _cache:
            _cache[k] = [make(d) for d in range(len(self.distinct))]
        return _cache[k]

    # ---- the reference, once per distinct stream ----
    def records(self, managed=None, quantise=None):
        """per DISTINCT stream the reference encoder's records (tests/feed_cases.py: reference_records); quantise: (a name
        for the cache, a function float32 [ch, frames] -> float32): what a half-precision source makes of the samples"""
        from oracle import ref

        def make(d):
            x = planar(self.distinct[d])
            if quantise is not None:
                x = np.ascontiguousarray(quantise[1](x), np.float32)
            enc = ref.RefEncoder(self.ch, self.rate, managed=managed) if managed else ref.RefEncoder(self.ch, self.rate, self.q)
            return enc.encode_stream(x)
        return self._once(("records", managed, quantise[0] if quantise else None), make)

    def rows(self, managed=None, quantise=None):
        """records() as the rows a feed returns: (bytes, granulepos, W, e_o_s) per packet"""
        recs = self.records(managed, quantise)
        return self._once(("rows", managed, quantise[0] if quantise else None),
                          lambda d: [(w["packet"], w["granulepos"], w["W"], w["eos"]) for w in recs[d]])

    def headers(self):
        """the three header packets of the setup's encoder (the reference's)"""
        return _headers(self.name)

    def decoded(self):
        """per DISTINCT stream the reference decoder's signal of the reference encoder's packets, float32 [ch, frames]"""
        rows, headers = self.rows(), _headers(self.name)

        def make(d):
            w = ref_host.reference_decode(headers + [r[0] for r in rows[d]], [r[1] for r in rows[d]])
            w.setflags(write=False)
            return w
        return self._once("decoded", make)

    # ---- what the group is for, from the reference alone ----
    def packets_of(self, managed=None):
        rows = self.rows(managed)
        return [len(rows[d]) for d in self.index]

    def class_counts(self, managed=None):
        """-> (short blocks, long blocks) of the whole group"""
        rows = self.rows(managed)
        per = [sum(r[2] for r in rows[d]) for d in range(len(self.distinct))]
        n = self.packets_of(managed)
        longs = sum(per[d] for d in self.index)
        return sum(n) - longs, longs

    def neighbours_differ(self):
        return all(a != b and not np.array_equal(self.distinct[a], self.distinct[b]) for a, b in zip(self.index, self.index[1:]))


def _headers(name):
    if ("headers", name) not in _cache:
        ch, rate, q = checker.SETUPS[name]
        _cache["headers", name] = ref_host.reference_headers(ch, rate, q)
    return _cache["headers", name]


def many_streams(name, count, lengths, kinds=KINDS, seed=0):
    """-> Many: `count` streams of setup `name`, made from D distinct streams dealt round.  lengths: D distinct lengths,
    or one length for all (the streams then differ in their signals alone); kinds: tests/signals.py's, cycled over the
    distinct streams."""
    lengths = (int(lengths),) * D if np.ndim(lengths) == 0 else tuple(int(n) for n in lengths)
    key = (name, lengths, tuple(kinds), seed)
    if (key, count) not in _groups:
        assert len(lengths) == D
        if ("distinct", key) not in _cache:
            ch = checker.SETUPS[name][0]
            out = []
            for d, n in enumerate(lengths):
                x = s16_streams(np.random.default_rng([seed, d]), ch, n, [kinds[d % len(kinds)]])[0]
                x.setflags(write=False)
                out.append(x)
            _cache["distinct", key] = out
        _groups[key, count] = Many(name, _cache["distinct", key], [s % D for s in range(count)], key)
    return _groups[key, count]


def join(*groups):
    """the groups' streams one group after the other -> Many (the reference still runs once per distinct stream)"""
    key = ("join",) + tuple((g.key, g.count) for g in groups)
    if key not in _groups:
        distinct, index = [], []
        for g in groups:
            index += [len(distinct) + i for i in g.index]
            distinct += g.distinct
        _groups[key] = Many(groups[0].name, distinct, index, key)
    return _groups[key]


# ---- the groups of the GPU ids ----
COUNT = 1049                         # > 1024; prime, so no stride of the kernels divides it
MANAGED_SETUPS = {"abr128_stereo": ("44k_stereo_q4", MANAGED_RATES), "minmax_mono": ("44k_mono_q5", MANAGED[3][1])}
assert MANAGED[3][0] == 1


def short_group(seed=1):
    """ids a, e, f, h: COUNT streams of 1 to 9024 frames"""
    return many_streams(SETUP, COUNT, SHORT, KINDS, seed)


def uniform_group(seed=2):
    """id b: COUNT streams of UNIFORM frames"""
    return many_streams(SETUP, COUNT, UNIFORM, UNIFORM_KINDS, seed)


def bench_group(seed=3):
    """id c: 101 streams of 1 to 46 001 frames, bursts and clicks in most of them"""
    return many_streams(SETUP, 101, LONG, LONG_KINDS, seed)


def managed_group(which, seed=4):
    """id d: streams of SHORT's lengths whose packets add up to an odd count below a slice (so that the next slice edge
    falls inside a stream), then 1100 streams of two packets each -- a slice of 2048 blocks inside that run begins in the
    middle of one and so holds 1025 streams --, then 250 more of SHORT's lengths, over further slice edges.  The count in
    front is chosen from the reference's own packet counts."""
    name, rates = MANAGED_SETUPS[which]
    pool = many_streams(name, 400, SHORT, KINDS, seed)
    n = pool.packets_of(rates)
    front, total = 0, 0
    for s in range(len(n)):          # the longest odd prefix that leaves the run's first stream astride the first slice edge
        if total + n[s] > BATCH_UNITS - 1:
            break
        total += n[s]
        if total % 2 == 1:
            front = s + 1
    assert front > 0
    return join(many_streams(name, front, SHORT, KINDS, seed), many_streams(name, 1100, TINY, KINDS, seed + 100),
                many_streams(name, 250, SHORT, KINDS, seed + 200))


def owner_group(which, seed=6):
    """id d's second group: a stream of clicks long enough for more than 2048 packets, in front -- it owns the whole first
    slice and is cut by its edge -- and two short ones behind it"""
    name, _ = MANAGED_SETUPS[which]
    key = ("owner", name, seed)
    if key not in _groups:
        ch = checker.SETUPS[name][0]
        distinct = [s16_streams(np.random.default_rng([seed, d]), ch, n, [k])[0] for d, (n, k) in
                    enumerate(((850001, "clicks"), (2049, "noise"), (7777, "gated")))]
        _groups[key] = Many(name, distinct, [0, 1, 2], key)
    return _groups[key]


def slices_of(stream_start, size=BATCH_UNITS):
    """From a group's stream_start: -> (number of slices of `size` blocks, the most streams any slice holds a block of,
    the streams with three or more packets that a slice edge cuts)"""
    start = np.asarray(stream_start, np.int64)
    nb = int(start[-1])
    nslices = (nb + size - 1) // size
    most, cut = 0, []
    for k in range(nslices):
        lo, hi = k * size, min((k + 1) * size, nb)
        first = int(np.searchsorted(start, lo, side="right")) - 1
        last = int(np.searchsorted(start, hi - 1, side="right")) - 1
        most = max(most, last - first + 1)
        if start[last] < hi < start[last + 1] and start[last + 1] - start[last] >= 3:
            cut.append(last)
    return nslices, most, cut


def conditions_of(which):
    """The numbers each GPU id asserts ahead of its comparison, from the lengths and the reference's records alone."""
    if which in ("a", "e", "f", "h"):
        g = short_group()
    elif which == "b":
        g = uniform_group()
    elif which == "c":
        g = bench_group()
    else:
        g = managed_group(which)
    longest = max(g.frames)
    s1, s2 = steps_of(longest)
    out = dict(group=g, ns=g.count, ingest=ingest_items(g.count, longest), pass1=g.count * s1, pass2=g.count * s2, steps1=s1)
    if which in MANAGED_SETUPS:
        rates = MANAGED_SETUPS[which][1]
        out["slices"], out["most"], out["cut"] = slices_of(np.concatenate([[0], np.cumsum(g.packets_of(rates))]))
    else:
        out["short"], out["long"] = g.class_counts()
    return out


# ---- id g: continuing streams ----
# one stream long enough for a round whose detector launch is tiled at 299 streams; the rest as SHORT
LIVE = (17001, 15002, 12003, 9024, 9023, 8001, 7777, 6001, 5000, 4097, 3073, 3072, 3071, 2500, 2049, 2048, 1500, 1023, 700, 100, 33, 20, 1)
LIVE_COUNT = 13 * D
WRITE_FRAMES = 1024
assert len(set(LIVE)) == D


def live_group(seed=5):
    return many_streams(SETUP, LIVE_COUNT, LIVE, KINDS, seed)


def live_cuts(frames, batch):
    """Per stream its pieces over at most four rounds (tests/feed_cases.py: run_live; a stream is closed with its last
    piece).  Copy c of a distinct stream takes pattern (c + batch) % 7, so the copies of one stream are all cut differently:
    whole in one piece; an empty piece first; a 1-frame piece first; a third, an empty piece, the rest; four random pieces
    (empty ones among them); two empty pieces first; a 1-frame piece last."""
    rng = np.random.default_rng([7, batch])
    out = []
    for s, n in enumerate(frames):
        v = (s // D + batch) % 7
        if v == 0:
            c = [n]
        elif v == 1:
            c = [0, n]
        elif v == 2:
            c = [1, n - 1]
        elif v == 3:
            c = [max(1, n // 3), 0, n - max(1, n // 3)]
        elif v == 4:
            e = [0] + sorted(int(p) for p in rng.integers(0, n + 1, 3)) + [n]
            c = [b - a for a, b in zip(e, e[1:])]
            if c[0] == 0 and c[1] == 0 and c[2] == 0:
                c = [0, 0, 0, n]
        elif v == 5:
            c = [0, 0, n - n // 2, n // 2]
        else:
            c = [n - 1, 1] if n > 1 else [0, 0, 1]
        assert sum(c) == n and len(c) <= 4 and all(p >= 0 for p in c)
        # (a stream is never closed on an empty piece before it had a frame: the feed refuses that)
        assert any(c[:-1]) or c[-1] > 0
        out.append(c)
    return out


def live_conditions(frames, cuts):
    """What id g asserts of its cuts: -> dict(rounds, tiled = the most `streams x detector steps` any round's launch has, at
    the least -- a piece of n frames brings n / 64 - 4 new steps or more, and the launch takes the longest piece's for all
    --, fresh = rounds in which a stream begins beside one that continues, closing = the rounds in which streams close,
    empty / single / ragged = pieces of 0 frames, of 1 frame, of no multiple of WRITE_FRAMES)"""
    rounds = max(len(c) for c in cuts)
    tiled, fresh = 0, 0
    for r in range(rounds):
        pieces = [c[r] if r < len(c) else 0 for c in cuts]
        tiled = max(tiled, len(cuts) * max(max(pieces) // SEARCHSTEP - VE_WIN, 0))
        begins = any(r < len(c) and c[r] > 0 and not any(c[:r]) for c in cuts)
        continues = any(r < len(c) and any(c[:r]) for c in cuts)
        fresh += bool(r > 0 and begins and continues)
    flat = [p for c in cuts for p in c]
    return dict(rounds=rounds, tiled=tiled, fresh=fresh, closing={len(c) - 1 for c in cuts}, empty=flat.count(0), single=flat.count(1),
                ragged=sum(1 for p in flat if p % WRITE_FRAMES))


# ---- id i: the tiled detector's flags against the reference's marks ----
# k_env_bits_tiled gives a wave 64 consecutive steps and stages the 13 rows of history in front of them; the oldest of those
# rows is read by the tile's first step alone, and only at the longest stretch.  Bursts of 1800 samples (28 steps: the
# stretch is at its longest again when one ends) every 65 steps (37 quiet steps between them: and again when the next
# begins) move every onset and every decay one step on from tile to tile, so that over 66 bursts each falls on the first
# step of a tile -- where the trigger reads that row.
SWEEP_PERIOD, SWEEP_ON, SWEEP_BURSTS = 65 * SEARCHSTEP, 1800, 66
SWEEP_COUNT = 2 * D


class Sweep:
    """distinct: per distinct stream the reference's own detector over it (oracle.ref.RefEncoder.envelope_feed): pcm as the
    detector saw it, steps, marks [steps + 2]; index[s]: which of them stream s is"""

    def __init__(self, name, distinct, index):
        self.name, self.distinct, self.index, self.count = name, distinct, index, len(index)
        self.steps = distinct[0]["steps"]
        assert all(o["steps"] == self.steps and o["pcm"].shape == distinct[0]["pcm"].shape for o in distinct)


def tile_starts_hit(marks, steps):
    """-> (tile-first steps j = 64 m where a run of marks begins after 26 steps without one, those where a run of marks ends)"""
    m = np.asarray(marks[:steps]) != 0
    begins = [j for j in range(64, steps, 64) if m[j] and not m[j - 26:j].any()]
    ends = [j for j in range(64, steps - 1, 64) if m[j - 1] and not m[j:j + 2].any()]
    return begins, ends


def sweep_group(seed=8):
    key = ("sweep", seed)
    if key not in _groups:
        from oracle import ref
        ch, rate, q = checker.SETUPS[SETUP]
        frames = SWEEP_PERIOD * SWEEP_BURSTS
        distinct = []
        for d in range(D):       # (the bursts of stream d begin 5 d samples earlier: the onsets lie differently inside their steps)
            x = np.ascontiguousarray(gated(ch, frames + 5 * d, 1000 * seed + d, period=SWEEP_PERIOD, on=SWEEP_ON)[:, 5 * d:])
            distinct.append(ref.RefEncoder(ch, rate, q).envelope_feed(x))
        _groups[key] = Sweep(SETUP, distinct, [s % D for s in range(SWEEP_COUNT)])
    return _groups[key]
