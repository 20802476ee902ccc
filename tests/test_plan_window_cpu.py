"""The stream walk through a sliding window of marks (k_blockout.h: MarkWindow under plan_stream, what k_plan_streams runs)
against the one-shot walk over a whole mark array, both compiled for the host from the shipped header
(tests/plan_window_host.py).  The window must never show: for every window size from plan_window_min up, the blocks, the
counts, the pending centre and the walk's final state are those of the one-shot walk, and no read falls outside the window
(the build counts them: that count is the check on the derived minimum)."""
import os

import numpy as np
import pytest

from tests import checker
from tests import plan_window_host as pwh

ROOT = checker.ROOT
STEP = 64
GOLDEN = ("44k_stereo_q4", "44k_mono_q5")
# the two pairs of libvorbis' setups (the minimum is the width of a trip of the walk, 65), and a pair the format allows whose
# horizon lies further off than a trip is wide (the minimum follows from the block sizes, 98)
BLOCKSIZES = [(256, 2048), (512, 4096), (64, 8192)]
IDS = ["256_2048", "512_4096", "64_8192"]


@pytest.fixture(scope="module")
def lib():
    return pwh.build()


def golden_flags(name):
    """The detector's flags over a golden's PCM (the host-compiled detector, held to the golden's marks by
    tests/test_envelope.py), repeated to a few thousand steps."""
    from tests.emul.emul import Emul
    from vorbis_amd import EnvelopeState
    z = np.load(os.path.join(ROOT, "tests", "golden", "envelope_%s.npz" % name))
    blob = np.fromfile(os.path.join(ROOT, "vorbis_amd", "data", "setup_%s.bin" % name), dtype=np.uint8)
    flags = Emul(blob).envelope_search(z["pcm"], int(z["steps"][0]), EnvelopeState())
    assert flags.any()
    return np.tile(flags, 11)


@pytest.fixture(scope="module")
def sequences():
    rng = np.random.default_rng(14)
    n = 4200
    seqs = {"golden_" + name: golden_flags(name) for name in GOLDEN}
    dense = np.zeros(n, np.uint8)
    at = np.cumsum(rng.integers(2, 12, n // 6))
    at = at[at < n]
    dense[at] = rng.choice([1, 2, 3, 5, 7], len(at))
    seqs["dense_clicks"] = dense
    sparse = np.zeros(n, np.uint8)  # long runs of long blocks between the clicks: the cursor far ahead of the centre
    at = np.cumsum(rng.integers(30, 400, 40))
    at = at[at < n]
    sparse[at] = rng.choice([1, 2, 3, 5, 7], len(at))
    seqs["sparse_clicks"] = sparse
    seqs["no_marks"] = np.zeros(n, np.uint8)
    seqs["every_step"] = rng.choice([1, 2, 3, 5, 7], n).astype(np.uint8)
    return seqs


def geometries(flags, bs):
    """(label, nsamples, eof): the stream goes on; it ends, with the reference's padding behind it and detector steps to its
    end; it ends far beyond the last detector step -- forced short blocks whose centres run on while the cursor stands."""
    n = len(flags) * STEP + 4 * STEP  # (every flag a step taken: last == len(flags))
    return [("open", n, 0), ("eof", n, n - 3 * bs[1]), ("eof_beyond_steps", n + 12 * bs[1], n + 9 * bs[1] - 77)]


def same(a, b, what):
    assert a.res == b.res, (what, a.res, b.res)
    assert np.array_equal(a.kind, b.kind) and np.array_equal(a.begin, b.begin), what


@pytest.mark.parametrize("bs", BLOCKSIZES, ids=IDS)
def test_every_window_size_from_the_minimum(lib, sequences, bs):
    pw = pwh.PlanWindow(lib, bs)
    lo = pw.minimum
    assert lo >= 65 and lo >= (3 * (bs[0] + bs[1]) // 4) // STEP
    assert lo == (98 if bs[1] == 8192 else 65)
    sizes = list(range(lo, lo + 131)) + [1000, 4096, 32768, 1 << 20]
    for name, flags in sequences.items():
        for label, nsamples, eof in geometries(flags, bs):
            want = pw.array(flags, nsamples, eof)
            assert want.res["blocks"] > 50, (name, label)
            if eof:
                assert want.res["pending"] == -1, (name, label)
            dry = pw.array(flags, nsamples if not eof else eof, 0)  # (k_plan_streams' dry run: as far as the real samples go)
            for size in sizes:
                got = pw.window(flags, nsamples, size, eof)
                what = (name, label, size)
                assert got.window == size and got.outside == 0, what + (got.window, got.outside)
                same(got, want, what)
                if size < 200 and label != "eof_beyond_steps":
                    assert got.refills > 15, what + (got.refills,)  # (the window did slide: many refills over the stream)
                if size >= len(flags) + 4:
                    assert got.refills == 0, what
            for size in (lo, lo + 7, 997):
                got = pw.window(flags, nsamples if not eof else eof, size, 0, dry=True)
                assert got.outside == 0 and got.kind is None and got.res == dry.res, (name, label, size, "dry")


@pytest.mark.parametrize("bs", BLOCKSIZES, ids=IDS)
def test_flags_in_two_arrays(lib, sequences, bs):
    """The steps from `split` on come from a second array (the second detector pass over a stream's padding): mark_at's
    neighbours straddle the seam, and so do refills."""
    pw = pwh.PlanWindow(lib, bs)
    lo = pw.minimum
    for name, flags in sequences.items():
        n = len(flags)
        for label, nsamples, eof in geometries(flags, bs):
            want = pw.array(flags, nsamples, eof)
            for split in (0, 1, lo - 1, lo, n // 2 + 3, n - 3 * bs[1] // STEP, n - 1, n):
                for size in (lo, lo + 1, lo + 64, 333, 1 << 16):
                    got = pw.window(flags, nsamples, size, eof, split=split)
                    assert got.outside == 0, (name, label, split, size)
                    same(got, want, (name, label, split, size))


@pytest.mark.parametrize("bs", BLOCKSIZES, ids=IDS)
def test_a_window_below_the_minimum_is_raised_to_it(lib, sequences, bs):
    pw = pwh.PlanWindow(lib, bs)
    flags = sequences["golden_44k_stereo_q4"]
    label, nsamples, eof = geometries(flags, bs)[1]
    want = pw.array(flags, nsamples, eof)
    for size in (pw.minimum - 1, 1, 0, -5):
        got = pw.window(flags, nsamples, size, eof)
        assert got.window == pw.minimum and got.outside == 0, (size, got.window, got.outside)
        same(got, want, size)
    # and the count of reads outside the window does bite: a window taken as given, far too small for a trip of the walk
    raw = pw.window(flags, nsamples, 8, eof, raw=True)
    assert raw.window == 8 and raw.outside > 0
    if bs == (64, 8192):  # where the block sizes set the minimum it is tight: one mark less and long blocks read past the window
        raw = pw.window(sequences["no_marks"], nsamples, pw.minimum - 1, eof, raw=True)
        assert pw.minimum == 98 and raw.outside > 0


def test_a_stream_shorter_than_the_window_is_read_once(lib):
    """What plan_streams does for short streams: the window is cut to the stream's marks (+ 4), below the minimum even, and
    never refilled."""
    pw = pwh.PlanWindow(lib, (256, 2048))
    rng = np.random.default_rng(5)
    for n in (0, 1, 3, 20, 60, 64, 65, 130):
        flags = (rng.random(n) < 0.2).astype(np.uint8) * 3
        for label, nsamples, eof in geometries(flags, pw.bs)[:2]:
            if eof < 0:
                continue
            want = pw.array(flags, nsamples, max(eof, 0))
            got = pw.window(flags, nsamples, n + 4, max(eof, 0), raw=True)
            assert got.refills == 0 and got.outside == 0, (n, label)
            same(got, want, (n, label))
