"""Blocks that take floor1_fit's split loop (k_floor.inc: floor_fit_posts, inspect_error_wave, fit_line_pair) through the
exits the loop's walk can end by.  Shared by tests/test_floor_split_gpu.py and the census of tools/fl_calls.py, which
counts per signal what the loop did (profiles/r19_floor_split.txt lists which exit each signal was seen to reach).

name            what it is there for
noise_hi/mid/lo white noise at three levels: the failing point lies in the first chunk of the range (the common case)
band_top        a flat low noise floor with a strong narrow band in the top sixteenth of the spectrum: the whole-range
                line and the right-hand ranges fail in their LAST chunk, after every earlier chunk has passed
band_low        the same with the band in the lowest bins: first chunk of the whole range, last of none
silent          floor1_fit returns NULL (nothing above the fit's floor): the loop is not entered
faint           noise just above the level at which the fit finds nothing: few points are of the class the point test looks
                at, so walks run to their end and the count thresholds / the squared-error sum decide.  (The whole-range
                line itself is not accepted at any level of white noise: the mask follows the threshold in quiet, which no
                line fits.  No signal here reaches "the first inspect returns 0".)
tones           test_floor_paths.py's full-scale two-tone block: many splits
six_sines       six sines over faint noise: many splits, fit_line_pair on short ranges, sides with denom <= 0
noise|silent, noise|faint, faint|noise
                one channel of a stereo block each: on the pair path one half of the wave stops in its first chunk
                while the other walks every trip (or never enters the loop)
"""
import numpy as np

NAMES = ("band_top", "noise|faint", "six_sines", "noise_hi", "noise_mid", "noise_lo", "band_low", "silent", "faint", "tones",
         "noise|silent", "faint|noise")
FAINT = 1e-6  # just above the level at which the fit finds nothing (2e-7): the fewest points of class a


def _noise(rng, n, amp):
    return ((rng.random(n, dtype=np.float32) - 0.5) * 2 * amp).astype(np.float32)


def _band(n, lo, hi, amp):
    """Five sines spread over the spectrum's bins [lo, hi) of an n-sample block (n / 2 bins)."""
    t = np.arange(n, dtype=np.float64)
    x = np.zeros(n)
    for j, b in enumerate(np.linspace(lo, hi - 1, 5)):
        x += np.sin(np.pi * (b + 0.5) / (n // 2) * t + 0.7 * j)
    return (amp / 5 * x).astype(np.float32)


def channel(kind, n, c, rng):
    n2 = n // 2
    t = np.arange(n, dtype=np.float64)
    if kind in ("noise", "noise_hi"):
        return _noise(rng, n, 0.5)
    if kind == "noise_mid":
        return _noise(rng, n, 0.03)
    if kind == "noise_lo":
        return _noise(rng, n, 0.002)
    if kind == "band_top":
        return _noise(rng, n, 1e-3) + _band(n, (15 * n2) // 16 + n2 // 64, n2 - n2 // 64, 0.5)
    if kind == "band_low":
        return _noise(rng, n, 1e-3) + _band(n, 1, max(6, n2 // 16), 0.5)
    if kind == "silent":
        return np.zeros(n, dtype=np.float32)
    if kind == "faint":
        return _noise(rng, n, FAINT)
    if kind == "tones":
        w0, w1 = 2 * np.pi * (0.031 + 0.017 * c), 2 * np.pi * (0.037 + 0.017 * c)
        return (0.5 * np.sin(w0 * t) + 0.5 * np.sin(w1 * t + 0.3)).astype(np.float32)
    if kind == "six_sines":
        x = np.zeros(n)
        for j, f in enumerate((0.011, 0.023, 0.058, 0.094, 0.171, 0.303)):
            x += np.sin(2 * np.pi * (f + 0.004 * c) * t + j)
        return (0.15 * x).astype(np.float32) + _noise(rng, n, 1e-4)
    raise ValueError(kind)


def block(kind, ch, n, rng):
    parts = kind.split("|")
    return np.stack([channel(parts[c % len(parts)], n, c, rng) for c in range(ch)])


def batch(nb, ch, n, seed):
    """[nb][ch][n] and each block's kind: NAMES in turn, so that three blocks already hold the last-chunk exit, a pair whose
    halves part ways and the many-split block."""
    rng = np.random.default_rng(seed)
    kinds = [NAMES[b % len(NAMES)] for b in range(nb)]
    return np.stack([block(k, ch, n, rng) for k in kinds]).astype(np.float32), kinds
