"""Signals for the tone fold's tests (test_tone_fold_groups_cpu.py / _gpu.py): one block each, chosen so that every arm of
max_seeds' fold (lib/psy.c:522-543, k_tone_fold.inc) is taken.

  silence      every seed line NEGINF: no group scans a real value (the minima stay +inf), minV == NEGINF
  sine_100     full scale, about 100 Hz: real lines only inside the long groups of the low octaves
  sine_15k     full scale, about 15 kHz: one-line groups, the tail bins' group
  noise_half   white noise at +-0.5, and
  noise_quiet  at +-1e-4: the ATH side of the final max
  impulse      a single sample
  half_silent  silence, then noise: both in one block
"""
import numpy as np

NAMES = ("silence", "sine_100", "sine_15k", "noise_half", "noise_quiet", "impulse", "half_silent")
RATE = 44100.0


def blocks(ch, n, seed=1700):
    """[len(NAMES)][ch][n] float32, the channels of a block slightly apart so that no two channel-blocks are equal."""
    rng = np.random.default_rng(seed + n)
    t = np.arange(n, dtype=np.float64)
    out = np.zeros((len(NAMES), ch, n), np.float32)
    for c in range(ch):
        out[1, c] = np.sin(2 * np.pi * (100.0 + 3.0 * c) / RATE * t + 0.1 * c)
        out[2, c] = np.sin(2 * np.pi * (15000.0 + 40.0 * c) / RATE * t + 0.1 * c)
        out[3, c] = (rng.random(n, dtype=np.float32) - 0.5)
        out[4, c] = (rng.random(n, dtype=np.float32) - 0.5) * np.float32(2e-4)
        out[5, c, (5 * n) // 16 + 7 * c] = 1.0
        out[6, c, n // 2:] = (rng.random(n - n // 2, dtype=np.float32) - 0.5)
    return out
