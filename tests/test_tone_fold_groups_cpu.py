"""CPU: the tone fold per group (k_tone_fold.inc, vamd_derive.h).

1. The per-group tables (group_p0, bin_group, line_slot) against max_seeds' own walk (lib/psy.c:512-545) replayed from
   each shipped blob's octave[], for every psy look: tests/c/tone_fold_groups.cpp, a program of its own built with
   -fsanitize=address,undefined.
2. The one-lane build of the bodies (tests/emul: tone_fold_prepare, tone_fold_quad as the GPU compiles them, one lane)
   over signals that take every arm of the fold (tests/tone_fold_signals.py), every shipped setup, both block sizes,
   bit for bit against tests/checker.py.
"""
import glob
import os
import subprocess

import numpy as np
import pytest

from tests import checker, hostbuild, tone_fold_signals
from tests.emul.emul import Emul

ROOT = checker.ROOT
ALL_SETUPS = tuple(checker.SETUPS) + tuple(checker.SURROUND)
KEYS = ("tone", "logmask", "mdct", "post_valid", "nonzero", "iwork")  # (+ posts: compare_block takes them itself)


def test_group_tables_follow_the_reference_walk():
    exe = hostbuild.program("tone_fold_groups.cpp")
    blobs = sorted(glob.glob(os.path.join(ROOT, "vorbis_amd", "data", "setup_*.bin")))
    assert len(blobs) == 5
    r = subprocess.run([exe] + blobs, capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count(": ok") == len(blobs), r.stdout[-4000:] + r.stderr[-4000:]


def _checker(name):
    if name in checker.SETUPS:
        return checker.Checker(name)
    from tests.feed_cases import SurroundChecker
    return SurroundChecker(name)


@pytest.mark.parametrize("name", ALL_SETUPS)
def test_one_lane_bodies_match_the_checker(name):
    blob = np.fromfile(os.path.join(ROOT, "vorbis_amd", "data", "setup_%s.bin" % name), dtype=np.uint8)
    em, chk = Emul(blob), _checker(name)
    bad = []
    for W in (0, 1):
        pcm = tone_fold_signals.blocks(em.channels, em.bs[W])
        for k, sig in enumerate(tone_fold_signals.NAMES):
            ref = chk.tap_block(pcm[k], W, W, W, W, -9999.0)
            got = em.analyze_block(pcm[k], W, W, W, W, -9999.0)
            assert "tone" in ref and "tone" in got
            if checker.compare_block(ref, got, 0, keys=KEYS, verbose=True):
                bad.append((W, sig))
    assert not bad, "checker=%s: %s" % (chk.kind, bad)
