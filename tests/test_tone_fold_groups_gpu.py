"""GPU suite (-m gpu): the tone fold per group (k_tone_fold.inc) on the device, every block bit for bit against the CPU checker.

Signals that take every arm of the fold (tests/tone_fold_signals.py: silence, low and high sines, loud and quiet noise,
an impulse, a half-silent block), one block each; the batch as it is (under 64 channel-blocks: both masks in one launch)
and repeated past 64 channel-blocks.  Two levels: LEVEL_PSY with the `tone` tap (the fold as k_tone_fold) and LEVEL_FULL
(the fold inside k_floor: what it leaves in logmask, mdct, posts, post_valid and, through the curve, iwork).  A stereo
setup's short blocks are also run as a batch large enough for the shipped pair threshold (k_floor_pair: two channels a
wave, 32 lanes each).
"""
import numpy as np
import pytest

from tests import checker, tone_fold_signals
from tests.feed_cases import channels, chk_for

pytestmark = pytest.mark.gpu
SETUPS = ("44k_stereo_q4", "44k_stereo_q9", "44k_mono_q5", "44k_51_q3")
FULL_KEYS = ("logmask", "mdct", "post_valid", "iwork")
PAIR_MIN_SHORT = 16384  # channel-blocks from which short stereo blocks pair their channels (vamd_kernels.h)
_refs = {}


def reference(name, W):
    """(signals [7][ch][n], the checker's taps of each, posts of the size class): computed once per (setup, size)."""
    if (name, W) not in _refs:
        import vorbis_amd
        an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(name), device=0)
        n, nposts = an.blocksizes[W], an.posts[W]
        an.close()
        pcm = tone_fold_signals.blocks(channels(name), n)
        chk = chk_for(name)
        _refs[(name, W)] = (pcm, [chk.tap_block(pcm[k], W, W, W, W, -9999.0) for k in range(len(pcm))], nposts)
    return _refs[(name, W)]


def run_and_compare(name, W, reps):
    import torch
    import vorbis_amd
    assert torch.cuda.is_available()
    pcm, refs, nposts = reference(name, W)
    nsig = len(refs)
    batch = torch.from_numpy(np.tile(pcm, (reps, 1, 1))).cuda()
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(name), device=0)
    bad = []
    for level, want, keys in ((vorbis_amd.LEVEL_PSY, ("tone",), ("tone",)),
                              (vorbis_amd.LEVEL_FULL, FULL_KEYS + ("posts",), FULL_KEYS)):
        outs = an.analyze(batch, W=W, lW=W, nW=W, blocktype=W, ampmax_in=-9999.0, level=level, want=want)
        torch.cuda.synchronize()
        got = {k: v.cpu().numpy() for k, v in outs.items()}
        for b in range(reps * nsig):  # every block
            if checker.compare_block(refs[b % nsig], {k: v[b] for k, v in got.items()}, nposts, keys=keys, verbose=len(bad) < 3):
                bad.append((level, b, tone_fold_signals.NAMES[b % nsig]))
    an.close()
    assert not bad, "checker=%s: %d blocks differ: %s" % (chk_for(name).kind, len(bad), bad[:8])
    # the signals are what they are meant to be: nothing real in a silent block's curve but the ATH side of the max
    assert not got["post_valid"][0].any()


@pytest.mark.parametrize("W", [0, 1])
@pytest.mark.parametrize("name", SETUPS)
def test_fold_arms_few_blocks(name, W):
    run_and_compare(name, W, 1)


@pytest.mark.parametrize("W", [0, 1])
@pytest.mark.parametrize("name", SETUPS)
def test_fold_arms_past_64_channel_blocks(name, W):
    nsig = len(tone_fold_signals.NAMES)
    run_and_compare(name, W, 64 // (nsig * channels(name)) + 1)


@pytest.mark.parametrize("name", ["44k_stereo_q4", "44k_stereo_q9"])
def test_fold_arms_paired_short_blocks(name):
    nsig = len(tone_fold_signals.NAMES)
    run_and_compare(name, 0, PAIR_MIN_SHORT // (2 * nsig) + 1)
