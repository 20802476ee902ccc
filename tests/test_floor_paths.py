"""GPU suite (-m gpu): every output of the floor stage against the CPU checker, bit for bit, for EVERY block of a batch.

The floor stage (k_floor, k_floor_pair: k_floor.inc) takes the tone fold, the mask mix, floor1_fit and the curve half of
floor1_encode in one wave per channel-block.  What it leaves -- mdct (scaled in place), logmask, posts, post_valid,
nonzero -- and what the next stage makes of its curve (iwork) are compared with tests.checker's tap_block for all the
blocks of the batch: the stage's tables are fetched once per channel-block and handed from the fit to the quantiser to
the curve (PostTables), and its table and tensor accesses go through one 32-bit offset per quad
(dm_load / dm_store), so a wrong table, offset or hand-over shows in whichever block it hits.

Setups: the bench's (44k_stereo_q4), one whose short blocks have 19 posts and pair their channels in a wave (q9,
k_floor_pair from VAMD_FLOOR_PAIR_MIN channel-blocks), an odd channel count (mono) and two submaps with a floor each
(5.1).  Both block sizes, the four window shapes of a long block, batches of 1, 3, 33 and 130 blocks (one wave, an odd
few, more than a CU's resident waves of one SIMD, more than 256 channel-blocks).  Inputs: seeded noise at mixed levels; a
silent block (the fit returns NULL: post_valid == 0); a lone spike; a full-scale two-tone block (many splits: the greedy
loop, fit_line_pair and the post tables at work) -- the special ones in the first, second, last-but-one and last places.
"""
import numpy as np
import pytest

from tests import checker
from tests.feed_cases import FLOOR_KEYS as KEYS, FLOOR_WANT as WANT, channels, chk_for

pytestmark = pytest.mark.gpu
SHAPES = ((1, 1), (0, 1), (1, 0), (0, 0))  # (lW, nW) of a long block
SETUPS = ("44k_stereo_q4", "44k_stereo_q9", "44k_mono_q5", "44k_51_q3")
_refs = {}


def make_blocks(nb, ch, n, seed):
    """[nb][ch][n] and each block's kind.  Noise at mixed levels, with the special blocks at both ends of the batch."""
    rng = np.random.default_rng(seed)
    amps = (10.0 ** rng.uniform(-4, 0, (nb, 1, 1))).astype(np.float32)
    pcm = ((rng.random((nb, ch, n), dtype=np.float32) - 0.5) * 2 * amps).astype(np.float32)
    kinds = ["noise"] * nb
    t = np.arange(n, dtype=np.float64)
    if nb == 1:
        place = {0: "tones"}
    elif nb == 3:
        place = {0: "silent", 1: "tones", 2: "spike"}
    else:
        place = {0: "silent", 1: "tones", 2: "spike", nb // 2: "silent", nb // 2 + 1: "tones", nb - 3: "spike", nb - 2: "tones",
                 nb - 1: "silent"}
    for b, kind in place.items():
        kinds[b] = kind
        pcm[b] = 0
        if kind == "spike":
            pcm[b, 0, (7 * n) // 16 + 3] = 0.9
            pcm[b, ch - 1, n - 5] = -0.25
        elif kind == "tones":  # full scale: two sines a few bins apart per channel, the pair moving with the channel
            for c in range(ch):
                w0, w1 = 2 * np.pi * (0.031 + 0.017 * c), 2 * np.pi * (0.037 + 0.017 * c)
                pcm[b, c] = (0.5 * np.sin(w0 * t) + 0.5 * np.sin(w1 * t + 0.3)).astype(np.float32)
    return pcm, kinds


def reference(name, W, nb):
    """The checker's taps of the batch (name, W, nb), computed once and shared by the cases that run it."""
    key = (name, W, nb)
    if key not in _refs:
        import vorbis_amd
        an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(name), device=0)
        n, nposts = an.blocksizes[W], an.posts[W]
        an.close()
        pcm, kinds = make_blocks(nb, channels(name), n, 1200 + 7 * nb + W)
        shape = np.arange(nb) % len(SHAPES)
        lW = np.array([SHAPES[s][0] if W else 0 for s in shape], dtype=np.int32)
        nW = np.array([SHAPES[s][1] if W else 0 for s in shape], dtype=np.int32)
        chk = chk_for(name)
        refs = [chk.tap_block(pcm[b], int(lW[b]), W, int(nW[b]), W, -9999.0) for b in range(nb)]
        _refs[key] = (pcm, kinds, lW, nW, refs, nposts)
    return _refs[key]


def run_and_compare(name, W, nb):
    import torch
    import vorbis_amd
    assert torch.cuda.is_available()
    pcm, kinds, lW, nW, refs, nposts = reference(name, W, nb)
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(name), device=0)
    dv = lambda v: torch.from_numpy(np.asarray(v, dtype=np.int32)).cuda()  # noqa: E731
    outs = an.analyze(torch.from_numpy(pcm).cuda(), W=W, lW=dv(lW), nW=dv(nW), blocktype=W, ampmax_in=-9999.0, want=WANT)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    config = an.config_string()
    an.close()
    bad = []
    for b in range(nb):  # every block
        if checker.compare_block(refs[b], {k: v[b] for k, v in got.items()}, nposts, keys=KEYS, verbose=len(bad) < 3):
            bad.append((b, kinds[b]))
    assert not bad, "checker=%s: %d of %d blocks differ: %s" % (chk_for(name).kind, len(bad), nb, bad[:8])
    # the inputs are what they are meant to be: no fit for a silent block, fits for a two-tone block (not for every
    # channel: a 5.1 setup's LFE has nothing above its fit's floor where these tones lie)
    for b in range(nb):
        if kinds[b] == "silent":
            assert not got["post_valid"][b].any(), b
        if kinds[b] == "tones":
            assert got["post_valid"][b][0] and got["post_valid"][b].sum() >= min(2, got["post_valid"][b].size) and got["nonzero"][b].any(), b
    return config


@pytest.mark.parametrize("nb", [1, 3, 33, 130])
@pytest.mark.parametrize("name", SETUPS)
def test_long_blocks_every_block(name, nb):
    run_and_compare(name, 1, nb)


@pytest.mark.parametrize("nb", [3, 130])
@pytest.mark.parametrize("name", SETUPS)
def test_short_blocks_every_block(name, nb):
    run_and_compare(name, 0, nb)


@pytest.mark.parametrize("name,W,nb", [("44k_stereo_q9", 0, 130), ("44k_stereo_q9", 0, 3), ("44k_stereo_q4", 0, 130),
                                       ("44k_stereo_q4", 1, 33), ("44k_stereo_q9", 1, 33)])
def test_paired_channels_every_block(name, W, nb, monkeypatch):
    """k_floor_pair (two channels a wave, the bodies compiled against the half-wave vocabulary) at batch sizes far below
    the one it is launched from by default: wherever a stereo setup's floor has at most 32 posts."""
    monkeypatch.setenv("VAMD_TEST_KNOBS", "1")
    monkeypatch.setenv("VAMD_FLOOR_PAIR_MIN", "0")
    assert "VAMD_FLOOR_PAIR_MIN=0" in run_and_compare(name, W, nb)
