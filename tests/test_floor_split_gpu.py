"""GPU suite (-m gpu): the split loop of floor1_fit (k_floor.inc) on blocks that take it through the exits its walk can end
by, every output of the floor stage against the CPU checker, bit for bit, for EVERY block of a batch.

Beside tests/test_floor_paths.py (seeded noise, a silent block, a spike, two tones).  inspect_error_wave ends its walk
with the first chunk of 64 points (32 on the pair path) that holds a failing point (VAMD_FL_INSPECT_STOP), and
fit_line_pair forms the two sides' fits in two groups of lanes; the signals of tests/floor_split_signals.py
say which exit each is there for: the failure in the first chunk (noise), in the LAST chunk of the whole range and of the
right-hand ranges (band_top), walks that run to their end (faint, band_low's left-hand ranges), no loop at all (silent),
many splits with short ranges and sides without a fit (tones, six_sines), and stereo blocks whose channels differ, so
that on the pair path one half of the wave stops in its first chunk while the other walks on or sits the loop out.

Batches of 3 and 33 blocks (the smallest at which a wave works more than one block and at which the pair path is taken):
the bench's setup on long blocks through k_floor, q9 on long blocks, q9 on short blocks with both halves of k_floor_pair
at work, and a bitrate-managed setup through k_floor_managed (three fits a channel-block).
"""
import numpy as np
import pytest

from tests import checker, floor_split_signals
from tests.feed_cases import FLOOR_KEYS as KEYS, FLOOR_WANT as WANT, chk_for

pytestmark = pytest.mark.gpu
_refs = {}


def reference(name, W, nb):
    """The checker's taps of the batch (name, W, nb), computed once and shared by the cases that run it."""
    key = (name, W, nb)
    if key not in _refs:
        import vorbis_amd
        an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(name), device=0)
        n, nposts = an.blocksizes[W], an.posts[W]
        an.close()
        pcm, kinds = floor_split_signals.batch(nb, checker.SETUPS[name][0], n, 1900 + 7 * nb + W)
        chk = chk_for(name)
        refs = [chk.tap_block(pcm[b], W, W, W, W, -9999.0) for b in range(nb)]
        _refs[key] = (pcm, kinds, refs, nposts)
    return _refs[key]


def run_and_compare(name, W, nb):
    import torch
    import vorbis_amd
    assert torch.cuda.is_available()
    pcm, kinds, refs, nposts = reference(name, W, nb)
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(name), device=0)
    flags = torch.full((nb,), W, dtype=torch.int32).cuda()
    outs = an.analyze(torch.from_numpy(pcm).cuda(), W=W, lW=flags, nW=flags, blocktype=W, ampmax_in=-9999.0, want=WANT)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in outs.items()}
    config = an.config_string()
    an.close()
    bad = []
    for b in range(nb):  # every block
        if checker.compare_block(refs[b], {k: v[b] for k, v in got.items()}, nposts, keys=KEYS, verbose=len(bad) < 3):
            bad.append((b, kinds[b]))
    assert not bad, "checker=%s: %d of %d blocks differ: %s" % (chk_for(name).kind, len(bad), nb, bad[:8])
    # the inputs are what they are meant to be: no fit for silence, a fit for everything else
    for b in range(nb):
        want = [part != "silent" for part in (kinds[b].split("|") * 2)[:2]]
        assert [bool(v) for v in got["post_valid"][b]] == want, (b, kinds[b])
    return config


@pytest.mark.parametrize("nb", [3, 33])
@pytest.mark.parametrize("name", ["44k_stereo_q4", "44k_stereo_q9"])
def test_long_blocks_one_channel_a_wave(name, nb):
    run_and_compare(name, 1, nb)


@pytest.mark.parametrize("name,W,nb", [("44k_stereo_q9", 0, 3), ("44k_stereo_q9", 0, 33), ("44k_stereo_q4", 1, 33)])
def test_paired_channels(name, W, nb, monkeypatch):
    """k_floor_pair: a half of the wave per channel, so the halves of "noise|faint", "faint|noise" and "noise|silent" leave
    the walk at different trips."""
    monkeypatch.setenv("VAMD_TEST_KNOBS", "1")
    monkeypatch.setenv("VAMD_FLOOR_PAIR_MIN", "0")
    assert "VAMD_FLOOR_PAIR_MIN=0" in run_and_compare(name, W, nb)


def test_managed_blocks():
    """k_floor_managed: the three fits of a bitrate-managed block (tests/test_managed.py), one block of every signal."""
    import torch
    import vorbis_amd
    from oracle import ref
    from tests.feed_cases import MANAGED_KEYS as M_KEYS, managed_same as same
    if not ref.available():
        pytest.skip("oracle/_ref not built: the managed setup is packed by the reference build")
    e = ref.RefEncoder(2, 44100, managed=(-1, 128000, -1))
    an = vorbis_amd.Analyzer(e.pack_setup(), 0)
    pcm, kinds = floor_split_signals.batch(len(floor_split_signals.NAMES), 2, 2048, 77)
    o = an.analyze_managed(torch.from_numpy(pcm).cuda(), residue=True)
    torch.cuda.synchronize()
    bad = []
    for i, kind in enumerate(kinds):
        a = e.tap_block_managed(pcm[i])
        k = same(a, {k: o[k][i].cpu().numpy() for k in M_KEYS})
        if k is not None:
            bad.append((i, kind, k))
    assert not bad, bad
