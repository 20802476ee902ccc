"""GPU suite (-m gpu): the 2048-sample transform against the CPU checker, with logfft tapped and untapped.

Where logfft itself is not tapped, k_transform<11> may form it inside the FFT's last trip and keep only its run peaks
and local_ampmax (xf_tail_fused, k_transform.h); a tapped logfft always takes the hand-over through LDS.  That is the only
thing in which the two runs can differ, so their bit-for-bit equality checks that one choice.  Everything else of the size's
path (the spectrum out of registers, FFT passes 1 + 2 -> 3 and the MDCT's head in registers) is taken in both runs alike and is checked by
the CPU checker alone, which shares no code with the kernels; so is vamd_mdct_forward_batch at 2048.

A persistent wave takes channel-blocks a stride apart (workgroups x waves: 2048 channel-blocks = 1024 stereo blocks
where every CU holds a workgroup of eight waves), so the batch sizes sit on both sides of one and two strides: the
second trip of a wave runs on the samples it fetched during the first.
"""
import numpy as np
import pytest

from tests import checker

pytestmark = pytest.mark.gpu
NAME = "44k_stereo_q4"
TAPPED = ("mdct_raw", "logmdct", "logfft", "local_ampmax", "tone", "posts")
UNTAPPED = ("mdct_raw", "local_ampmax", "tone", "posts")
SHAPES = ((1, 1, 1), (0, 1, 1), (1, 1, 0), (0, 1, 0))  # (lW, W, nW) of a long block


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def an():
    import vorbis_amd
    return vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(NAME), device=0)


@pytest.fixture(scope="module")
def chk():
    return checker.Checker(NAME)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def make_blocks(nb, n, seed):
    """Seeded noise at mixed levels; block 1 (and the one before last) silent, block 2 (and the last) a lone spike."""
    rng = np.random.default_rng(seed)
    amps = (10.0 ** rng.uniform(-4, 0, (nb, 1, 1))).astype(np.float32)
    pcm = ((rng.random((nb, 2, n), dtype=np.float32) - 0.5) * 2 * amps).astype(np.float32)
    special = []
    for silent, spike in ((1, 2), (nb - 2, nb - 1)):
        if 0 < silent < spike < nb:
            pcm[silent] = 0
            pcm[spike] = 0
            pcm[spike, 0, (7 * n) // 16 + 3] = 0.9
            pcm[spike, 1, n - 5] = -0.25  # (under the window's last samples: a long next window keeps it, a short one zeroes it)
            special += [silent, spike]
    return pcm, special


def run(torch, an, pcm, W, lW, nW, want):
    dv = lambda v: torch.from_numpy(np.asarray(v, dtype=np.int32)).cuda()  # noqa: E731
    outs = an.analyze(torch.from_numpy(pcm).cuda(), W=W, lW=dv(lW), nW=dv(nW), ampmax_in=-9999.0, want=want)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items()}


@pytest.mark.parametrize("nb", [3, 8, 1023, 1025, 2047, 2050])
def test_long_blocks_tapped_and_untapped(torch_mod, an, chk, nb):
    n = an.blocksizes[1]
    assert n == 2048
    pcm, special = make_blocks(nb, n, 1100 + nb)
    shape = np.arange(nb) % len(SHAPES)
    if nb > 1024:  # every window shape on a wave's second trip too
        shape[1024:] = (np.arange(nb - 1024) + 1) % len(SHAPES)
    lW = np.array([SHAPES[s][0] for s in shape], dtype=np.int32)
    nW = np.array([SHAPES[s][2] for s in shape], dtype=np.int32)
    tapped = run(torch_mod, an, pcm, 1, lW, nW, TAPPED)
    untapped = run(torch_mod, an, pcm, 1, lW, nW, UNTAPPED)
    for k in UNTAPPED:  # every block: what the two runs have in common
        assert np.array_equal(bits(tapped[k]), bits(untapped[k])), k
    # the CPU checker on the blocks at the batch's ends, round the stride and the special ones (it takes its time per block)
    pick = sorted(set([b for b in list(range(6)) + list(range(1020, 1030)) + list(range(2044, 2052)) + special if 0 <= b < nb]
                      + list(range(max(0, nb - 4), nb))))
    bad = 0
    for b in pick:
        ref = chk.tap_block(pcm[b], int(lW[b]), 1, int(nW[b]), 1, -9999.0)
        bad += checker.compare_block(ref, {k: v[b] for k, v in tapped.items()}, an.posts[1], keys=TAPPED[:-1], verbose=bad < 4)
        bad += checker.compare_block(ref, {k: v[b] for k, v in untapped.items()}, an.posts[1], keys=UNTAPPED[:-1], verbose=bad < 4)
    assert bad == 0, "checker=%s, %d blocks checked" % (chk.kind, len(pick))


def test_short_blocks_keep_their_path(torch_mod, an, chk):
    """(lW, W, nW) = (*, 0, *): the short block's window takes no neighbour into account; its transform is another
    instantiation and must not notice any of this."""
    n = an.blocksizes[0]
    nb = 70
    pcm, special = make_blocks(nb, n, 77)
    z = np.zeros(nb, dtype=np.int32)
    tapped = run(torch_mod, an, pcm, 0, z, z, TAPPED)
    untapped = run(torch_mod, an, pcm, 0, z, z, UNTAPPED)
    for k in UNTAPPED:
        assert np.array_equal(bits(tapped[k]), bits(untapped[k])), k
    bad = 0
    for b in sorted(set([0, 3, nb - 3] + special)):
        ref = chk.tap_block(pcm[b], 0, 0, 0, 1, -9999.0)
        bad += checker.compare_block(ref, {k: v[b] for k, v in tapped.items()}, an.posts[0], keys=TAPPED[:-1], verbose=True)
    assert bad == 0, "checker=%s" % chk.kind


@pytest.mark.parametrize("nf", [1, 63, 4095, 4097, 8200])
def test_mdct_forward_2048(torch_mod, an, chk, nf):
    """vamd_mdct_forward_batch at 2048 (k_mdct_only<11>, sixteen waves per workgroup: 4096 frames in flight where every CU
    holds one), frame counts on both sides of that."""
    n = an.blocksizes[1]
    rng = np.random.default_rng(500 + nf)
    x = ((rng.random((nf, n), dtype=np.float32) - 0.5) * 2).astype(np.float32)
    if nf > 2:
        x[1] = 0
        x[nf - 1] = 0
        x[nf - 1, n // 2 + 1] = 1.0
    y = an.mdct_forward(1, torch_mod.from_numpy(x).cuda()).cpu().numpy()
    for i in sorted(set([0, 1, nf // 2, nf - 2, nf - 1]) & set(range(nf))):
        assert np.array_equal(bits(y[i]), bits(chk.mdct_forward(1, x[i]))), i
    # the rest against the same frames run alone (a one-frame launch: first trip of the first wave)
    for i in sorted(set([4094, 4095, 4096, 8190, 8199]) & set(range(nf))):
        y1 = an.mdct_forward(1, torch_mod.from_numpy(x[i:i + 1].copy()).cuda()).cpu().numpy()[0]
        assert np.array_equal(bits(y[i]), bits(y1)), i
