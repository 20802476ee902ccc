"""GPU suite: the persistent transform hands out its channel-blocks by ticket (k_transform: the waves of a workgroup draw
from a counter in its LDS) -- the edges of that counter, not the workload: batches around the worker counts of the two
large persistent kernels of the path (k_transform: grid x waves; k_noise, which keeps its static stride: its grid), the
same context called with large and tiny batches in turn, both size classes in turn, one small mixed-size plan.  The
44.1 kHz q 0.4 stereo setup at LEVEL_FULL; every block of every case is held to tests/checker.py: a batch is a tiling of
eight blocks, the batch's first tile is compared with the checker tensor by tensor, and every other block with the block
of the first tile it repeats, byte for byte.  The counter lives and dies with a workgroup, so there is nothing to read
back between calls: a ticket drawn twice or never shows as a block that is wrong or was never written (the outputs are
filled with NaN / the type's largest integer before every call).

The worker counts are computed as the launch code does (launch_transform, launch_masks in csrc/vamd_batch.h) from the
device's CU count.  A stereo block is two channel-blocks, so the batches either side of a worker count N have N - 2 and
N + 2 channel-blocks (N - 1 and N + 1 where N is odd)."""
import numpy as np
import pytest

from tests import checker

pytestmark = pytest.mark.gpu
SETUP = "44k_stereo_q4"
ALL = ("mdct_raw", "logfft", "logmdct", "noise", "tone", "logmask", "mdct", "posts", "post_valid", "ilogmask",
       "iwork", "nonzero", "local_ampmax", "ampmax_out")
TILE = 8
FLAGS = {1: dict(lW=1, nW=1, blocktype=1), 0: dict(lW=0, nW=0, blocktype=0)}
XF_WAVES, NOISE_TEAMS = 8, 6   # VAMD_XF_WAVES (vamd_kernels.h); noise_teams_per_cu beside the tone chain (vamd_batch.h)


@pytest.fixture(scope="module")
def world():
    """The context all cases share, the eight blocks of either size class with the checker's tensors for them, and the
    worker counts of a full grid."""
    import torch
    import vorbis_amd
    assert torch.cuda.is_available()
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(SETUP), device=0)
    chk = checker.Checker(SETUP)
    rng = np.random.default_rng(3301)
    tiles, refs = {}, {}
    for W in (0, 1):
        n = an.blocksizes[W]
        amps = (10.0 ** rng.uniform(-3, 0, (TILE, 1, 1))).astype(np.float32)
        tiles[W] = ((rng.random((TILE, 2, n), dtype=np.float32) - 0.5) * 2 * amps).astype(np.float32)
        tiles[W][3, 1] = 0  # one silent channel
        refs[W] = [chk.tap_block(tiles[W][b], FLAGS[W]["lW"], W, FLAGS[W]["nW"], FLAGS[W]["blocktype"], -9999.0) for b in range(TILE)]
    w = dict(torch=torch, an=an, chk=chk, tiles={W: torch.from_numpy(tiles[W]).cuda() for W in (0, 1)}, refs=refs)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    w["workers"] = {"k_transform": cus * XF_WAVES, "k_noise": cus * NOISE_TEAMS}
    yield w
    an.close()


def run(w, W, nb):
    """`nb` blocks of size class W through the analysis, into outputs that start as NaN / the largest integer; every block checked"""
    torch, an = w["torch"], w["an"]
    pcm = w["tiles"][W].repeat((nb + TILE - 1) // TILE, 1, 1)[:nb].contiguous()
    outs = an.alloc_outputs(W, nb, ALL)
    for v in outs.values():
        v.fill_(float("nan") if v.is_floating_point() else torch.iinfo(v.dtype).max)
    an.analyze(pcm, W=W, ampmax_in=-9999.0, outs=outs, **FLAGS[W])
    torch.cuda.synchronize()
    head = {k: v[:TILE].cpu().numpy() for k, v in outs.items()}
    bad = 0
    for b in range(min(nb, TILE)):
        bad += checker.compare_block(w["refs"][W][b], {k: v[b] for k, v in head.items()}, an.posts[W], verbose=bad < 3)
    assert bad == 0, "W=%d, %d blocks: checker=%s" % (W, nb, w["chk"].kind)
    for k, v in outs.items():  # block b repeats block b % TILE
        whole = nb // TILE * TILE
        if whole > TILE:
            assert bool((v[:whole].reshape((nb // TILE, TILE) + tuple(v.shape[1:])) == v[:TILE].unsqueeze(0)).all()), (k, W, nb)
        if nb > whole and nb > TILE:
            assert torch.equal(v[whole:], v[:nb - whole]), (k, W, nb)
    return outs


def test_two_channel_blocks(world):
    run(world, 1, 1)


@pytest.mark.parametrize("kernel", ["k_noise", "k_transform"])
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_around_the_worker_count(world, kernel, delta):
    """one stereo block fewer than the workers of a full grid, as many channel-blocks as workers, one block more"""
    run(world, 1, world["workers"][kernel] // 2 + delta)


def test_reset_between_calls_of_different_sizes(world):
    big = world["workers"]["k_transform"] + 2 * TILE + 3
    for nb in (big, 1, big):
        run(world, 1, nb)


def test_alternating_size_classes(world):
    nw = world["workers"]
    for W, nb in ((1, nw["k_noise"] // 2 + 5), (0, nw["k_transform"] + 3), (1, 3), (0, 2), (1, nw["k_transform"] + 1), (0, nw["k_transform"] // 2 + 1)):
        run(world, W, nb)


def test_small_mixed_plan(world):
    """one small analyze_plan call: both size classes in one run, the ampmax chain across them"""
    torch, an, chk = world["torch"], world["an"], world["chk"]
    rng = np.random.default_rng(3302)
    frames = 40000
    gate = np.where((np.arange(frames) % 9000) < 900, 0.5, 0.0005).astype(np.float32)
    raw = ((rng.random((2, 2, frames), dtype=np.float32) - 0.5) * 2 * gate).astype(np.float32)
    streams = torch.from_numpy(raw).cuda()
    plan, _ = an.plan_streams(streams)
    L = an.plan_lists(plan)
    assert plan.nblocks[0] > 4 and plan.nblocks[1] > 4
    pcm_blocks = [an.gather_blocks(plan, W, streams) for W in (0, 1)]
    want = ("mdct", "posts", "post_valid", "iwork", "nonzero", "ampmax_out")
    outs = [an.alloc_outputs(W, plan.nblocks[W], want) for W in (0, 1)]
    states = torch.full((2,), -9999.0, device="cuda")
    an.analyze_plan(plan, pcm_blocks, outs, states)
    torch.cuda.synchronize()
    host = [{k: v.cpu().numpy() for k, v in outs[W].items()} for W in (0, 1)]
    pcm = [p.cpu().numpy() for p in pcm_blocks]
    for s in range(2):
        amp = -9999.0
        for o in L["order"][int(L["stream_start"][s]):int(L["stream_start"][s + 1])]:
            W, i = (int(o) >> 30) & 1, int(o) & 0x3fffffff
            r = chk.tap_block(pcm[W][i], int(L["lW"][W][i]), W, int(L["nW"][W][i]), int(L["blocktype"][W][i]), chk.enc.ampmax_decay(amp, W))
            amp = r["ampmax_out"]
            g = {k: v[i] for k, v in host[W].items()}
            assert np.float32(g["ampmax_out"]) == np.float32(amp), (s, W, i)
            assert checker.compare_block(r, g, an.posts[W], keys=("mdct", "post_valid", "iwork", "nonzero"), verbose=True) == 0, (s, W, i)
        assert np.float32(states[s].item()) == np.float32(amp)
