"""GPU suite: the batch kernels at their own sizes, held to the reference.

The launch sequence (vorbis_amd/csrc/vamd_batch.h) picks kernels by batch size: k_residue_chunks and k_pack_waves
(persistent waves) above 2048 units, k_couple with one wave a unit, the lane-per-block tone walk above 32768
channel-blocks, k_floor_pair for short stereo blocks from 16384 channel-blocks, k_residue with two waves and k_pack for the
layouts beyond stereo.  The soak (tests/soak_lib.py) has the breadth -- fourteen signal kinds, twelve configurations,
random flags -- but its batches stay below every one of those thresholds.  Here the soak's signals and setups go through
batches that are above all of them, unforced (no knob is set), and the context's launch record (vamd_launch_record) is
held against a literal expectation per (configuration, size class), so that a moved threshold fails the test instead of
quietly sending it down the small-batch road.

Two steps, so that the CPU reference is needed D times and every one of the N rows is still checked:
  1. D distinct cases as a batch of D (the small-batch roads) against the reference on the host: status exact, packet and
     ampmax bit-equal.  A case the reference's own quantised values put beyond the setup's integer bound is held to its
     status and ampmax only; its packet is deterministic but unspecified and is left out of both steps.
  2. N blocks -- the cases gathered by an index vector: in order at the front, reversed at the back, seeded random between,
     so every kind sits at both ends of the batch and under every neighbour -- against step 1's tensors gathered by the
     same vector, on the device, stage by stage in pipeline order; the first stage that differs is named with the block,
     its kind and its position modulo 4 (waves a workgroup of the persistent kernels) and 64 (lanes of the tone walk).

Outside the input domain (test_hostile_blocks_on_the_batch_roads): soak_lib.hostile_batch's NaN / Inf / 1e30 / +94 dB blocks
replicated the same way.  Values of INT_MIN / INT_MAX then reach residue_wave_chunks and pack_block_body; what bounds every
index that derives from a value, as read in the kernels:
  - residue_besterror_regs (k_residue.h): the lattice digit m is clamped to [0, quantvals - 1] whatever the arithmetic in
    front of it wrapped to, so index < quantvals ** dim = the book's entries, which bounds len[index]; the exhaustive
    search indexes len[] with its loop counter alone.  A partition's class comes out of a bounded loop (< nparts); an
    output position is off[] (a prefix sum of table constants) plus the lane's run, and every store tests e0 + k < R.cap.
    (|INT_MIN| stays negative and so never sets the range bit here; k_couple has set it: its own bound is 0x7fffff80.)
  - pack_block_body (k_pack.h): book_word refuses an entry outside [0, entries) before it reads lengths or codes -- post
    values, cascade words, residue entries alike; a (class, stage) row is indexed by classes the residue stage bounded; a
    ring slot is the word index masked with VAMD_PK_RING - 1, the ring is flushed before a batch of fields could lap
    it, and ring_flush stores word w only where w < out_words: a packet longer than its row is counted and dropped.
  - tone_seed_block (k_tone.h): seed_level converts the peak with a saturating conversion (NaN -> 0) and clamps the
    result to [0, VAMD_P_LEVELS - 1]; tone_chase_regs indexes by its loop counter and window mask only -- a NaN line
    changes which lines are popped, never where anything is read or written.
"""
import numpy as np
import pytest

from oracle import ref
from tests import soak_lib
from tests.soak_lib import NKINDS

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not ref.available(), reason="oracle/_ref is not built (the reference's sources were not there at build time)")]

CASES = {1: 3 * NKINDS, 0: 2 * NKINDS}     # distinct cases per size class: every kind at least twice, with different draws
CASES_MANAGED = {1: 2 * NKINDS, 0: NKINDS}
# One seed per configuration of soak_lib.CONFIGS.  Kind 11's impulse has one amplitude (2e4) whatever the draw, and in a
# short block at q 0.9 / 0.7 it quantises past the bound wherever the window leaves it whole: those two configurations'
# seeds (339, 170) are ones whose draws put both impulses of the short blocks under the window's skirt.
SEEDS = [101, 102, 339, 104, 105, 106, 170, 108, 109, 110, 111, 112]
STAGES = ("mdct", "logmask", "posts", "post_valid", "iwork", "nonzero", "res_count", "res_class", "res_entries")
WANT = ("status", "ampmax_out", "packets", "packet_bits") + STAGES


@pytest.fixture(autouse=True)
def no_test_knobs(monkeypatch):
    """Nothing here is forced by a knob, whatever the caller's environment holds (tools/alt_paths.sh runs the suite with
    every test knob turned the other way): a context reads its knobs once, at vamd_create, and ignores the test knobs
    without this variable -- so the literal launch records below hold under that tool as well."""
    monkeypatch.delenv("VAMD_TEST_KNOBS", raising=False)


def batch_blocks(ch, cus):
    """N of the VBR batches: past every threshold of the launch sequence, odd, and for stereo more than twice what one trip
    of the persistent residue / pack grids holds (cus x at most 8 resident workgroups x 4 waves)."""
    n = max(32768 // ch + 165, 2 * cus * 8 * 4 + 1 if ch == 2 else 0, 4 * cus, 2049) | 1
    assert n * ch > 32768 + 64 and n > 2048 and n >= 4 * cus and n % 2 == 1 and n % 4 != 0
    assert ch != 2 or n > 2 * cus * 8 * 4
    return n


def managed_blocks(cus):
    n = max(2 * cus * 8 * 4 // 15 + 108, 4 * cus // 15 + 1, 2049 // 15 + 1) | 1
    assert 15 * n > 2 * cus * 8 * 4 and 15 * n > 2048 and 15 * n >= 4 * cus and n % 2 == 1
    return n


def spread(ncases, n, seed):
    """The index vector of a batch of n blocks over ncases cases: in order, seeded random, in reverse order"""
    assert n >= 2 * ncases
    idx = np.empty(n, np.int64)
    idx[:ncases] = np.arange(ncases)
    idx[n - ncases:] = np.arange(ncases)[::-1]
    idx[ncases:n - ncases] = np.random.default_rng(seed).integers(0, ncases, n - 2 * ncases)
    return idx


def rows_differ(a, b):
    """per row of two device tensors: does any bit differ"""
    import torch
    if a.dtype.is_floating_point:
        a, b = a.view(torch.int32), b.view(torch.int32)
    ne = a != b
    return ne.reshape(ne.shape[0], -1).any(1)


def hold_batch_to_cases(big, small, idx, stages, full, nposts, packets, bits, what):
    """Step 2: the N rows of `big` against the rows of `small` that `idx` (device) names.  full: per case, whether it is
    compared in full (device bool); the others are held to status and ampmax alone."""
    import torch
    rows = full[idx]

    def fail(stage, bad):
        r = int(torch.nonzero(bad)[0])
        c = int(idx[r])
        pytest.fail("%s: %s differs in %d of %d blocks, first block %d = case %d (kind %d), block %% 4 = %d, block %% 64 = %d"
                    % (what, stage, int(bad.sum()), len(idx), r, c, c % NKINDS, r % 4, r % 64))
    for stage in ("status", "ampmax_out"):
        bad = rows_differ(big[stage], small[stage][idx])
        if bad.any():
            fail(stage, bad)
    for stage in stages:
        a, b = big[stage], small[stage][idx]
        if stage.endswith("posts"):
            a, b = a[..., :nposts], b[..., :nposts]
        bad = rows_differ(a, b) & rows
        if bad.any():
            fail(stage, bad)
    bad = rows_differ(big[bits], small[bits][idx]) & rows
    if bad.any():
        fail(bits, bad)
    # the packets' own bytes: what lies behind a packet's end differs between the pack kernels
    nbytes = (big[bits] + 7) // 8
    cols = torch.arange(big[packets].shape[-1], device=nbytes.device) < nbytes[..., None]
    bad = ((big[packets] != small[packets][idx]) & cols).reshape(len(idx), -1).any(1) & rows
    if bad.any():
        fail(packets, bad)


# per (configuration of soak_lib.CONFIGS, size class): the launch record of the batch of D, then of the batch of N --
# written from a run on a 256-CU MI355X and checked against vamd_batch.h by reading
LANES = "k_noise k_tone_seed k_tone_chase_regs "   # past 32768 channel-blocks: the tone walk a lane per block
LONG, SHORT = "k_noise k_tone_seed_chase k_floor ", "k_noise_tone k_floor "   # a handful of long / short blocks
STEREO_BIG = (LANES + "k_floor k_couple/64 k_residue_chunks k_pack_waves", LANES + "k_floor_pair k_couple/64 k_residue_chunks k_pack_waves")
NORM_BIG = (LANES + "k_floor k_couple_norm k_residue_chunks k_pack_waves", LANES + "k_floor_pair k_couple_norm k_residue_chunks k_pack_waves")
SIX = LONG + "k_couple_general k_residue/256 k_residue/256 k_pack_pair"   # 5.1: two submaps, k_pack for the batch
MANY = LONG + "k_couple_general k_residue/256 k_pack_pair"
ROADS = {
    (0, 1): (LONG + "k_couple/256 k_residue:team/256 k_pack_pair", STEREO_BIG[0]),
    (0, 0): (SHORT + "k_couple/64 k_residue:team/64 k_pack_pair", STEREO_BIG[1]),
    (1, 1): (LONG + "k_couple_norm k_residue:team/192 k_pack_pair", NORM_BIG[0]),
    (1, 0): (SHORT + "k_couple_norm k_residue:team/64 k_pack_pair", NORM_BIG[1]),
    (2, 1): (LONG + "k_couple/256 k_residue:team/256 k_pack_pair", STEREO_BIG[0]),
    (2, 0): (SHORT + "k_couple/64 k_residue:team/64 k_pack_pair", STEREO_BIG[1]),
    # q -0.1: 2048 bins are more than a wave folds beside its fit (the fold is a launch of its own), and more runs of
    # eight than the team search takes
    (3, 1): ("k_noise k_tone_seed_chase k_tone_fold k_floor k_couple_norm k_residue/256 k_pack_pair",
             LANES + "k_tone_fold k_floor k_couple_norm k_residue_chunks k_pack_waves"),
    (3, 0): (SHORT + "k_couple_norm k_residue:team/64 k_pack_pair", NORM_BIG[1]),
    (4, 1): (SHORT + "k_couple_norm k_residue/256 k_pack_pair", LANES + "k_floor k_couple_norm k_residue/128 k_pack_waves"),   # mono
    (4, 0): (SHORT + "k_couple_norm k_residue/256 k_pack_pair", LANES + "k_floor k_couple_norm k_residue/128 k_pack_waves"),
    # 5.1: the five-channel bundle of a long block keeps four waves (line 338: bundle * n2 > 4096), the LFE's two
    (5, 1): (SIX, LANES + "k_floor k_couple_general k_residue/256 k_residue/128 k_pack"),
    (5, 0): (SIX, LANES + "k_floor k_couple_general k_residue/128 k_residue/128 k_pack"),
    (6, 1): (SIX, LANES + "k_floor k_couple_general k_residue/256 k_residue/128 k_pack"),
    (6, 0): (SIX, LANES + "k_floor k_couple_general k_residue/128 k_residue/128 k_pack"),
    (7, 1): (LONG + "k_couple/256 k_residue/256 k_pack_pair", LANES + "k_floor k_couple/64 k_residue/128 k_pack_waves"),   # uncoupled stereo
    (7, 0): (SHORT + "k_couple/64 k_residue/256 k_pack_pair", LANES + "k_floor_pair k_couple/64 k_residue/128 k_pack_waves"),
    (8, 1): (MANY, LANES + "k_floor k_couple_general k_residue/128 k_pack_waves"),   # four channels
    (8, 0): (MANY, LANES + "k_floor k_couple_general k_residue/128 k_pack_waves"),
    (9, 1): (LONG + "k_couple_norm k_residue:team/128 k_pack_pair", NORM_BIG[0]),   # 22 kHz: 1024 / 512 samples
    (9, 0): (SHORT + "k_couple/64 k_residue:team/64 k_pack_pair", STEREO_BIG[1]),
    (10, 1): (LONG + "k_couple/256 k_residue:team/256 k_pack_pair", STEREO_BIG[0]),
    (10, 0): (SHORT + "k_couple/64 k_residue:team/64 k_pack_pair", STEREO_BIG[1]),
    (11, 1): (MANY, LANES + "k_floor k_couple_general k_residue/256 k_pack_waves"),   # eight channels: bundle * n2 > 4096
    (11, 0): (MANY, LANES + "k_floor k_couple_general k_residue/128 k_pack_waves"),
}


def test_the_expectations_reach_every_batch_kernel():
    """The tables themselves: between them the batches of N take every kernel the launch sequence has for a batch."""
    words = {w.split("/")[0] for t in (ROADS, MANAGED_ROADS) for small, big in t.values() for w in big.split()}
    assert words >= {"k_noise", "k_tone_seed", "k_tone_chase_regs", "k_floor", "k_floor_pair", "k_couple", "k_couple_norm", "k_couple_general",
                     "k_residue_chunks", "k_residue", "k_pack_waves", "k_pack", "k_floor_managed", "k_tone_fold"}
    assert {w for small, big in ROADS.values() for w in small.split()} >= {"k_pack_pair", "k_residue:team/256", "k_residue/256"}


@pytest.mark.parametrize("W", [1, 0])
@pytest.mark.parametrize("ci", range(len(soak_lib.CONFIGS)))
def test_soak_signals_on_the_batch_roads(ci, W):
    import torch
    import vorbis_amd
    ch, rate, q, coupled = soak_lib.CONFIGS[ci]
    what = "%d ch %d Hz q %.1f coupled=%s W=%d" % (ch, rate, q, coupled, W)
    e = ref.RefEncoder(ch, rate, q, coupled=coupled)
    an = vorbis_amd.Analyzer(e.pack_setup(), 0)
    D, n = CASES[W], e.blocksize(W)
    rng = np.random.default_rng([SEEDS[ci], W])
    x = soak_lib.signals(rng, D, ch, n)
    lW, nW, bt, amp_in = soak_lib.draw_flags(rng, D, W)
    # the reference, once per case, and what it says of the domain -- before anything runs on the GPU
    taps = [e.tap_block(x[k], int(lW[k]), W, int(nW[k]), int(bt[k]), float(amp_in[k])) for k in range(D)]
    want_st = np.stack([an.beyond_quant_limit(W, a["iwork"]) for a in taps])
    beyond = want_st.any(1)
    assert not beyond[np.arange(D) % NKINDS < 12].any(), \
        "%s: a case of kinds 0-11 is beyond the integer bound: cases %s (another seed for this configuration)" % (what, np.nonzero(beyond)[0].tolist())
    # step 1: the D cases on the small-batch roads against the reference
    dev = {k: torch.from_numpy(v).cuda() for k, v in (("x", x), ("lW", lW), ("nW", nW), ("bt", bt), ("amp", amp_in))}
    small = an.analyze(dev["x"], W=W, lW=dev["lW"], nW=dev["nW"], blocktype=dev["bt"], ampmax_in=dev["amp"], want=WANT)
    torch.cuda.synchronize()
    roads_small = " ".join(an.launch_record(W))
    assert an.input_status() == (int(want_st.astype(bool).sum()), 0), what
    st, rows, bits, amps = (small[k].cpu().numpy() for k in ("status", "packets", "packet_bits", "ampmax_out"))
    for k, a in enumerate(taps):
        assert np.array_equal(st[k], want_st[k]), (what, "status of case", k, k % NKINDS, st[k].tolist(), want_st[k].tolist())
        assert np.float32(amps[k]) == np.float32(a["ampmax_out"]), (what, "ampmax of case", k, k % NKINDS)
        if not beyond[k]:
            assert a["packet_matches_real"] and vorbis_amd.packet_bytes(rows[k], bits[k]) == a["packet"], (what, "packet of case", k, k % NKINDS)
    # step 2: N blocks on the batch roads against step 1
    N = batch_blocks(ch, torch.cuda.get_device_properties(0).multi_processor_count)
    idx = torch.from_numpy(spread(D, N, SEEDS[ci])).cuda()
    big = an.analyze(dev["x"][idx], W=W, lW=dev["lW"][idx], nW=dev["nW"][idx], blocktype=dev["bt"][idx], ampmax_in=dev["amp"][idx], want=WANT)
    torch.cuda.synchronize()
    roads_big = " ".join(an.launch_record(W))
    print("ROADS (%d, %d): N = %d, cases %d in full + %d beyond the bound\n    small %s\n    big   %s" % (ci, W, N, int((~beyond).sum()), int(beyond.sum()), roads_small, roads_big))
    assert an.input_status() == (int((big["status"] != 0).sum()), 0), what
    hold_batch_to_cases(big, small, idx, STAGES, torch.from_numpy(~beyond).cuda(), an.posts[W], "packets", "packet_bits", what)
    assert (ci, W) in ROADS, "%s: no expectation for its launch record" % what
    assert roads_small == ROADS[ci, W][0], (what, roads_small)
    assert roads_big == ROADS[ci, W][1], (what, roads_big)
    an.close()


MANAGED_STAGES = ("mdct", "logmask", "m_posts", "m_post_valid", "m_iwork", "m_nonzero", "m_res_count", "m_res_class", "m_res_entries")
M_SMALL, M_BIG = "k_noise_tone k_tone_fold k_floor_managed ", "k_noise k_tone_seed_chase k_tone_fold k_floor_managed "
# (the 5.1 setup's 28 / 14 blocks are more than 64 channel-blocks: the tone chain runs beside the noise mask already)
MANAGED_ROADS = {
    (0, 1): (M_SMALL + "k_couple/256 k_residue:team/256 k_pack_pair", M_BIG + "k_couple/64 k_residue_chunks k_pack_waves"),
    (0, 0): (M_SMALL + "k_couple/64 k_residue:team/64 k_pack_pair", M_BIG + "k_couple/64 k_residue_chunks k_pack_waves"),
    (1, 1): (M_SMALL + "k_couple_norm k_residue:team/192 k_pack_pair", M_BIG + "k_couple_norm k_residue_chunks k_pack_waves"),
    (1, 0): (M_SMALL + "k_couple_norm k_residue:team/64 k_pack_pair", M_BIG + "k_couple_norm k_residue_chunks k_pack_waves"),
    (2, 1): (M_BIG + "k_couple_general k_residue/256 k_residue/256 k_pack_pair", M_BIG + "k_couple_general k_residue/256 k_residue/128 k_pack"),
    (2, 0): (M_BIG + "k_couple_general k_residue/256 k_residue/256 k_pack_pair", M_BIG + "k_couple_general k_residue/128 k_residue/128 k_pack"),
    (3, 1): (M_SMALL + "k_couple_norm k_residue/256 k_pack_pair", M_BIG + "k_couple_norm k_residue/128 k_pack_waves"),
    (3, 0): (M_SMALL + "k_couple_norm k_residue/256 k_pack_pair", M_BIG + "k_couple_norm k_residue/128 k_pack_waves"),
}


@pytest.mark.parametrize("W", [1, 0])
@pytest.mark.parametrize("mi", range(len(soak_lib.MANAGED)))
def test_managed_candidates_on_the_batch_roads(mi, W):
    """The soak's four bitrate-managed setups, all fifteen candidate packets a block: fifteen units a block through the
    batch residue and pack kernels, the tone fold as a launch of its own, k_floor_managed.
    vamd_input_status() is held to a range here, not to the number of non-zero status bytes: a channel-block counts once
    for every one of its fifteen candidates that finds it unflagged and beyond the bound, and the candidates' units race for
    the flag (include/vorbis_amd.h: "up to fifteen times") -- the count is not deterministic and must not be tightened."""
    import torch
    import vorbis_amd
    ch, rates = soak_lib.MANAGED[mi]
    what = "managed %d ch %s W=%d" % (ch, rates, W)
    e = ref.RefEncoder(ch, 44100, managed=rates)
    an = vorbis_amd.Analyzer(e.pack_setup(), 0)
    D, n, bt = CASES_MANAGED[W], e.blocksize(W), 1 if W else 0
    rng = np.random.default_rng([200 + mi, W])
    x = soak_lib.signals(rng, D, ch, n)
    lW, nW = soak_lib.draw_flags(rng, D, W, managed=True)
    taps = [e.tap_block_managed(x[k], int(lW[k]), W, int(nW[k]), bt) for k in range(D)]
    want_st = np.stack([np.bitwise_or.reduce([an.beyond_quant_limit(W, a["m_iwork"][j]) for j in range(15)]) for a in taps])
    beyond = want_st.any(1)
    assert not beyond[np.arange(D) % NKINDS < 12].any(), \
        "%s: a case of kinds 0-11 is beyond the integer bound: cases %s (another seed for this setup)" % (what, np.nonzero(beyond)[0].tolist())
    dev = {k: torch.from_numpy(v).cuda() for k, v in (("x", x), ("lW", lW), ("nW", nW))}
    small = an.analyze_managed(dev["x"], W=W, lW=dev["lW"], nW=dev["nW"], blocktype=bt, residue=True, packets=True, want=("status",))
    torch.cuda.synchronize()
    roads_small = " ".join(an.launch_record(W))
    flagged, nz = an.input_status(), int(want_st.astype(bool).sum())   # (a channel-block counts once per candidate that is beyond the bound)
    assert nz <= flagged[0] <= 15 * nz and flagged[1] == 0, (what, flagged, nz)
    st, rows, bits, amps = (small[k].cpu().numpy() for k in ("status", "m_packets", "m_packet_bits", "ampmax_out"))
    for k, a in enumerate(taps):
        assert np.array_equal(st[k], want_st[k]), (what, "status of case", k, k % NKINDS, st[k].tolist(), want_st[k].tolist())
        assert np.float32(amps[k]) == np.float32(a["ampmax_out"]), (what, "ampmax of case", k, k % NKINDS)
        if not beyond[k]:
            assert a["packets_match_real"] and [vorbis_amd.packet_bytes(rows[k, j], bits[k, j]) for j in range(15)] == a["m_packets"], \
                (what, "packets of case", k, k % NKINDS)
    N = managed_blocks(torch.cuda.get_device_properties(0).multi_processor_count)
    idx = torch.from_numpy(spread(D, N, 200 + mi)).cuda()
    big = an.analyze_managed(dev["x"][idx], W=W, lW=dev["lW"][idx], nW=dev["nW"][idx], blocktype=bt, residue=True, packets=True, want=("status",))
    torch.cuda.synchronize()
    roads_big = " ".join(an.launch_record(W))
    print("ROADS managed (%d, %d): N = %d, cases %d in full + %d beyond the bound\n    small %s\n    big   %s" % (mi, W, N, int((~beyond).sum()), int(beyond.sum()), roads_small, roads_big))
    flagged, nz = an.input_status(), int((big["status"] != 0).sum())
    assert nz <= flagged[0] <= 15 * nz and flagged[1] == 0, (what, flagged, nz)
    hold_batch_to_cases(big, small, idx, MANAGED_STAGES, torch.from_numpy(~beyond).cuda(), an.posts[W], "m_packets", "m_packet_bits", what)
    assert (mi, W) in MANAGED_ROADS, "%s: no expectation for its launch record" % what
    assert roads_small == MANAGED_ROADS[mi, W][0], (what, roads_small)
    assert roads_big == MANAGED_ROADS[mi, W][1], (what, roads_big)
    for word in ("k_floor_managed", "k_tone_fold"):
        assert word in roads_big.split(), (what, roads_big)
    an.close()


# (48 short stereo blocks are more than 64 channel-blocks: the tone chain runs beside the noise mask, not in its launch)
HOSTILE_ROADS = {
    (0, 1): ROADS[0, 1], (0, 0): (LONG + "k_couple/64 k_residue:team/64 k_pack_pair", STEREO_BIG[1]),
    (1, 1): ROADS[1, 1], (1, 0): (LONG + "k_couple_norm k_residue:team/64 k_pack_pair", NORM_BIG[1]),
    (2, 1): ROADS[5, 1], (2, 0): ROADS[5, 0],
    (3, 1): (SHORT + "k_couple/256 k_residue/256 k_pack_pair", LANES + "k_floor k_couple/64 k_residue/128 k_pack_waves"),   # mono, 22 kHz
    (3, 0): (SHORT + "k_couple/64 k_residue/256 k_pack_pair", LANES + "k_floor k_couple/64 k_residue/128 k_pack_waves"),
}


@pytest.mark.parametrize("W", [1, 0])
@pytest.mark.parametrize("hi", range(len(soak_lib.HOSTILE_CONFIGS)))
def test_hostile_blocks_on_the_batch_roads(hi, W):
    """soak_lib.hostile_batch's 48 blocks -- sixteen of them with a NaN, an Inf, 1e30, FLT_MAX or a sine 94 dB over full
    scale in one channel -- replicated to a batch on the batch roads, held to what soak_lib.run_hostile holds the 48 to: the
    non-finite bit on exactly the channel that holds the sample, the context's count and verdict, and every replica of a
    clean block equal to its twin of the small batch in full.  (The module's docstring: what bounds the indices.)"""
    import torch
    import vorbis_amd
    from tests.soak_lib import NONFINITE
    ch, rate, q = soak_lib.HOSTILE_CONFIGS[hi]
    what = "hostile %d ch %d Hz q %.1f W=%d" % (ch, rate, q, W)
    e = ref.RefEncoder(ch, rate, q)
    an = vorbis_amd.Analyzer(e.pack_setup(), 0)
    D, n, bt = 48, e.blocksize(W), 1 if W else 0
    x, lW, nW, want, loud = soak_lib.hostile_batch(np.random.default_rng([300 + hi, W]), D, ch, n, W)
    hostile = want.any(1)
    taps = {k: e.tap_block(x[k], int(lW[k]), W, int(nW[k]), bt, -9999.0) for k in range(D) if not hostile[k]}
    want_r = {k: an.beyond_quant_limit(W, a["iwork"]) for k, a in taps.items()}
    beyond = np.array([k in want_r and bool(want_r[k].any()) for k in range(D)])
    assert set(np.nonzero(beyond)[0].tolist()) <= set(loud), (what, "an ordinary block is beyond the integer bound")
    dev = {k: torch.from_numpy(v).cuda() for k, v in (("x", x), ("lW", lW), ("nW", nW))}
    small = an.analyze(dev["x"], W=W, lW=dev["lW"], nW=dev["nW"], blocktype=bt, want=WANT)
    torch.cuda.synchronize()
    roads_small = " ".join(an.launch_record(W))
    st, rows, bits, amps = (small[k].cpu().numpy() for k in ("status", "packets", "packet_bits", "ampmax_out"))
    assert np.array_equal(st & NONFINITE, want), (what, np.argwhere((st & NONFINITE) != want)[:8].tolist())
    assert an.input_status() == (int((st != 0).sum()), 0) and an.last_input_code == vorbis_amd.VAMD_ENONFINITE, what
    for k, a in taps.items():
        assert np.array_equal(st[k], want_r[k]), (what, "status of block", k, st[k].tolist(), want_r[k].tolist())
        assert np.float32(amps[k]) == np.float32(a["ampmax_out"]), (what, "ampmax of block", k)
        if not beyond[k]:
            assert vorbis_amd.packet_bytes(rows[k], bits[k]) == a["packet"], (what, "packet of block", k)
    N = batch_blocks(ch, torch.cuda.get_device_properties(0).multi_processor_count)
    idx_h = spread(D, N, 300 + hi)
    idx = torch.from_numpy(idx_h).cuda()
    big = an.analyze(dev["x"][idx], W=W, lW=dev["lW"][idx], nW=dev["nW"][idx], blocktype=bt, want=WANT)
    torch.cuda.synchronize()
    roads_big = " ".join(an.launch_record(W))
    print("ROADS hostile (%d, %d): N = %d, blocks %d clean + %d beyond the bound + %d non-finite\n    small %s\n    big   %s"
          % (hi, W, N, int((~hostile & ~beyond).sum()), int(beyond.sum()), int(hostile.sum()), roads_small, roads_big))
    stb = big["status"]
    assert torch.equal(stb & NONFINITE, torch.from_numpy(want).cuda()[idx]), what
    assert an.input_status() == (int((stb != 0).sum()), 0) and an.last_input_code == vorbis_amd.VAMD_ENONFINITE, what
    # the blocks without a non-finite sample: status and ampmax of all of them, the clean ones in full
    quiet = torch.from_numpy(~hostile).cuda()[idx]
    for stage in ("status", "ampmax_out"):
        bad = rows_differ(big[stage], small[stage][idx]) & quiet
        assert not bad.any(), (what, stage, "of block", int(torch.nonzero(bad)[0]))
    clean = torch.from_numpy(~hostile & ~beyond).cuda()
    only = torch.nonzero(clean[idx])[:, 0]
    hold_batch_to_cases({k: v[only] for k, v in big.items()}, small, idx[only], STAGES, clean, an.posts[W], "packets", "packet_bits", what)
    assert (hi, W) in HOSTILE_ROADS, "%s: no expectation for its launch record" % what
    assert roads_small == HOSTILE_ROADS[hi, W][0], (what, roads_small)
    assert roads_big == HOSTILE_ROADS[hi, W][1], (what, roads_big)
    an.close()
