"""CPU suite: the two extrapolated ends of a stream on the case table of tests/stream_edge_cases.py -- streams at the edges
of the input domain, lengths either side of every line lib/block.c:417-458 and :474-512 draw -- through the reference's
application loop and through vamd_plan_streams_whole's pieces compiled for the host (tests/emul): the block list and every
block's samples, compared as uint32.  The same table then runs on the GPU (tests/test_stream_ends_gpu.py), whose forms of
lpc_from_data and lpc_predict (k_lpc.h, #if VAMD_GPU) are not the ones compiled here; the reach tests below are what
gives that module its teeth, and they look at the reference's records alone.

Why the GPU module compares SAMPLES and not packets (census(), run by hand: python -m tests.test_stream_ends_cpu): over
the whole table (250 streams, 2293 blocks) 69 blocks hold denormal samples that the reference's fp32 predictor chain
produced (44k_stereo_q4 16, 44k_stereo_qm1 29, 8k_mono_q3 3, 22k_stereo_q4 3, 44k_51_q3 18), and flushing those samples
to zero changes the packet of 0 of the 69 -- while it makes the sample comparison below fail on all 69."""
import numpy as np
import pytest

from oracle import ref
from tests import stream_edge_cases as sc

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")
SETUP_NAMES = tuple(sc.SETUPS)
_EMUL = {}


def emul_of(setup):
    from tests.emul.emul import Emul
    if setup not in _EMUL:
        _EMUL[setup] = Emul(sc.encoder(setup).pack_setup())
    return _EMUL[setup]


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def ends_of(setup, i):
    """-> per block of case i of the reference's records: (the block's samples in the head room, those in the tail)"""
    bs = sc.SETUPS[setup][3]
    recs, frames = sc.records(setup)[i], sc.case_list(setup)[i][1]
    out = []
    for b, begin in zip(recs, sc.begins_of(recs, bs)):
        h, t = sc.regions(begin, bs[b["W"]], frames, bs[1])
        out.append((b["pcm"][:, h], b["pcm"][:, t]))
    return out


@pytest.mark.parametrize("setup", SETUP_NAMES)
def test_the_tables_block_sizes_are_the_references(setup):
    enc = sc.encoder(setup)
    assert (enc.blocksize(0), enc.blocksize(1)) == sc.SETUPS[setup][3]
    assert enc.channels == sc.SETUPS[setup][0]
    bs1 = sc.SETUPS[setup][3][1]
    assert sc.FULL_FRAMES[bs1] >= sc.n_head(bs1) + bs1   # the tail's fit sees none of the head's samples
    assert len(set(sc.case_list(setup))) == len(sc.case_list(setup))


@pytest.mark.parametrize("setup", SETUP_NAMES)
def test_host_bodies_match_the_reference(setup):
    """every case: the reference reports no error and ends the stream with an e_o_s block; tests/emul's whole_stream gives
    its block list (W, lW, nW, blocktype), its block positions and every block's samples bit for bit"""
    ch, _, _, bs = sc.SETUPS[setup]
    em = emul_of(setup)
    assert em.bs == bs and em.channels == ch
    for i, (kind, frames) in enumerate(sc.case_list(setup)):
        recs, x = sc.records(setup)[i], sc.signals(setup)[i]
        what = "%s, %d frames" % (kind, frames)
        assert recs and all(b["error"] == 0 and b["packet"] is not None for b in recs), what
        assert recs[-1]["eos"] == 1 and not any(b["eos"] for b in recs[:-1]), what
        assert recs[-1]["granulepos"] == frames, what
        assert all(np.isfinite(b["pcm"]).all() for b in recs), what
        buf, kinds, begins = em.whole_stream(x, write_frames=sc.WRITE_FRAMES)
        assert np.isfinite(buf).all(), what
        assert len(kinds) == len(recs), (what, len(kinds), len(recs))
        assert [int(b) for b in begins] == sc.begins_of(recs, bs), what
        assert np.array_equal(u32(buf[:, bs[1] // 2:bs[1] // 2 + frames]), u32(x)), what + ": the real samples changed"
        for k, b in enumerate(recs):
            kd = int(kinds[k])
            assert (kd & 1, (kd >> 1) & 1, (kd >> 2) & 1, (kd >> 3) & 1) == (b["W"], b["lW"], b["nW"], b["blocktype"]), (what, k)
            got = buf[:, int(begins[k]):int(begins[k]) + bs[b["W"]]]
            diff = np.nonzero((u32(got) != u32(b["pcm"])).any(axis=0))[0]
            assert not len(diff), "%s: block %d of %d differs first at sample %d: %s %d" % (
                (what, k, len(recs), diff[0]) + sc.where_of(int(begins[k]), int(diff[0]), frames, bs[1]))


# ---- reach: on the reference's records alone ----
@pytest.mark.parametrize("setup", SETUP_NAMES)
def test_reach_denormals_out_of_both_extrapolations(setup):
    """some case's blocks hold denormal samples in the head room, some case's in the tail: what a predictor that flushes
    denormals, or rounds one product differently, gets wrong (8 kHz, whose 512-sample blocks show 256 samples of head room:
    held to the tail only)"""
    head = tail = 0
    for i in sc.full_cases(setup):
        ends = ends_of(setup, i)
        head += any(sc.is_denormal(h).any() for h, _ in ends)
        tail += any(sc.is_denormal(t).any() for _, t in ends)
    assert tail >= 1
    assert head >= 1 or setup == "8k_mono_q3"


@pytest.mark.parametrize("setup", SETUP_NAMES)
def test_reach_the_line_below_which_the_fit_gives_up(setup):
    """Levinson-Durbin's `error < epsilon` (lib/lpc.c:91): a noise amplitude whose two extrapolations are entirely zero
    although its samples are not, and the next amplitude up, whose extrapolations are not zero"""
    kinds = [k for k, _ in sc.case_list(setup)]
    zero = []
    for a in sc.NOISE_AMPS:
        i = kinds.index("noise_" + a)
        assert sc.signals(setup)[i].all()
        ends = ends_of(setup, i)
        assert sum(h.size for h, _ in ends) and sum(t.size for _, t in ends)
        zero.append(not any(h.any() or t.any() for h, t in ends))
    assert zero[0] and not zero[-1]
    assert any(z and not nz for z, nz in zip(zero, zero[1:]))
    assert zero == sorted(zero, reverse=True), "one line: zero below it, not zero above"


@pytest.mark.parametrize("setup", SETUP_NAMES)
def test_reach_block_sizes_and_stream_ends(setup):
    bs = sc.SETUPS[setup][3]
    seen = set()
    for (kind, frames), recs in zip(sc.case_list(setup), sc.records(setup)):
        seen |= set(b["W"] for b in recs)
        assert recs[-1]["eos"] == 1, (kind, frames)
        # the last block reaches into the tail, the first into the head room
        begins = sc.begins_of(recs, bs)
        assert begins[0] < bs[1] // 2 and begins[-1] + bs[recs[-1]["W"]] > bs[1] // 2 + frames, (kind, frames)
    assert seen == ({0, 1} if bs[0] != bs[1] else {0})
    # lengths either side of every line: order * 2 samples for either fit, half a long block, a long block, n_head
    lengths = set(n for k, n in sc.case_list(setup) if k == "noise_0.4")
    for line in (32, 64, bs[1] // 2, bs[1], sc.n_head(bs[1])):
        assert any(n < line for n in lengths) and any(n > line for n in lengths), line
    assert {32, 64, sc.n_head(bs[1])} <= lengths


# ---- the measurement (not a test) ----
def census(setup):
    """-> (blocks holding denormal samples in their extrapolated parts, how many of their packets change when those samples
    are flushed to zero): tap_block over both forms of the block, the chain's state as the stream had it"""
    enc = sc.encoder(setup)
    blocks = changed = 0
    for i in range(len(sc.case_list(setup))):
        for b, (h, t) in zip(sc.records(setup)[i], ends_of(setup, i)):
            if not (sc.is_denormal(h).any() or sc.is_denormal(t).any()):
                continue
            blocks += 1
            flushed = np.where(sc.is_denormal(b["pcm"]), np.float32(0), b["pcm"])
            args = (b["lW"], b["W"], b["nW"], b["blocktype"], b["ampmax_in"])
            changed += enc.tap_block(b["pcm"], *args)["packet"] != enc.tap_block(flushed, *args)["packet"]
    return blocks, changed


if __name__ == "__main__":
    for name in SETUP_NAMES:
        nb = sum(len(r) for r in sc.records(name))
        print("%-16s %d streams, %d blocks; %d blocks hold extrapolated denormals, %d of their packets change when flushed"
              % ((name, len(sc.records(name)), nb) + census(name)))
