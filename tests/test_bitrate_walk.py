"""The bitrate manager's walk (vorbis_amd/csrc/k_bitrate.h, vorbis_bitrate_addblock of lib/bitrate.c:73-227) held to
the reference encoder on whole ABR / CBR / min-max streams, CPU only: the reference's own fifteen candidates of every
block go through the host-compiled walk, the handed-out packet is rebuilt from the chosen one, and it must equal the
packet the reference's application loop emitted, byte for byte.  The branches those streams do not reach (max forcing,
truncation) are stepped through by hand.  Managed blobs come from bitrate_host.managed_blob: the oracle's packer, or the
recorded section where that packer predates it."""
import numpy as np
import pytest

from oracle import ref
from tests import bitrate_host as bh

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built (needs /root/reference)")


@pytest.fixture(scope="module")
def walk_lib():
    return bh.build()


def run_config(lib, ch, rates, kind, seconds=4.0, seed=7):
    x = bh.signal(kind, ch, int(44100 * seconds), seed)
    recs = ref.RefEncoder(ch, 44100, managed=rates).encode_stream(x)
    tap = ref.RefEncoder(ch, 44100, managed=rates)
    hw = bh.HostWalk(lib, bh.managed_blob(ch, rates))
    cands = [tap.tap_block_managed(r["pcm"], r["lW"], r["W"], r["nW"], r["blocktype"], r["ampmax_in"])["m_packets"] for r in recs]
    sizes = np.array([[len(p) for p in c] for c in cands], np.int32)
    choice, fin, flags = hw.walk(hw.new_state(), sizes, [r["W"] for r in recs])
    bad = [k for k, r in enumerate(recs) if bh.handed_out(cands[k][choice[k]], int(fin[k])) != r["packet"]]
    return recs, choice, flags, bad


def test_blob_carries_the_manager_only_when_managed():
    vbr = ref.RefEncoder(2, 44100, 0.4).pack_setup()
    assert bh.section_offset(vbr) == 0
    for name, ch, rates, kind in bh.CONFIGS:
        packed = ref.RefEncoder(ch, 44100, managed=rates).pack_setup()
        if bh.section_offset(packed):
            # an oracle built from this packer: its blob is exactly the section-less one with the recorded section
            plain = packed[:bh.section_offset(packed)].copy()
            plain[bh.OFF_BITRATE:bh.OFF_BITRATE + 4] = 0
            plain[12:16] = np.frombuffer(np.uint32(plain.size).tobytes(), np.uint8)
            assert np.array_equal(bh.graft_section(plain, bh.recorded_section(ch, 44100, rates)), packed), name
    blob = bh.managed_blob(2, (-1, 128000, -1))
    t = bh.tab_from_blob(blob)
    assert t.short_per_long == 8 and t.rate == 44100 and t.avgfloat == 7.0 and t.reservoir_bits > 0
    # rint(1. * avg_rate * halfsamples / ratesamples), lib/bitrate.c:41
    assert t.avg_bitsper == int(np.rint(128000.0 * 128 / 44100)) and t.min_bitsper == 0 and t.max_bitsper == 0


@pytest.mark.parametrize("name,ch,rates,kind", bh.CONFIGS, ids=[c[0] for c in bh.CONFIGS])
def test_walk_emits_the_reference_packets(walk_lib, name, ch, rates, kind):
    recs, choice, flags, bad = run_config(walk_lib, ch, rates, kind)
    assert len(recs) > 50
    assert not bad, "%s: %d of %d packets differ from the reference's (first at block %d)" % (name, len(bad), len(recs), bad[0])


def test_branches_the_reference_streams_reach(walk_lib):
    """On the reference's own streams the floater's slew clamp, min forcing and zero padding fire (and are then held to
    its packets above).  libvorbisenc's reservoirs (two seconds of the max rate) never filled in streams of a few seconds
    whatever the signal tried (white, spiky, tonal, impulsive), so max forcing and truncation are pinned by the
    hand-worked cases below instead."""
    seen = 0
    for name, ch, rates, kind in bh.CONFIGS:
        _, _, flags, bad = run_config(walk_lib, ch, rates, kind)
        assert not bad, name
        for f in flags:
            seen |= int(f)
    for bit, what in ((bh.SLEW_CLAMPED, "slew clamp"), (bh.MIN_FORCED, "min forcing"), (bh.PADDED, "padding")):
        assert seen & bit, what + " never fired"


def _tab(**kw):
    t = bh.BitrateTab()
    t.short_per_long, t.rate, t.reservoir_bias, t.slew_damp, t.avgfloat = 8, 44100, 0.1, 1.5, 7.0
    for k, v in kw.items():
        setattr(t, k, v)
    return t


def test_max_forcing_and_truncation_worked_by_hand(walk_lib):
    """lib/bitrate.c:152-178 and :194-219 stepped through by hand on a nearly full max reservoir."""
    blob = bh.managed_blob(2, (-1, 128000, -1))
    hw = bh.HostWalk(walk_lib, blob)
    hw.tab = _tab(max_bitsper=100, reservoir_bits=1000, minmax_reservoir=900)
    st = hw.new_state()
    # short block, every candidate 50 bytes = 400 bits > max_target 100: 900 + 300 > 1000 walks the choice below 0;
    # maxsize = (100 + (1000 - 900)) / 8 = 25 bytes; this_bits 200 -> reservoir 900 + 100 = 1000
    c, fin, fl = hw.walk(st, [[50] * 15], [0])
    assert (c[0], fin[0]) == (0, 25) and fl[0] == bh.MAX_FORCED | bh.BELOW_ZERO | bh.TRUNCATED and st.minmax_reservoir == 1000
    # candidates growing with the index: the walk steps down and stops at the first candidate that fits
    st2 = hw.new_state()
    st2.minmax_reservoir = 950
    sizes = [[10 + 2 * k for k in range(15)]]       # candidate 7: 24 bytes = 192 bits; 950 + 92 > 1000
    c, fin, fl = hw.walk(st2, sizes, [0])
    # 6: 176 bits, 950 + 76 > 1000; 5: 160, +60 > 1000; 4: 144, 994 <= 1000 -> choice 4, 18 bytes, reservoir 950 + 44
    assert (c[0], fin[0]) == (4, 18) and fl[0] == bh.MAX_FORCED and st2.minmax_reservoir == 994
    # choice < 0 but candidate 0 already short enough: not cut
    hw.tab = _tab(max_bitsper=100, reservoir_bits=1000, minmax_reservoir=900)
    st3 = hw.new_state()
    c, fin, fl = hw.walk(st3, [[20] + [50] * 14], [0])   # 0: 160 bits, 900 + 60 <= 1000 -> stops at 0 without going below
    assert (c[0], fin[0]) == (0, 20) and fl[0] == bh.MAX_FORCED
    st4 = hw.new_state()
    st4.minmax_reservoir = 990
    c, fin, fl = hw.walk(st4, [[13] + [50] * 14], [0])   # 0: 104 bits, 990 + 4 <= 1000 ... maxsize (100 + 10) / 8 = 13
    assert (c[0], fin[0]) == (0, 13) and fl[0] == bh.MAX_FORCED


def test_final_bits_of_cut_and_padded_packets(walk_lib):
    blob = bh.managed_blob(2, (-1, 128000, -1))
    hw = bh.HostWalk(walk_lib, blob)
    assert hw.final_bits(1001, 126) == 1001          # untouched: the candidate's own oggpack_bits()
    assert hw.final_bits(1001, 100) == 800           # oggpack_writetrunc(b, 100 * 8)
    assert hw.final_bits(1001, 130) == 1001 + 8 * 4  # four oggpack_write(b, 0, 8) after the last write


def _create(blob):
    import ctypes as C
    import vorbis_amd
    L = vorbis_amd.load_library()
    h = C.c_void_p()
    r = L.vamd_create_abi(C.byref(h), C.c_void_p(blob.ctypes.data), blob.size, -1, L.vamd_abi_version())
    assert not h.value
    return r


def test_create_rejects_a_bad_manager_section_without_touching_the_gpu():
    blob = bh.managed_blob(2, (-1, 128000, -1))
    off = bh.section_offset(blob)
    out = blob.copy()
    out[bh.OFF_BITRATE:bh.OFF_BITRATE + 4] = np.frombuffer(np.uint32(blob.size - 16).tobytes(), np.uint8)
    assert _create(out) == -131                                   # beyond total_bytes
    slew = blob.copy()
    slew[off + 80:off + 88] = np.frombuffer(np.float64(0.0).tobytes(), np.uint8)  # slew_damp = 0
    assert _create(slew) == -131
    vbr = ref.RefEncoder(2, 44100, 0.4).pack_setup()
    vbr[bh.OFF_BITRATE:bh.OFF_BITRATE + 4] = np.frombuffer(np.uint32(vbr.size - 96).tobytes(), np.uint8)
    assert _create(vbr) == -131                                   # a section on a setup without a manager


def test_feed_refuses_a_managed_blob_without_the_section():
    """A managed blob packed before the section existed must not be fed the VBR candidates: refused, with a reason,
    before any GPU is looked at."""
    import vorbis_amd
    blob = bh.managed_blob(2, (-1, 128000, -1))
    blob[bh.OFF_BITRATE:bh.OFF_BITRATE + 4] = 0
    with pytest.raises(vorbis_amd.VamdError) as e:
        vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=1, max_frames=4096)
    assert e.value.code == -130 and "bitrate manager" in str(e.value)
