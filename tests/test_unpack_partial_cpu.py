"""CPU: the packet decoder under the keep policy (vamd_decode_partial) -- k_unpack.h's second instantiation of the walk and
k_synth.h's bounded residue add, compiled for one lane on the host (tests/c/unpack_partial_host.cpp, a program of its own
built with -fsanitize=address,undefined) -- against the reference decoder, bit for bit (floats as bit patterns).

Every audio packet for which libvorbis' vorbis_synthesis() returns 0 decodes to its vb->pcm and is flagged STATUS_PARTIAL
alone where it stopped being read early; every packet it refuses flags its stream as under the default policy.
1. every cut of every packet of two stereo streams, and thinned cuts of a 5.1 and a mono stream;
2. the places the reader first failed at over those cuts cover every kind of stop (a condition of the test);
3. whole streams with cut packets against reference_decode, clean neighbours untouched;
4. seeded bit flips and random packets;
5. a setup whose residue books are value lists (the k_synth_values path);
6. the default policy on test 3's inputs is what it was;
7. the stops that leave the reader alone -- a phrase word beyond the classes, a phrase book and a floor book without used
   entries -- under rewritten headers (decode_partial_cases.rewritten_headers), and the one stated limit: a residue value
   book without used entries still flags its packet."""
import numpy as np
import pytest

from oracle import ref
from tests import decode_partial_cases as cases
from tests import unpack_partial_host as host
from tests.feed_cases import same_bits
from tests.unpack_partial_host import AT_CLASSES, AT_ENTRY, AT_FLAG, AT_FLOORBOOK, AT_PHRASE, AT_POST, STATUS_PARTIAL, STATUS_TRUNCATED

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")


@pytest.fixture(scope="module")
def exe():
    return host.build()


def check_blocks(got, classes, what):
    """a packet the reference decodes is kept, with its vb->pcm; a packet it refuses is flagged and has no frames"""
    for g, (r, pcm), w in zip(got, classes, what):
        if r == 0:
            assert g["status"] & ~STATUS_PARTIAL == 0 and g["pcm"] is not None, (w, g["status"])
            assert g["pcm"].shape == pcm.shape, (w, g["pcm"].shape, pcm.shape)
            assert same_bits(g["pcm"], pcm), (w, g["place"], g["index"], g["stage"], int((g["pcm"].view(np.uint32) != pcm.view(np.uint32)).sum()))
        else:
            assert g["status"] & ~STATUS_PARTIAL and g["pcm"] is None, (w, g["status"])


def check_cuts(S_bs, got, default, classes, cases_, whole, ends):
    """what test 1 asks of cut packets: the status is exactly PARTIAL where the reference returns 0, else the default
    policy's; res_count[1] is what was read -- the entries of the WHOLE packet's walk whose last bit lies inside the cut
    (ends: unpack_partial_host.host_entry_ends of the whole packets; up to the first failed read a cut packet reads what
    the whole one reads, and behind it nothing)"""
    check_blocks(got, classes, cases_)
    for g, d, (r, _), c in zip(got, default, classes, cases_):
        key = c[:-2]  # (the packet the cut is of)
        if r == 0:
            assert g["status"] == STATUS_PARTIAL and g["place"], (c[:-1], g["status"], g["place"])
            assert d["status"] == STATUS_TRUNCATED and d["pcm"] is None, (c[:-1], d["status"])
            full = whole[key]["res_count"]
            for sm in range(2):
                slots, read = g["res_count"][2 * sm:2 * sm + 2]
                assert slots in (0, full[2 * sm]) and 0 <= read <= full[2 * sm + 1], (c[:-1], g["res_count"], full)
                assert read == int((ends[key][sm] <= 8 * len(c[-1])).sum()), (c[:-1], sm, g["res_count"])
        else:
            assert g["status"] == d["status"] and g["pcm"] is None and d["pcm"] is None, (c[:-1], g["status"], d["status"])


def places(got, classes):
    return {(g["place"], g["index"], g["stage"] > 0) for g, (r, _) in zip(got, classes) if r == 0}


def test_every_cut_of_two_stereo_streams(exe, tmp_path):
    S, cases_, classes = cases.stereo_cut_cases()
    setup = host.setup_args(tmp_path, blob=S.blob)
    cut = [c for _, _, _, c in cases_]
    got = host.host_blocks(exe, tmp_path, setup, cut, S.bs, S.channels, keep=1)
    default = host.host_blocks(exe, tmp_path, setup, cut, S.bs, S.channels, keep=0)
    streams = cases.stereo_streams()
    keys = [(s, k) for s, (packets, _) in enumerate(streams) for k in range(len(packets))]
    whole = dict(zip(keys, host.host_blocks(exe, tmp_path, setup, [streams[s][0][k] for s, k in keys], S.bs, S.channels, keep=1)))
    assert all(w["status"] == 0 and w["place"] == 0 for w in whole.values())  # an uncut packet is not partial
    ends = dict(zip(keys, host.host_entry_ends(exe, tmp_path, setup, [streams[s][0][k] for s, k in keys])))
    check_cuts(S.bs, got, default, classes, cases_, whole, ends)
    assert sum(r == 0 for r, _ in classes) > len(classes) * 0.9
    # coverage is a condition: the flag bit, a post's value bits, a floor book's codeword, a stage-0 phrase word, an entry
    # at stage 0 and one at a later stage
    seen = {(p, later) for p, _, later in places(got, classes)}
    for need in ((AT_FLAG, False), (AT_POST, False), (AT_FLOORBOOK, False), (AT_PHRASE, False), (AT_ENTRY, False), (AT_ENTRY, True)):
        assert need in seen, (need, sorted(seen))


@pytest.mark.parametrize("name", ["44k_51_q3", "44k_mono_q5"])
def test_thinned_cuts_of_a_surround_and_a_mono_stream(exe, tmp_path, name):
    """44k_51_q3: two submaps, coupling deeper than one step, the LFE floor of two posts; long packets thinned by
    decode_partial_cases.thinned"""
    S = cases.setup(name)
    packets, _ = cases.stream_of(name)
    assert S.bs[0] == S.bs[1] or {(p[0] >> 1) & 1 for p in packets} == {0, 1}
    cases_ = [(0,) + c for c in cases.cuts(packets, cases.thinned)]
    cut = [c[-1] for c in cases_]
    classes = cases.classify(S.headers, cut)
    setup = host.setup_args(tmp_path, blob=S.blob)
    got = host.host_blocks(exe, tmp_path, setup, cut, S.bs, S.channels, keep=1)
    default = host.host_blocks(exe, tmp_path, setup, cut, S.bs, S.channels, keep=0)
    whole = {(0, k): w for k, w in enumerate(host.host_blocks(exe, tmp_path, setup, packets, S.bs, S.channels, keep=1))}
    assert all(w["status"] == 0 for w in whole.values())
    ends = {(0, k): e for k, e in enumerate(host.host_entry_ends(exe, tmp_path, setup, packets))}
    check_cuts(S.bs, got, default, classes, cases_, whole, ends)
    if name == "44k_51_q3":
        kept = [g for g, (r, _) in zip(got, classes) if r == 0]
        # a stop in submap 0 behind which submap 1 reads nothing, and a stop in submap 1
        assert any(g["place"] in (AT_PHRASE, AT_ENTRY) and g["index"] == 0 and g["res_count"][2] > 0 and g["res_count"][3] == 0 for g in kept)
        assert any(g["place"] in (AT_PHRASE, AT_ENTRY) and g["index"] == 1 for g in kept)
        # the LFE floor's end posts (channel 5, two posts and no codeword: libvorbis reads them unchecked)
        assert any(g["place"] == AT_POST and g["index"] == 5 for g in kept)


def check_streams(got, want, damaged):
    for s, ((status, pcm), w, d) in enumerate(zip(got, want, damaged)):
        assert status == (STATUS_PARTIAL if d else 0), (s, status)
        assert pcm.shape == w.shape and same_bits(pcm, w), (s, pcm.shape, w.shape)


def test_streams_with_cut_packets(exe, tmp_path):
    """a cut packet in first, middle and last place and two in one stream: the whole stream is reference_decode's of the same
    packets, the last block's end-granule cut included; the clean streams between them are what they are alone"""
    S, streams, ends, damaged, want = cases.damaged_streams()
    setup = host.setup_args(tmp_path, blob=S.blob)
    got = host.host_streams(exe, tmp_path, setup, streams, ends, S.channels, keep=1)
    check_streams(got, want, damaged)
    clean = [s for s, d in enumerate(damaged) if not d]
    alone = host.host_streams(exe, tmp_path, setup, [streams[s] for s in clean], [ends[s] for s in clean], S.channels, keep=1)
    for s, (status, pcm) in zip(clean, alone):
        assert status == 0 and same_bits(pcm, got[s][1]), s


def test_default_policy_is_untouched(exe, tmp_path):
    """with the setting off the same inputs give what they gave: STATUS_TRUNCATED and no frames; the clean streams decode"""
    S, streams, ends, damaged, want = cases.damaged_streams()
    got = host.host_streams(exe, tmp_path, host.setup_args(tmp_path, blob=S.blob), streams, ends, S.channels, keep=0)
    for s, ((status, pcm), w, d) in enumerate(zip(got, want, damaged)):
        if d:
            assert status == STATUS_TRUNCATED and pcm.shape == (S.channels, 0), (s, status, pcm.shape)
        else:
            assert status == 0 and same_bits(pcm, w), s


@pytest.mark.parametrize("name,flips,randoms", [("44k_stereo_q4", 500, 200), ("44k_51_q3", 150, 60)])
def test_mutations(exe, tmp_path, name, flips, randoms):
    """seeded bit flips and random packets: every case for which the reference returns 0 is compared in full, every other
    is flagged with no frames.  (The phrase books of these genuine setups have exactly classes^dim entries: the stops that
    leave the reader alone are test_stops_that_leave_the_reader_alone's, under rewritten headers.)"""
    S, packets, classes = cases.mutations(name, flips, randoms)
    got = host.host_blocks(exe, tmp_path, host.setup_args(tmp_path, blob=S.blob), packets, S.bs, S.channels, keep=1)
    check_blocks(got, classes, range(len(packets)))
    kept = sum(r == 0 for r, _ in classes)
    assert kept > len(packets) // 2 and kept < len(packets)
    assert any(g["status"] == STATUS_PARTIAL for g in got) and any(g["status"] == 0 for g in got)


@pytest.mark.parametrize("name,kind", [("44k_stereo_q4", "spare_phrase"), ("44k_51_q3", "spare_phrase"), ("44k_stereo_q4", "empty_phrase"),
                                       ("44k_stereo_q4", "empty_floor")])
def test_stops_that_leave_the_reader_alone(exe, tmp_path, name, kind):
    """rewritten headers (decode_partial_cases.rewritten_headers) under genuine and bit-flipped packets: a phrase word beyond
    the classes, a phrase book and a floor book without used entries.  libvorbis stops the submap, or drops the floor,
    with the reader where it stands: the next submap (5.1) or the next channel reads real bits from there."""
    hv, bs, ch, packets, classes = cases.rewritten_cases(name, kind)
    got = host.host_blocks(exe, tmp_path, host.setup_args(tmp_path, headers=hv), packets, bs, ch, keep=1)
    check_blocks(got, classes, range(len(packets)))
    assert sum(r == 0 for r, _ in classes) >= len(packets) - 2
    place = {"spare_phrase": AT_CLASSES, "empty_phrase": AT_PHRASE, "empty_floor": AT_FLOORBOOK}[kind]
    hit = [g for g in got if g["place"] == place and g["status"] == STATUS_PARTIAL]
    assert len(hit) >= 10, (kind, len(hit))
    if name == "44k_51_q3":  # the stop is in submap 0, and submap 1 went on to read its own residue from where the reader stood
        assert any(g["index"] == 0 and g["res_count"][2] > 0 and g["res_count"][3] > 0 for g in hit)
    default = host.host_blocks(exe, tmp_path, host.setup_args(tmp_path, headers=hv), packets, bs, ch, keep=0)
    assert all(d["status"] & ~STATUS_PARTIAL and d["pcm"] is None for d, g in zip(default, got) if g["status"] == STATUS_PARTIAL)


def test_a_value_book_without_used_entries_still_flags(exe, tmp_path):
    """the stated limit of header-made setups: libvorbis adds nothing for such a book and reads on; here the packet is
    flagged STATUS_BADCODE under either policy (never decoded to something else), and every other packet is the reference's"""
    hv, bs, ch, packets, classes = cases.rewritten_cases("44k_stereo_q4", "empty_value")
    got = host.host_blocks(exe, tmp_path, host.setup_args(tmp_path, headers=hv), packets, bs, ch, keep=1)
    flagged = 0
    for k, (g, (r, pcm)) in enumerate(zip(got, classes)):
        if g["status"] == host.STATUS_BADCODE:
            assert g["pcm"] is None, k
            flagged += 1
        elif r == 0:
            assert g["status"] & ~STATUS_PARTIAL == 0 and same_bits(g["pcm"], pcm), (k, g["status"])
        else:
            assert g["status"] & ~STATUS_PARTIAL and g["pcm"] is None, (k, g["status"])
    assert flagged >= 10 and flagged < len(packets)


def test_a_value_list_setup(exe, tmp_path):
    hv, bs, cases_, classes = cases.value_list_cases()
    got = host.host_blocks(exe, tmp_path, host.setup_args(tmp_path, headers=hv), [c for _, _, c in cases_], bs, 2, keep=1)
    check_blocks(got, classes, [c[:2] for c in cases_])
    for g, (r, _), c in zip(got, classes, cases_):
        assert g["status"] == (STATUS_PARTIAL if r == 0 else STATUS_TRUNCATED), (c[:2], g["status"])
    assert any(g["place"] == AT_ENTRY and g["stage"] > 0 for g in got)
