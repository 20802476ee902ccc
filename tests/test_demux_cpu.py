"""CPU: the Ogg decode entry's way from files to packets -- the shipped scan (vorbis_amd/csrc/vamd_demux.h) and
k_ogg_depage's body (k_demux.h) compiled for the host, tests/c/demux_host.cpp, a program of its own built with
-fsanitize=address,undefined and run as a child process -- against tests/ogg_framing.py's reader (the container) and the
reference decoder (the signal), neither of which comes from the code under test.

1. the packet table: every cut policy of tests/ogg_demux_cases.py x every feed setup -- the packed arena and the packet
   table are the independent reader's audio packets byte for byte, the end granule is its, the status 0;
2. the whole decode: those packets on through the existing host decode path (tests/unpack_host.py: plan, unpack_packet,
   synth, lap), against the reference decoder, bit for bit;
3. damaged files: the status bit the contract gives each kind, and their clean neighbours as without them;
4. seeded mutations of small files, each file also alone in a buffer of exactly its length: no sanitizer report, and clean
   exactly where a non-asserting reader reads the file whole."""
import numpy as np
import pytest

from oracle import ref
from tests import decode_cases, demux_host, ogg_demux_cases as cases, synth_host, unpack_host
from tests.feed_cases import same_bits

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")
CONTAINER = cases.STATUS_BADPAGE | cases.STATUS_BADHEADER


@pytest.fixture(scope="module")
def exe():
    return demux_host.build()


@pytest.fixture(scope="module")
def unpack_exe():
    return unpack_host.build()


def check_table(got, f):
    packets, end, _ = cases.expected(f, decode=False)
    assert got["status"] == 0 and got["end"] == end, (got["status"], got["end"], end)
    assert got["packets"] == packets, (len(got["packets"]), len(packets))


@pytest.mark.parametrize("name", synth_host.FEED_SETUPS)
def test_packet_table(exe, tmp_path, name):
    """all six policies of a setup's four base streams in one group, as the GPU test has them: 24 files back to back"""
    files = []
    for policy in cases.POLICIES:
        blob, headers, four = cases.base_files(name, policy)
        files += four
    got = demux_host.host_scan(exe, tmp_path, blob, files)
    for g, f in zip(got, files):
        check_table(g, f)
    # the policies do what they are there for: a packet across pages, a page that completes nothing, a page without a
    # segment, a maximal page, the setup header and audio packets on one page
    from tests import ogg_framing
    pages = [p for f in files for p in ogg_framing.demux(f)[0]]
    assert any(p["open"] for p in pages) and any(p["done"] == 0 and p["nseg"] for p in pages) and any(p["nseg"] == 0 for p in pages)
    assert any(p["body"] == 255 * 255 for p in pages)
    shared = ogg_framing.demux(cases.base_files(name, "shared")[2][0])[0]
    assert shared[2]["done"] == 4 and not shared[2]["flags"] & 1


def test_with_a_setup_header(exe, tmp_path):
    """the setup header given: the same result where it is the files'; every stream flagged where it is not"""
    blob, headers, files = cases.base_files("44k_stereo_q4", "seeded")
    for g, f in zip(demux_host.host_scan(exe, tmp_path, blob, files, headers[2]), files):
        check_table(g, f)
    other = headers[2][:-1] + bytes([headers[2][-1] ^ 1])
    for h in (other, headers[2] + b"\0", headers[2][:-1]):
        got = demux_host.host_scan(exe, tmp_path, blob, files, h)
        assert [g["status"] for g in got] == [cases.STATUS_BADHEADER] * 4 and not any(g["packets"] or g["frames"] for g in got)


def decode(exe, unpack_exe, tmp_path, blob, ch, files, setup_header=None):
    """scan + depage, then the existing host decode path over the packets they give -> [(status, pcm)]; the frames of the
    plan made from the scan's first bytes are those of the plan made from the packets"""
    got = demux_host.host_scan(exe, tmp_path, blob, files, setup_header)
    pcm = unpack_host.host_decode_streams(unpack_exe, tmp_path, blob, [g["packets"] for g in got], [g["end"] for g in got], ch)
    out = []
    for g, (st, x) in zip(got, pcm):
        assert g["status"] or st or g["frames"] == x.shape[1]
        out.append((g["status"] | st, x if not g["status"] else x[:, :0]))
    return out


@pytest.mark.parametrize("policies", [("seeded", "big_comment"), ("feed", "shared")])
def test_full_decode(exe, unpack_exe, tmp_path, policies):
    name = "44k_stereo_q4"
    files = [f for p in policies for f in cases.base_files(name, p)[2]]
    blob = cases.base_files(name, policies[0])[0]
    for (status, pcm), f in zip(decode(exe, unpack_exe, tmp_path, blob, 2, files), files):
        want = cases.expected(f)[2]
        assert status == 0 and same_bits(pcm, want), (status, pcm.shape, want.shape)


def test_short_streams(exe, unpack_exe, tmp_path):
    """one-frame streams, streams of two packets, end granules that cut the last block"""
    g = decode_cases.short_streams(8)
    for policy in ("one_packet", "full_255"):
        files = cases.group_files(g, policy)
        got = decode(exe, unpack_exe, tmp_path, g.blob, g.channels, files)
        assert [pcm.shape[1] for _, pcm in got] == list(synth_host.SHORT_LENGTHS)
        for (status, pcm), f in zip(got, files):
            assert status == 0 and same_bits(pcm, cases.expected(f)[2])


@pytest.mark.parametrize("name", ["44k_stereo_q4", "44k_51_q3"])
def test_damage(exe, unpack_exe, tmp_path, name):
    d = cases.damaged(name)
    ch = synth_host.SETUPS[name][0]
    got = decode(exe, unpack_exe, tmp_path, d.blob, ch, d.files, d.setup_header)
    alone = {}
    for s, ((status, pcm), f) in enumerate(zip(got, d.files)):
        what = (name, s, d.kind[s], status)
        if d.bit[s]:
            assert status & d.bit[s] and pcm.shape == (ch, 0), what
            continue
        assert status == 0 and same_bits(pcm, cases.expected(f)[2]), what
        if d.kind[s] is None:  # a clean neighbour: byte for byte what the file gives in a group of its own
            if f not in alone:
                alone[f] = decode(exe, unpack_exe, tmp_path, d.blob, ch, [f], d.setup_header)[0]
            assert alone[f][0] == 0 and same_bits(pcm, alone[f][1]), what
    assert {k for k in d.kind if k} == set(cases.DAMAGE) and sum(b == cases.STATUS_BADHEADER for b in d.bit) == 3


FUZZ = 2400


def test_fuzz(exe, tmp_path):
    """scan + depage over seeded mutations of small files under the sanitisers (the program also scans each file alone in
    a buffer of exactly its length, and holds the result against the group's); each file comes out clean exactly where
    the non-asserting reader reads it whole"""
    g = decode_cases.short_streams(4)
    files = cases.group_files(g, "one_packet") + cases.group_files(g, "seeded")
    ch, rate = synth_host.SETUPS[g.name][:2]
    from tests import ref_host
    enc = ref_host.encoder(g.name)
    bs = (enc.blocksize(0), enc.blocksize(1))
    assert all(cases.reads_whole(f, ch, rate, bs) for f in files)
    mutated = cases.mutations(files, FUZZ)
    got = demux_host.host_scan(exe, tmp_path, g.blob, mutated)
    clean = 0
    for i, (r, f) in enumerate(zip(got, mutated)):
        whole = cases.reads_whole(f, ch, rate, bs)
        assert (r["status"] & CONTAINER == 0) == whole, (i, i % 6, r["status"], whole, len(f))
        clean += whole
    assert FUZZ // 20 <= clean <= FUZZ - FUZZ // 4, clean  # both verdicts are well represented
