"""The header-made decoder under hand-made setups (tests/setup_maker.py) and packets written for them
(tests/packet_writer.py), on the one-lane host builds (tests/c/decode_headers_host.cpp in `streams` mode for the default
policy, tests/c/unpack_partial_host.cpp with keep = 1 for the keep policy; both -fsanitize=address,undefined): first the
writer against the reference alone -- every written packet is one vorbis_synthesis decodes to its last bit and no further --,
then plan, unpack, synth and lap against libvorbis' decoder under the same headers, bit for bit."""
import subprocess

import numpy as np
import pytest

from oracle import ref
from tests import hostbuild, packet_writer, setup_maker, unpack_partial_host as partial
from tests.feed_cases import same_bits

pytestmark = pytest.mark.skipif(not ref.available(), reason="needs the reference build")

NAMES, get, host_decode = setup_maker.NAMES, setup_maker.get, setup_maker.host_decode
SEEDS = tuple(range(24))
EVERY = NAMES + tuple("seed%d" % s for s in SEEDS)
TWO_MODES = tuple(n for n in NAMES if n not in ("equal_64_one_mode", "one_mode_short"))


@pytest.fixture(scope="module")
def exe():
    return hostbuild.program("decode_headers_host.cpp")


@pytest.fixture(scope="module")
def keep_exe():
    return partial.build()


# ---- the maker and the writer ----
@pytest.mark.parametrize("name", EVERY)
def test_every_written_packet_is_the_references_to_its_last_bit(name):
    """vorbis_synthesis returns 0, oggpack_bits(&vb->opb) is the writer's length, decode_cases.classify says complete"""
    c = get(name)
    assert packet_writer.self_check(c) == sum(len(s) for s in c.streams)
    assert all(10 <= len(s) <= 14 for s in c.streams)
    assert len(c.headers[0]) == 30 and len(c.streams) == (4 if name in NAMES else 2)


@pytest.mark.parametrize("name", NAMES)
def test_the_written_choices_cover_the_modes_and_the_flag_pairs(name):
    c = get(name)
    modes, pairs = packet_writer.coverage(c)
    if name in TWO_MODES:
        assert modes == {0, 1} and pairs == {(0, 0), (0, 1), (1, 0), (1, 1)}, (modes, pairs)
        for s in range(len(c.streams)):  # and every stream steps from a long block to a short one and back
            assert {(1, 0), (0, 1)} <= set(zip(c.size_classes(s)[:-1], c.size_classes(s)[1:]))
    else:
        assert modes == {0} and len(c.M.S["modes"]) == 1


def test_book_shapes_writes_a_32_bit_codeword_and_entry_65534():
    c = get("book_shapes")
    deep = set().union(*(n["deep"] for row in c.notes for n in row))
    books = c.M.S["books"]
    assert any(books[b]["lengths"][e] == 32 for b, e in deep) and max(n["longest"] for row in c.notes for n in row) == 32
    assert (c.M.big, 65534) in deep and books[c.M.big]["entries"] == 65535
    assert any(b == c.M.comb_value for b, _ in deep)  # ... a residue book's, beside the floor's and the phrase book's


def test_the_cases_have_the_shapes_their_names_promise():
    S = get("eight_ch_max").M.S
    long_map = S["maps"][S["modes"][1][3]]
    assert [c for c, sm in enumerate(long_map["mux"]) if sm == 1] == [1, 4, 6] and len(long_map["coupling"]) == 4
    r0, r1 = (S["residues"][long_map["sub"][sm][2]] for sm in (0, 1))
    assert (r0["type"], r1["type"]) == (1, 2) and (2048 - r0["begin"]) // (r0["grouping"] + 1) * 5 == 510 and r1["end"] > 3 * 2048
    dirtied = [n["dirtied"] for row in get("eight_ch_max").notes for n in row]
    assert any(dirtied) and {1, 4, 6} & set().union(*dirtied) and {0, 2, 3, 5, 7} & set().union(*dirtied)  # in either submap
    assert max(len(f["x"]) for f in get("floor_shapes").M.S["floors"]) == 63
    mults = {f["mult"] + 1 for n in ("floor_shapes", "eight_ch_max") for f in get(n).M.S["floors"]}
    assert mults == {1, 2, 3, 4}
    assert [low | high << 3 for low, _, high in get("cascade_holes").M.S["residues"][0]["cascade"]] == [0b10100101, 1, 0]


def test_a_floor_of_65_posts_makes_an_image(exe, tmp_path):
    """the regression case of bind_params' post levels (derive_post_levels kept 64 where a floor may have VAMD_POSIT = 65
    posts: a write past the vector, which this sanitized build reports): the headers alone, through headers_to_image"""
    M = setup_maker.posts65()
    headers = M.headers()
    assert len(M.S["floors"][0]["x"]) + 2 == 65
    job, out = tmp_path / "codes.job", tmp_path / "codes.out"
    with open(job, "wb") as f:
        f.write(np.int32(1).tobytes())
        for p in (headers[0], headers[2]):
            f.write(np.int32(len(p)).tobytes() + bytes(p) + b"\0" * (-len(p) & 3))
    r = subprocess.run([exe, "codes", str(job), str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert list(np.fromfile(out, np.int32)) == [0], r.stdout


# ---- the default policy ----
@pytest.mark.parametrize("name", EVERY)
def test_streams_equal_the_reference(exe, tmp_path, name):
    c = get(name)
    got, lattice, table = host_decode(exe, tmp_path, c, c.streams)
    peak = 0.0
    for s, ((status, pcm), packets) in enumerate(zip(got, c.streams)):
        want = setup_maker.reference(c, packets)
        assert status == 0 and pcm.shape == want.shape, (name, s, status, pcm.shape, want.shape)
        assert same_bits(pcm, want), (name, s, int((pcm.view(np.uint32) != want.view(np.uint32)).sum()))
        peak = max(peak, float(np.abs(want).max()))
    assert peak > 0 and np.isfinite(peak)
    if name == "book_shapes":
        assert lattice > 0 and table > 0  # lattice books and value-list books side by side
    (lds0, lds1), (off0, off1) = host_decode.lds  # as the library's own synth_lds_words and bind_params give them
    n2 = [c.bs[W] // 2 for W in (0, 1)]
    assert (lds0, lds1) == tuple(setup_maker.synth_lds_bytes(c.channels, n2[W], (off0, off1)[W]) for W in (0, 1)), (name, host_decode.lds)
    if name == "eight_ch_max":
        # the largest demand the covered shape has: 8 spectra of 2048 floats and 8 butterfly vectors of 2176; the offsets row
        # of a long block is 8 stages x 510 slots + 1 (submap 0; submap 1: 3 x 512 + 1), of a short one 8 x 60 + 1
        assert (off0, off1) == (8 * 60 + 1, 8 * 510 + 1) and off1 == 4081
        assert lds1 == 135168 and lds1 < 160 * 1024  # (the LDS of a gfx950 workgroup; the GPU test asks the device)


# ---- the keep policy ----
@pytest.mark.parametrize("name", NAMES)
def test_cut_packets_are_kept_as_the_reference_keeps_them(keep_exe, tmp_path, name):
    c = get(name)
    streams = setup_maker.keep_streams(c)
    res = partial.host_streams(keep_exe, tmp_path, partial.setup_args(tmp_path, headers=c.headers), streams, [-1] * len(streams), c.channels, keep=1)
    for s, ((status, pcm), packets) in enumerate(zip(res, streams)):
        want = setup_maker.reference(c, packets)
        assert status == partial.STATUS_PARTIAL, (name, s, len(packets[1]), status)
        assert pcm.shape == want.shape and same_bits(pcm, want), (name, s, len(packets[1]), pcm.shape, want.shape)
