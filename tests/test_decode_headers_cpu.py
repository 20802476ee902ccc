"""The header-made decoder on the host (vorbis_amd/csrc/vamd_headers.h through tests/c/decode_headers_host.cpp, built with
-fsanitize=address,undefined): the image made from a stream's own headers against the reference packer's blob, the derived
windows against the reference's tables, whole streams under genuine and rewritten headers (tests/setup_header_cases.py)
against the reference decoder bit for bit -- the table form of the residue add among them --, the parser's return codes
against vorbis_synthesis_headerin's over cut and bit-flipped headers, and the Ogg header reader."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import ref
from tests import checker, decode_cases, hostbuild, ogg_demux_cases, ref_host, setup_header_cases as shc
from tests.feed_cases import same_bits
from tests.unpack_host import _streams_job

pytestmark = pytest.mark.skipif(not ref.available(), reason="needs the reference build")

OK, EIMPL, ENOTVORBIS, EBADHEADER, EVERSION = 0, -130, -132, -133, -134
EXTRA, encoder = shc.EXTRA, shc.encoder
SETUPS = tuple(checker.ENCODERS) + tuple(EXTRA)
STREAM_SETUPS = ("44k_stereo_q4", "44k_mono_q5", "44k_51_q3", "44k_stereo_q4_uncoupled")
_cache = {}


def setup(name):
    """-> (headers, blob) of a setup"""
    if name not in _cache:
        _cache[name] = ([bytes(h) for h in ref_host.encoder_headers(encoder(name))], np.ascontiguousarray(encoder(name).pack_setup(), np.uint8))
    return _cache[name]


@pytest.fixture(scope="module")
def exe():
    return hostbuild.program("decode_headers_host.cpp")


def _file(tmp, name, data):
    path = os.path.join(str(tmp), name)
    with open(path, "wb") as f:
        f.write(bytes(data))
    return path


def _run(exe, args):
    # (the parser's and the decoder's time is bounded: the longest of these runs takes 10 s here)
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-4000:]
    return r.stdout


# ---- the image ----
@pytest.mark.parametrize("name", SETUPS)
def test_image_equals_the_packers_blob(exe, tmp_path, name):
    """every decode-side field -- trig, bit-reverse and window tables byte for byte, floors, residues, book lengths and
    codes, modes and coupling -- and every residue book recognised as a lattice book"""
    headers, blob = setup(name)
    out = hostbuild.run_ok(exe, ["image", _file(tmp_path, "id", headers[0]), _file(tmp_path, "setup", headers[2]), _file(tmp_path, "blob", blob.tobytes())])
    assert "differs" not in out, out


def test_windows_64_to_4096(exe, tmp_path):
    """the derived window (the formula's "%.10f" text read as a float, C's sin) equals the reference's table for every
    size: through _vorbis_window_get where the oracle library exports it (all of 64 .. 4096, 8192 too); the sizes the
    encoders reach (256, 512, 1024, 2048, 4096) are also held to the blobs' copies in the image test above"""
    L = C.CDLL(ref.LIB_PATH)
    assert hasattr(L, "_vorbis_window_get"), "the oracle library does not export _vorbis_window_get: 64 and 128 would go unchecked"
    L._vorbis_window_get.restype, L._vorbis_window_get.argtypes = C.POINTER(C.c_float), [C.c_int]
    for k, n in enumerate((64, 128, 256, 512, 1024, 2048, 4096, 8192)):
        out = os.path.join(str(tmp_path), "w%d" % n)
        _run(exe, ["window", str(n), out])
        got, want = np.fromfile(out, np.float32), np.ctypeslib.as_array(L._vorbis_window_get(k), (n // 2,))
        assert got.size == n // 2 and same_bits(got, want), (n, int((got.view(np.uint32) != want.view(np.uint32)).sum()))


# ---- the helper itself ----
@pytest.mark.parametrize("name", STREAM_SETUPS)
def test_helper_re_emits_a_header_as_it_is(name):
    headers, _ = setup(name)
    assert shc.variant(headers, "identity")[2] == headers[2]
    assert shc.variant(headers, "cover")[2] != headers[2]


def test_the_setups_hold_every_length_encoding():
    shc.assert_encodings([setup(name)[0] for name in STREAM_SETUPS])


# ---- whole streams on the one-lane build ----
def host_decode(exe, tmp, headers, streams, ends, ch):
    out = os.path.join(str(tmp), "streams.out")
    text = _run(exe, ["streams", _file(tmp, "id", headers[0]), _file(tmp, "setup", headers[2]), _streams_job(tmp, streams, ends), out])
    raw, at, res = np.fromfile(out, np.int32), 0, []
    for _ in streams:
        status, frames = int(raw[at]), int(raw[at + 1])
        res.append((status, raw[at + 2:at + 2 + ch * frames].view(np.float32).reshape(ch, frames)))
        at += 2 + ch * frames
    assert at == raw.size
    lattice, table = (int(v) for v in text.split()[1:3])
    return res, lattice, table


def reference(headers, packets, end):
    key = ("ref", headers[2], tuple(packets), end)
    if key not in _cache:
        w = ref_host.reference_decode(list(headers) + list(packets), [-1] * (len(packets) - 1) + [end])
        w.setflags(write=False)
        _cache[key] = w
    return _cache[key]


@pytest.mark.parametrize("kind", shc.VARIANTS)
@pytest.mark.parametrize("name", STREAM_SETUPS)
def test_streams_under_rewritten_headers(exe, tmp_path, name, kind):
    """plan, unpack, synth (the value path where a book has a value list), lap: bit for bit the reference under the same
    headers; identity, cover and explicit also the original's PCM"""
    _, headers, bs, base = decode_cases.base_streams(name, 1)
    hv = shc.variant(headers, kind)
    ch = headers[0][11]
    got, lattice, table = host_decode(exe, tmp_path, hv, [p for p, _ in base], [e for _, e in base], ch)
    assert (table > 0) == (kind in ("explicit", "scaled", "sequence", "permuted")), (kind, lattice, table)
    for (status, pcm), (packets, end) in zip(got, base):
        want = reference(hv, packets, end)
        assert status == 0 and pcm.shape == want.shape and same_bits(pcm, want), (name, kind, status, pcm.shape, want.shape)
        if kind in ("identity", "cover", "explicit"):
            assert same_bits(pcm, reference(headers, packets, end))
        else:
            assert not same_bits(pcm, reference(headers, packets, end)), "the variant changes no value"


def test_block_sizes_64_and_128_and_a_single_entry_book(exe, tmp_path):
    """a hand-made setup (setup_header_cases.small_blocks) under packets of random bits, each of which the reference
    decodes without meeting its end: the transforms of 64 and 128 samples, floors of range 32 and 64, posts read through a
    book of one entry from bits of either value"""
    headers = setup("44k_stereo_q4")[0]
    hv, streams = shc.small_blocks(headers)
    dec = ref_host.BlockDecoder(hv)
    assert dec.bs == (64, 128)
    classes = {decode_cases.classify(dec, p) for packets in streams for p in packets}
    dec.close()
    assert classes == {"complete"}, classes
    assert {(p[0] >> 1) & 1 for packets in streams for p in packets} == {0, 1}
    got, lattice, table = host_decode(exe, tmp_path, hv, streams, [-1] * len(streams), 2)
    for (status, pcm), packets in zip(got, streams):
        want = reference(hv, packets, -1)
        assert status == 0 and pcm.shape == want.shape and pcm.shape[1] > 300 and same_bits(pcm, want), (status, pcm.shape, want.shape)
        assert np.abs(want).max() > 0


# ---- return codes ----
def reference_codes(ident, setup_packet, comment):
    codes, vi, vc = ref_host._headerin(ref_host._reflib(), [ident, comment, setup_packet])
    L = ref_host._reflib()
    L.vorbis_comment_clear(vc)
    L.vorbis_info_clear(vi)
    assert len(codes) != 2, "the comment header is refused"
    return codes[-1]


def run_codes(exe, tmp, cases):
    job, out = os.path.join(str(tmp), "codes.job"), os.path.join(str(tmp), "codes.out")
    with open(job, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for pair in cases:
            for p in pair:
                f.write(np.int32(len(p)).tobytes() + bytes(p) + b"\0" * (-len(p) & 3))
    text = _run(exe, ["codes", job, out])
    why = {int(line.split(" ", 1)[0]): line.split(" ", 1)[1] for line in text.splitlines() if line}
    return np.fromfile(out, np.int32), why


@pytest.mark.parametrize("name", SETUPS)
def test_return_codes_are_the_references(exe, tmp_path, name):
    """every header cut at every byte length, 2 000 seeded single-bit flips of the identification and setup headers: where
    vorbis_synthesis_headerin answers nonzero the parser answers the same code, where it answers zero the parser answers
    VAMD_OK or VAMD_EIMPL; never a sanitizer report"""
    (ident, comment, setup_packet), _ = setup(name)
    cases = [(ident[:n], setup_packet) for n in range(len(ident))] + [(ident, setup_packet[:n]) for n in range(len(setup_packet))]
    rng = np.random.default_rng(len(setup_packet))
    for k in range(2000):
        which = ident if k % 4 == 0 else setup_packet
        bit = int(rng.integers(0, 8 * len(which)))
        p = bytearray(which)
        p[bit >> 3] ^= 1 << (bit & 7)
        cases.append((bytes(p), setup_packet) if which is ident else (ident, bytes(p)))
    got, why = run_codes(exe, tmp_path, cases)
    assert got.size == len(cases)
    seen = set()
    for k, (a, b) in enumerate(cases):
        want = reference_codes(a, b, comment)
        seen.add((want, int(got[k])))
        if want:
            assert got[k] == want, (name, k, want, int(got[k]))
        else:
            assert got[k] in (OK, EIMPL), (name, k, int(got[k]), why.get(k))
    assert {w for w, _ in seen} >= {0, ENOTVORBIS, EBADHEADER, EVERSION}, seen  # the cases reach every class of answer


def test_shapes_outside_the_covered_one_are_refused_with_a_reason(exe, tmp_path):
    headers, _ = setup("44k_stereo_q4")
    cases = [shc.variant(headers, "modes3"), shc.variant(headers, "residue0"), shc.ident_8192(headers)]
    for h in cases:
        assert reference_codes(h[0], h[2], h[1]) == 0  # the reference takes all three
    got, why = run_codes(exe, tmp_path, [(h[0], h[2]) for h in cases])
    assert list(got) == [EIMPL] * 3, list(got)
    assert "3 modes" in why[0] and "residue type 0" in why[1] and "8192" in why[2], why


# ---- the Ogg header reader ----
def _python_headers(f):
    """an independent walk: the first three packets of the file's pages, or None where the file ends first"""
    pos, packets, cur = 0, [], b""
    while len(packets) < 3:
        if len(f) - pos < 27 or f[pos:pos + 4] != b"OggS":
            return None
        n = f[pos + 26]
        if len(f) - pos - 27 < n:
            return None
        lace = f[pos + 27:pos + 27 + n]
        at = pos + 27 + n
        if len(f) - at < sum(lace):
            return None
        for v in lace:
            cur += f[at:at + v]
            at += v
            if v < 255:
                packets.append(cur)
                cur = b""
                if len(packets) == 3:
                    break
        pos += 27 + n + sum(lace)
    return packets


def read_headers(exe, tmp, f):
    out = os.path.join(str(tmp), "ogg.out")
    _run(exe, ["ogg", _file(tmp, "file.ogg", f), out])
    raw = open(out, "rb").read()
    code, a, b, c = struct.unpack_from("<iqqq", raw, 0)
    body = raw[28:]
    assert len(body) == a + b + c
    return code, [body[:a], body[a:a + b], body[a + b:]]


@pytest.mark.parametrize("policy", ogg_demux_cases.POLICIES)
def test_ogg_read_headers(exe, tmp_path, policy):
    """headers across pages, the setup header and audio on one page, a comment header of many pages; and the file cut short"""
    _, headers, files = ogg_demux_cases.base_files("44k_stereo_q4", policy)
    f = bytes(files[0])
    code, got = read_headers(exe, tmp_path, f)
    want = _python_headers(f)
    assert code == 0 and got == want and got[0] == bytes(headers[0]) and got[2] == bytes(headers[2])
    rng = np.random.default_rng(5)
    end = f.find(got[2][-16:]) + 16  # a byte behind the setup header's last
    cuts = sorted({0, 1, 26, 27, 28, 57, 58, 59, end - 1, end, end + 1, len(f) - 1} | {int(v) for v in rng.integers(0, min(len(f), end + 300), 12)})
    for n in cuts:
        code, got = read_headers(exe, tmp_path, f[:n])
        want = _python_headers(f[:n])
        assert (code, got) == ((0, want) if want else (EBADHEADER, [b"", b"", b""])), (policy, n, code)
