"""CPU: the packet decoder's front half (vorbis_amd/csrc/k_unpack.h) compiled for one lane on the host -- tests/c/
unpack_host.cpp, a program of its own built with -fsanitize=address,undefined and run as a child process -- against the
one-lane emulation's own tensors and the reference decoder, bit for bit (floats as bit patterns).

1. single blocks, per setup and size class: the rows unpacked from a block's packet are the emulation's rows of that block,
   and synth_block over them is vb->pcm of vorbis_synthesis() on the same packet;
2. whole streams: plan from the packets' mode bits, unpack, synth, lap against the reference decoder's output;
3. malformed input: every packet of a stream cut at every byte length, seeded bit flips, random bytes -- a status or rows
   inside the bounds the synthesis walk relies on, under the sanitisers;
4. mutated streams and the end granule's edges (tests/decode_cases.py, the cases tests/test_decode_gpu.py runs on the GPU):
   what a mutated packet decodes to where libvorbis decodes it in full, and the last block's cut, against the reference."""
import numpy as np
import pytest

from oracle import ref
from tests import decode_cases, ref_host, synth_host, unpack_host
from tests.feed_cases import same_bits
from tests.signals import gated_noise, managed_streams
from tests.synth_host import RES_CLASS_STRIDE

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")


@pytest.fixture(scope="module")
def exe():
    return unpack_host.build()


@pytest.mark.parametrize("name", list(synth_host.SETUPS))
def test_single_blocks(exe, tmp_path, name):
    from tests.emul.emul import Emul
    enc = ref_host.encoder(name)
    blob = enc.pack_setup()
    em = Emul(blob)
    dec = ref_host.BlockDecoder(ref_host.encoder_headers(ref_host.encoder(name)))
    bs, ch = (enc.blocksize(0), enc.blocksize(1)), enc.channels
    rows, want, what = [], [], []
    for W in ((1, 0) if bs[0] != bs[1] else (0,)):
        for kind, pcm in synth_host.block_set(ch, bs[W], 7 + W).items():
            b = synth_host.emul_block(em, pcm, W)
            packet, _ = enc.real_block(pcm, W, W, W, 1 if W else 0)
            assert b["packet"] == packet, (kind, W)  # the packet unpacked below is the reference encoder's
            rows.append(b)
            want.append(dec.block(packet, W))
            what.append((kind, W))
    dec.close()
    got, geo = unpack_host.host_unpack_blocks(exe, tmp_path, blob, [(b["W"], b["packet"]) for b in rows], bs, ch)
    curves = 0
    for w, g, b, pcm in zip(what, got, rows, want):
        G = geo[b["W"]]
        assert g["status"] == 0, w
        assert np.array_equal(g["post_valid"], b["post_valid"]), w
        assert np.array_equal(g["res_count"], b["res_count"]), w
        for sm in range(G["submaps"]):
            slots, total = (int(v) for v in b["res_count"][2 * sm:2 * sm + 2])
            c0, e0 = sm * RES_CLASS_STRIDE, G["ent_base"][sm]
            assert np.array_equal(g["res_class"][c0:c0 + slots], b["res_class"][c0:c0 + slots]), (w, sm)
            assert np.array_equal(g["res_entries"][e0:e0 + total], b["res_entries"][e0:e0 + total]), (w, sm)
        for c in range(ch):
            n = G["look_n"][G["sub"][c]]
            if b["post_valid"][c] and n & (n - 1) == 0:
                assert np.array_equal(g["ilogmask"][c], b["ilogmask"][c]), (w, c)
                curves += 1
        assert same_bits(g["pcm"], pcm), (w, int((g["pcm"].view(np.uint32) != pcm.view(np.uint32)).sum()))
    # the set does what it is there for: floors were compared, a block without any floor, residues with entries
    assert curves and any(not b["post_valid"].any() for b in rows) and any(b["res_count"][1] > 0 for b in rows)


def _stream(name, frames, seed):
    enc = ref_host.encoder(name)
    recs = enc.encode_stream(gated_noise(enc.channels, enc.rate, frames, seed))
    headers = ref_host.encoder_headers(ref_host.encoder(name))
    return enc, headers, [r["packet"] for r in recs], [r["granulepos"] for r in recs], [r["W"] for r in recs]


@pytest.mark.parametrize("name,seconds", [("44k_stereo_q4", 1.5), ("44k_stereo_qm1", 1.0), ("44k_51_q3", 1.0), ("8k_mono_q3", 2.0)])
def test_streams(exe, tmp_path, name, seconds):
    ch, rate, _, _ = synth_host.SETUPS[name]
    frames = int(rate * seconds) + 13
    enc, headers, packets, granules, Ws = _stream(name, frames, 5)
    if enc.blocksize(0) != enc.blocksize(1):  # long/long, long/short, short/long, short/short
        assert synth_host.lap_cases(Ws) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    want = ref_host.reference_decode(headers + packets, granules)
    assert want.shape == (ch, frames)
    (status, got), = unpack_host.host_decode_streams(exe, tmp_path, enc.pack_setup(), [packets], [granules[-1]], ch)
    assert status == 0
    assert same_bits(got, want), (got.shape, want.shape)


def test_short_streams(exe, tmp_path):
    """the lengths of tests/test_feed.py::test_short_streams in one group, the one-frame stream included"""
    streams, ends, want = [], [], []
    for frames in synth_host.SHORT_LENGTHS:
        enc, headers, packets, granules, _ = _stream("44k_stereo_q4", frames, frames)
        streams.append(packets)
        ends.append(granules[-1])
        want.append(ref_host.reference_decode(headers + packets, granules))
        assert want[-1].shape == (2, frames)
    got = unpack_host.host_decode_streams(exe, tmp_path, enc.pack_setup(), streams, ends, 2)
    for frames, (status, pcm), w in zip(synth_host.SHORT_LENGTHS, got, want):
        assert status == 0 and same_bits(pcm, w), frames


def test_flagged_streams(exe, tmp_path):
    """what tests/test_decode_gpu.py asks of the GPU: a stream whose third packet is cut to 5 bytes, one with a flipped
    packet-type bit; their neighbours untouched"""
    enc, headers, packets, granules, _ = _stream("44k_stereo_q4", 20000, 3)
    assert len(packets) > 4 and len(packets[2]) > 5
    cut = packets[:2] + [packets[2][:5]] + packets[3:]
    typed = packets[:1] + [bytes([packets[1][0] ^ 1]) + packets[1][1:]] + packets[2:]
    want = ref_host.reference_decode(headers + packets, granules)
    got = unpack_host.host_decode_streams(exe, tmp_path, enc.pack_setup(), [packets, cut, typed, packets], [granules[-1]] * 4, 2)
    assert [s for s, _ in got] == [0, unpack_host.STATUS_TRUNCATED, unpack_host.STATUS_NOTAUDIO, 0]
    assert got[1][1].shape == (2, 0) and got[2][1].shape == (2, 0)
    assert same_bits(got[0][1], want) and same_bits(got[3][1], want)


def test_managed_streams(exe, tmp_path):
    """a bitrate-managed encoder's packets: the streams none of whose packets the manager cut decode as the reference
    decodes them; a cut packet is a truncated one, and at this rate on these inputs the reference cuts in at most half of
    the streams (the cap tests/test_decode_gpu.py holds the feed's own packets to)"""
    blob, headers, streams = managed_streams()
    got = unpack_host.host_decode_streams(exe, tmp_path, blob, [p for p, _ in streams], [g[-1] for _, g in streams], 2)
    flagged = [s for s, (st, _) in enumerate(got) if st]
    assert all(got[s][0] == unpack_host.STATUS_TRUNCATED for s in flagged) and 2 * len(flagged) <= len(streams), flagged
    for s, (packets, granules) in enumerate(streams):
        if s not in flagged:
            assert same_bits(got[s][1], ref_host.reference_decode(headers + packets, granules)), s


MUTATED_CASES = 96


@pytest.mark.parametrize("name", list(synth_host.SETUPS))
def test_mutated_streams(exe, tmp_path, name):
    """packets no encoder wrote (tests/decode_cases.py: one packet of a stream with a bit flipped or its tail replaced),
    each classified by the reference alone, and what the decoder makes of them held against the reference: a packet
    libvorbis decodes without reaching its end decodes to the same bits and is not flagged, a packet that is no audio packet
    is flagged as one, a packet libvorbis ran out of is flagged and nothing is compared.  The statuses seen over the eight
    setups: 0, STATUS_TRUNCATED, and STATUS_NOTAUDIO once (44k_stereo_q4); never STATUS_BADCODE -- the books are complete
    trees, the phrase books have exactly nparts^dim entries."""
    g = decode_cases.cases(name, MUTATED_CASES)
    decode_cases.check(g, unpack_host.host_decode_streams(exe, tmp_path, g.blob, g.streams, g.ends, g.channels))


def test_end_granules(exe, tmp_path):
    """the plan's cut of the last block against vorbis_synthesis_blockin's, at its edges (tests/decode_cases.py)"""
    g = decode_cases.end_granules()
    got = unpack_host.host_decode_streams(exe, tmp_path, g.blob, g.streams, g.ends, g.channels)
    decode_cases.check(g, got)
    assert tuple(pcm.shape[1] for _, pcm in got[:10]) == decode_cases.END_COUNTS_9000


@pytest.mark.parametrize("name", ["44k_stereo_q4", "44k_51_q3"])
def test_malformed(exe, tmp_path, name):
    enc, _, packets, _, Ws = _stream(name, 7777, 9)
    assert 0 in Ws or 1 in Ws
    line = unpack_host.host_fuzz(exe, tmp_path, enc.pack_setup(), packets)
    cut, flagged, decoded, walked = (int(w) for w in line.replace(",", "").split() if w.isdigit())
    assert cut == sum(len(p) for p in packets) and flagged >= cut and walked > 0
    assert flagged + decoded == cut + 4000  # the fixed counts: 3000 flips, 1000 random packets
