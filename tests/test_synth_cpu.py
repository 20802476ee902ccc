"""CPU: the decoder's back half (vorbis_amd/csrc/k_synth.h) compiled for one lane on the host -- tests/c/synth_host.cpp, a
program of its own built with -fsanitize=address,undefined -- against the reference decoder, bit for bit (floats are
compared as bit patterns: signed zeros count).

1. single blocks, per setup and size class: synth_block over the one-lane emulation's posts / classes / entries of a
   block against vb->pcm of vorbis_synthesis() on the reference encoder's packet for that block;
2. mdct_backward alone, every size 256 ... 4096;
3. the lap: lap_find / lap_sample over the reference decoder's own vb->pcm of a stream's packets against
   vorbis_synthesis_blockin / _pcmout of the same packets."""
import numpy as np
import pytest

from oracle import ref
from tests import ref_host, synth_host
from tests.feed_cases import same_bits
from tests.signals import gated_noise

pytestmark = pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built (needs /root/reference)")


@pytest.fixture(scope="module")
def exe():
    return synth_host.build()


@pytest.mark.parametrize("n", [256, 512, 1024, 2048, 4096])
def test_mdct_backward(exe, tmp_path, n):
    rng = np.random.default_rng(n)
    spectra = [(rng.standard_normal(n // 2) * 10.0 ** rng.uniform(-6, 3, n // 2)).astype(np.float32),
               ((rng.random(n // 2) - 0.5) * 200).astype(np.float32).round(),
               np.zeros(n // 2, np.float32)]  # (all zero: the arithmetic still runs, -0*T - 0*T is -0)
    spectra.append(spectra[0] * (rng.random(n // 2) < 0.1))
    spectra.append(np.full(n // 2, 1e-41, np.float32))  # fp32 subnormals are kept
    for k, x in enumerate(spectra):
        want, trig = ref_host.reference_mdct_backward(n, x)
        got = synth_host.host_mdct_backward(exe, tmp_path, n, trig, x)
        assert same_bits(got, want), "n=%d spectrum %d: %d of %d values differ" % (n, k, int((got.view(np.uint32) != want.view(np.uint32)).sum()), n)
    assert np.signbit(want).any()  # (the last one asked for signed zeros / subnormals; the zero spectrum gives -0)


@pytest.mark.parametrize("name", list(synth_host.SETUPS))
def test_single_blocks(exe, tmp_path, name):
    from tests.emul.emul import Emul
    enc = ref_host.encoder(name)
    blob = enc.pack_setup()
    em = Emul(blob)
    dec = ref_host.BlockDecoder(ref_host.encoder_headers(ref_host.encoder(name)))
    bs = (enc.blocksize(0), enc.blocksize(1))
    assert dec.bs == bs and dec.channels == enc.channels
    blocks, want, what = [], [], []
    for W in ((1, 0) if bs[0] != bs[1] else (0,)):
        for kind, pcm in synth_host.block_set(enc.channels, bs[W], 7 + W).items():
            b = synth_host.emul_block(em, pcm, W)
            packet, _ = enc.real_block(pcm, W, W, W, 1 if W else 0)
            assert b["packet"] == packet, (kind, W)  # the entries below are those of the packet the reference decodes
            blocks.append(b)
            want.append(dec.block(packet, W))
            what.append((kind, W))
    dec.close()
    got = synth_host.host_synth_blocks(exe, tmp_path, blob, blocks, bs, enc.channels)
    bad = [(w, int((g.view(np.uint32) != r.view(np.uint32)).sum())) for w, g, r in zip(what, got, want) if not same_bits(g, r)]
    assert not bad, bad
    # the set does what it is there for: a block without any floor, one whose floors differ between channels, and signal
    assert any(not b["post_valid"].any() for b in blocks) and any(np.abs(w).max() > 0.1 for w in want)
    if enc.channels > 1:
        assert any(b["post_valid"].any() and not b["post_valid"].all() for b in blocks)


def _stream(name, frames, seed):
    """-> (blocks [(W, vb->pcm)], headers, packets, granules) of the reference encoder over gated noise"""
    enc = ref_host.encoder(name)
    x = gated_noise(enc.channels, enc.rate, frames, seed)
    recs = enc.encode_stream(x)
    headers = ref_host.encoder_headers(ref_host.encoder(name))
    dec = ref_host.BlockDecoder(headers)
    blocks = [(r["W"], dec.block(r["packet"], r["W"])) for r in recs]
    dec.close()
    return blocks, headers, [r["packet"] for r in recs], [r["granulepos"] for r in recs]


@pytest.mark.parametrize("name,seconds", [("44k_stereo_q4", 1.5), ("44k_stereo_qm1", 1.0), ("44k_51_q3", 1.0), ("8k_mono_q3", 2.0)])
def test_lap(exe, tmp_path, name, seconds):
    ch, rate, _, _ = synth_host.SETUPS[name]
    frames = int(rate * seconds) + 13
    blocks, headers, packets, granules = _stream(name, frames, 5)
    enc = ref_host.encoder(name)
    bs = (enc.blocksize(0), enc.blocksize(1))
    if bs[0] != bs[1]:  # long/long, long/short, short/long, short/short
        assert synth_host.lap_cases([W for W, _ in blocks]) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    want = ref_host.reference_decode(headers + packets, granules)
    assert want.shape == (ch, frames)
    got = synth_host.host_lap(exe, tmp_path, bs, synth_host.windows(enc.pack_setup(), bs), blocks, frames)
    assert same_bits(got, want), int((got.view(np.uint32) != want.view(np.uint32)).sum())


@pytest.mark.parametrize("frames", synth_host.SHORT_LENGTHS)
def test_lap_short_streams(exe, tmp_path, frames):
    blocks, headers, packets, granules = _stream("44k_stereo_q4", frames, frames)
    enc = ref_host.encoder("44k_stereo_q4")
    bs = (enc.blocksize(0), enc.blocksize(1))
    want = ref_host.reference_decode(headers + packets, granules)
    assert want.shape == (2, frames)
    got = synth_host.host_lap(exe, tmp_path, bs, synth_host.windows(enc.pack_setup(), bs), blocks, frames)
    assert same_bits(got, want)
