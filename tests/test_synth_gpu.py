"""GPU: vamd_analyze_batch_synth (k_synth) over the block set of tests/test_synth_cpu.py -- every setup, both size classes --
against vb->pcm of the reference decoder's vorbis_synthesis() on the reference encoder's packet for the block, bit for bit;
and the call's ordinary outputs against vamd_analyze_batch's."""
import numpy as np
import pytest

from oracle import ref
from tests import ref_host, synth_host

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built (needs /root/reference)")]

WANT = ("mdct", "logmask", "posts", "post_valid", "iwork", "nonzero", "ampmax_out", "res_class", "res_entries", "res_count", "packets",
        "packet_bits")


@pytest.mark.parametrize("name", list(synth_host.SETUPS))
def test_blocks_against_the_reference_decoder(name):
    import torch
    import vorbis_amd
    enc = ref_host.encoder(name)
    an = vorbis_amd.Analyzer(enc.pack_setup(), 0)
    dec = ref_host.BlockDecoder(ref_host.encoder_headers(ref_host.encoder(name)))
    bs = (enc.blocksize(0), enc.blocksize(1))
    bad = []
    for W in ((1, 0) if bs[0] != bs[1] else (0,)):
        assert an.residue_capacity(W) > 0
        kinds = synth_host.block_set(enc.channels, bs[W], 7 + W)
        pcm = torch.from_numpy(np.stack(list(kinds.values()))).cuda()
        args = dict(W=W, lW=W, nW=W, blocktype=1 if W else 0)
        got = an.analyze(pcm, want=WANT + ("synth",), **args)
        plain = an.analyze(pcm, want=WANT, **args)
        torch.cuda.synchronize()
        for k in WANT:
            assert torch.equal(got[k], plain[k]), "%s differs from vamd_analyze_batch's (W=%d)" % (k, W)
        synth = got["synth"].cpu().numpy()
        for b, kind in enumerate(kinds):
            packet, _ = enc.real_block(kinds[kind], W, W, W, 1 if W else 0)
            assert vorbis_amd.packet_bytes(got["packets"][b].cpu().numpy(), int(got["packet_bits"][b])) == packet, (kind, W)
            want = dec.block(packet, W)
            diff = int((synth[b].view(np.uint32) != want.view(np.uint32)).sum())
            if diff:
                bad.append((kind, W, diff))
    dec.close()
    assert not bad, bad


def test_synth_without_any_other_output():
    """synth alone: the residue search runs although nobody takes its outputs"""
    import torch
    import vorbis_amd
    enc = ref_host.encoder("44k_stereo_q4")
    an = vorbis_amd.Analyzer(enc.pack_setup(), 0)
    dec = ref_host.BlockDecoder(ref_host.encoder_headers(ref_host.encoder("44k_stereo_q4")))
    kinds = synth_host.block_set(2, enc.blocksize(1), 8)
    pcm = torch.from_numpy(np.stack(list(kinds.values()))).cuda()
    synth = an.analyze(pcm, W=1, want=("synth",))["synth"].cpu().numpy()
    for b, kind in enumerate(kinds):
        want = dec.block(enc.real_block(kinds[kind], 1, 1, 1, 1)[0], 1)
        assert np.array_equal(synth[b].view(np.uint32), want.view(np.uint32)), kind
    dec.close()
