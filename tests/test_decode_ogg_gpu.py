"""GPU: the Ogg decode entry (vamd_decode_ogg_plan / vamd_decode_ogg; Analyzer.decode_ogg) -- whole Ogg Vorbis files in
host memory to PCM on the device: the page walk on the host, k_ogg_depage (checksums, unpaging) ahead of k_unpack, k_synth
and k_lap -- against what tests/ogg_framing.py reads back from the same files and libvorbis' decoder makes of it, bit for
bit.  The files are tests/ogg_demux_cases.py's (cut policies no encoder follows, damaged files) and an Ogg feed's own; the
same files have been through the same code on the host in tests/test_demux_cpu.py."""
import numpy as np
import pytest

from oracle import ref
from tests import decode_cases, ogg_demux_cases as cases, ogg_framing, ref_host, synth_host
from tests.feed_cases import Q4, same_bits
from tests.signals import gated_streams as streams

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")]
EINVAL = -131


def results(got, status):
    return [(int(status[s]), got[s].cpu().numpy()) for s in range(len(got))]


def decode(an, files, setup_header=None):
    got, status = an.decode_ogg(files, setup_header, with_status=True)
    assert len(got) == len(files) and all(t.is_cuda and t.device.index == an.device for t in got)
    return results(got, status)


def check_clean(got, files):
    for s, ((status, pcm), f) in enumerate(zip(got, files)):
        want = cases.expected(f)[2]
        assert status == 0 and same_bits(pcm, want), (s, status, pcm.shape, want.shape)


@pytest.mark.parametrize("name", synth_host.FEED_SETUPS)
def test_setups(name):
    """four base streams under the six policies, 24 files in one group"""
    import vorbis_amd
    files = [f for policy in cases.POLICIES for f in cases.base_files(name, policy)[2]]
    an = vorbis_amd.Analyzer(cases.base_files(name, "feed")[0])
    try:
        check_clean(decode(an, files), files)
    finally:
        an.close()


def test_short_streams():
    """one-frame streams, streams of two packets, end granules that cut the last block: 24 streams a policy"""
    import vorbis_amd
    g = decode_cases.short_streams(24)
    an = vorbis_amd.Analyzer(g.blob)
    try:
        for policy in ("one_packet", "full_255"):
            files = cases.group_files(g, policy)
            got = decode(an, files)
            assert [pcm.shape[1] for _, pcm in got[:8]] == list(synth_host.SHORT_LENGTHS)
            check_clean(got, files)
    finally:
        an.close()


@pytest.mark.parametrize("name", ["44k_stereo_q4", "44k_51_q3"])
def test_damage(name):
    """tests/test_demux_cpu.py::test_damage on the GPU: every kind carries its bit and yields a [ch, 0] tensor; the clean
    streams between them decode as they do in a group without damage"""
    import vorbis_amd
    d = cases.damaged(name)
    ch = synth_host.SETUPS[name][0]
    clean = [f for f, k, b in zip(d.files, d.kind, d.bit) if k is None]
    an = vorbis_amd.Analyzer(d.blob)
    try:
        got = decode(an, d.files, d.setup_header)
        alone = dict(zip(clean, decode(an, clean, d.setup_header)))
    finally:
        an.close()
    for s, ((status, pcm), f) in enumerate(zip(got, d.files)):
        what = (name, s, d.kind[s], status)
        if d.bit[s]:
            assert status & d.bit[s] and pcm.shape == (ch, 0), what
            continue
        assert status == 0 and same_bits(pcm, cases.expected(f)[2]), what
        if d.kind[s] is None:
            assert alone[f][0] == 0 and same_bits(pcm, alone[f][1]), what


def test_round_trip():
    """an Ogg feed's own files: decode_ogg gives what the reference decodes from the demuxed packets -- and what
    decode_streams gives on the feed's packets (a cross-check only)"""
    import vorbis_amd
    parts = streams(Q4, (0.9, 1.0, 1.1), 51)
    blob = ref_host.encoder(Q4).pack_setup()
    headers = ref_host.encoder_headers(ref_host.encoder(Q4))
    feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=3, max_frames=max(len(p) for p in parts), fmt=vorbis_amd.FEED_F32,
                           ogg_headers=headers)
    an = vorbis_amd.Analyzer(blob)
    try:
        files = feed.encode_ogg(parts)
        rows = feed.encode(parts)
        got = decode(an, files, headers[2])
        via_packets = an.decode_streams([[p for p, _, _, _ in row] for row in rows], [row[-1][1] for row in rows])
    finally:
        an.close()
        feed.close()
    assert all(len(ogg_framing.demux(f)[0]) > 5 for f in files)
    check_clean(got, files)
    for s, p in enumerate(parts):
        assert got[s][1].shape == (2, len(p)) and same_bits(got[s][1], via_packets[s].cpu().numpy()), s


def test_context_reuse():
    """a small group, a larger one, an empty one and one file on one context, a decode_streams call among them: the
    workspaces grow, and every group decodes as in a context of its own (the reference's bits)"""
    import vorbis_amd
    blob, headers, small = cases.base_files(Q4, "seeded")
    large = [f for policy in cases.POLICIES for f in cases.base_files(Q4, policy)[2]]
    packets = decode_cases.base_streams(Q4, 1)[3]
    an = vorbis_amd.Analyzer(blob)
    try:
        check_clean(decode(an, small[:2]), small[:2])
        check_clean(decode(an, large), large)
        via_packets = an.decode_streams([p for p, _ in packets], [end for _, end in packets])
        assert decode(an, []) == []
        check_clean(decode(an, small[3:]), small[3:])
        check_clean(decode(an, large), large)
        prep = an.decode_ogg_prepare(small)
        pcm, frames, off, status = an.decode_ogg_run(prep)
        assert not status.any() and [int(f) for f in frames] == [cases.expected(f)[2].shape[1] for f in small]
    finally:
        an.close()
    for s, f in enumerate(small):
        assert same_bits(via_packets[s].cpu().numpy(), cases.expected(f)[2]), s


def test_module_level_decode_ogg():
    import vorbis_amd
    blob, headers, files = cases.base_files(Q4, "one_packet")
    got = vorbis_amd.decode_ogg(blob, files[:1], setup_header=headers[2])
    assert same_bits(got[0].cpu().numpy(), cases.expected(files[0])[2])
    assert (vorbis_amd.STATUS_BADPAGE, vorbis_amd.STATUS_BADHEADER) == (cases.STATUS_BADPAGE, cases.STATUS_BADHEADER)


def test_bad_descriptors():
    """VAMD_EINVAL with a reason, nothing launched, and the context decodes the next group as before"""
    import ctypes as C
    import vorbis_amd
    blob, headers, files = cases.base_files(Q4, "seeded")
    sizes = np.cumsum([0] + [len(f) for f in files])
    an = vorbis_amd.Analyzer(blob)
    try:
        for off, why in ((sizes[[0, 2, 1, 3, 4]], "monotone"), (sizes - 1, "negative"), (sizes + (1 << 40), "2^40")):
            with pytest.raises(vorbis_amd.VamdError) as e:
                an.decode_ogg(files, file_offset=off)
            assert e.value.code == EINVAL and why in str(e.value), str(e.value)
        with pytest.raises(ValueError):
            an.decode_ogg([files[0], None])
        prep = an.decode_ogg_prepare(files)
        frames, status = np.zeros(4, np.int64), np.zeros(4, np.uint8)
        vp = C.c_void_p
        assert an.L.vamd_decode_ogg_plan(an.h, None, vp(frames.ctypes.data), None) == EINVAL
        assert an.L.vamd_decode_ogg(an.h, None, None, None, vp(status.ctypes.data)) == EINVAL
        d = prep["desc"]
        for field in ("file_offset", "bytes"):
            keep = getattr(d, field)
            setattr(d, field, None)
            assert an.L.vamd_decode_ogg_plan(an.h, C.byref(d), vp(frames.ctypes.data), None) == EINVAL
            assert an.L.vamd_decode_ogg(an.h, C.byref(d), None, None, vp(status.ctypes.data)) == EINVAL
            setattr(d, field, keep)
        d.setup_header_bytes = -1
        assert an.L.vamd_decode_ogg_plan(an.h, C.byref(d), vp(frames.ctypes.data), None) == EINVAL
        d.setup_header_bytes = 0
        assert an.L.vamd_decode_ogg(an.h, C.byref(d), None, None, vp(status.ctypes.data)) == EINVAL  # (frames to decode, nowhere to put them)
        check_clean(decode(an, files), files)
    finally:
        an.close()
