"""GPU: files as a reader takes them (vamd_decode_follow; Analyzer.follow_links) and packets with marks
(vamd_decode_streams_marked) -- the host's walk of links, foreign pages and page granules, then k_ogg_depage, k_unpack,
k_synth and k_lap_segments -- against libvorbis' decoder over what an independent reader makes of each file
(tests/decode_links_cases.py; tests/test_decode_links_cpu.py has taken every case through the one-lane host build), bit
for bit."""
import numpy as np
import pytest

from oracle import ref
from tests import decode_links_cases as cases
from tests.feed_cases import same_bits

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")]
BADPAGE, PARTIAL = cases.STATUS_BADPAGE, 128


def same(got, want):
    g = got.cpu().numpy()
    return g.shape == want.shape and same_bits(g, want)


def test_files_in_one_call():
    """the trim, shift and no-EOS files, a three-link file and a multiplexed file beside two plain files"""
    import vorbis_amd
    F, a, b = cases.files(), cases.stream(cases.STEREO, 0), cases.stream(cases.STEREO, 1)
    plain2 = b"".join(cases.logical(b, 0x111))
    names = ["trim_k3_below", "shift", "no_eos", "three_links", "foreign_interleaved", "trim_only_page_eos", "mid_high"]
    files = [F["plain"][0]] + [F[n][0] for n in names] + [plain2]
    an = vorbis_amd.Analyzer(a.blob)
    try:
        assert an.follow_links is False
        off, off_status = an.decode_ogg(files, a.headers[2], with_status=True)
        off = [p.clone() for p in off]
        an.follow_links = True
        assert an.follow_links is True
        on, on_status = an.decode_ogg(files, a.headers[2], with_status=True)
        on = [p.clone() for p in on]
        again = an.decode_ogg(files[:1], a.headers[2], follow_links=False)  # (per call, and the context's setting stands)
        assert an.follow_links is True and same(again[0], cases.expected(files[0])[0])
    finally:
        an.close()
    assert not on_status.any()
    for f, got, name in zip(files, on, ["plain"] + names + ["plain2"]):
        assert same(got, cases.expected(f)[0]), name
    for i in (0, len(files) - 1):  # the plain files: what the call without the policy gives
        assert off_status[i] == 0 and same(on[i], off[i].cpu().numpy())
    for name, st, got in zip(names, off_status[1:], off[1:]):
        if name in ("three_links", "foreign_interleaved"):  # as at the parent
            assert st == BADPAGE and got.shape[1] == 0, name
        else:
            assert st == 0, name
    # the wrong tail without the policy: the shifted file keeps the padding the reference drops
    assert off[2].shape[1] == sum(a.steps()) > on[2].shape[1] == a.end


def test_marks_through_the_packet_entry():
    """the files' marks as vamd_decode_marks; and without marks, vamd_decode_streams"""
    import vorbis_amd
    F, a, b = cases.files(), cases.stream(cases.STEREO, 0), cases.stream(cases.STEREO, 1)
    names = ["trim_k3_below", "trim_k1_equal", "shift", "no_eos", "trim_only_page_eos", "mid_low", "plain"]
    streams, grans, eoss = [], [], []
    for name in names:
        (_, _, _, pages), = cases.read_links(F[name][0])
        packets, gran, eos = cases.link_marks(pages)
        streams.append(packets[3:]), grans.append(gran), eoss.append(eos)
    an = vorbis_amd.Analyzer(a.blob)
    try:
        got, status = an.decode_streams(streams, with_status=True, packet_granules=grans, eos=eoss)
        got = [p.clone() for p in got]
        none, _ = an.decode_streams(streams, with_status=True, packet_granules=[[-1] * len(s) for s in streams])
        none = [p.clone() for p in none]
        plain = an.decode_streams(streams)
        for x, y in zip(none, plain):
            assert same(x, y.cpu().numpy())
        last, _ = an.decode_streams(streams[-1:], with_status=True, packet_granules=[a.granules])  # eos NULL: the last packet
        assert same(last[0], cases.expected(F["plain"][0])[0])
        with pytest.raises(vorbis_amd.VamdError):
            an.decode_streams(streams[:1], packet_granules=grans[:1], stream_start=[0, len(streams[0]) + 2])
    finally:
        an.close()
    assert not status.any()
    for name, g in zip(names, got):
        assert same(g, cases.expected(F[name][0])[0]), name


def _chain():
    """a chained file whose links have two setups and two channel counts, and one whose links have two stereo setups"""
    a, m = cases.stream(cases.STEREO, 0), cases.stream(cases.MONO, 3)
    q = cases.stream("44k_stereo_q9", 1)
    return (b"".join(cases.logical(a, 0x400) + cases.logical(m, 0x401) + cases.logical(a, 0x402, eos=False)),
            b"".join(cases.logical(a, 0x410) + cases.foreign(0x4ff, 2, bos=False)[:1] + cases.logical(q, 0x411)))


def test_decode_ogg_files_follows_links():
    import vorbis_amd
    mixed, stereo = _chain()
    plain = cases.files()["plain"][0]
    got, status = vorbis_amd.decode_ogg_files([mixed, plain, stereo], with_status=True, follow_links=True, links=True)
    assert not status.any() and [len(g) for g in got] == [3, 1, 2]
    for f, parts in zip((mixed, plain, stereo), got):
        for p, want in zip(parts, cases.expected(f)[1]):
            assert same(p, want)
    assert [int(p.shape[0]) for p in got[0]] == [2, 1, 2]
    whole, status = vorbis_amd.decode_ogg_files([stereo, plain], with_status=True, follow_links=True)
    assert not status.any() and same(whole[0], cases.expected(stereo)[0]) and same(whole[1], cases.expected(plain)[0])
    with pytest.raises(ValueError, match="links=True"):
        vorbis_amd.decode_ogg_files([mixed], follow_links=True)
    assert [(b, e) for b, e, _ in vorbis_amd.ogg_links(mixed)] == [(b, e) for b, e, _, _ in cases.read_links(mixed)]
    assert [s for _, _, s in vorbis_amd.ogg_links(stereo)] == [0x410, 0x411]
    # without the policy, as before: flagged at the second serial number
    _, status = vorbis_amd.decode_ogg_files([mixed, plain], with_status=True)
    assert list(status) == [BADPAGE, 0]


def test_a_cut_packet_in_the_second_link():
    """under keep_partial a packet cut short in the second of three links is decoded as libvorbis decodes it"""
    import vorbis_amd
    a, b, c = (cases.stream(cases.STEREO, v) for v in range(3))
    k = len(b.packets) - 2  # a long block's packet, cut inside its residue
    cut = b.packets[:k] + [b.packets[k][:len(b.packets[k]) * 2 // 3]] + b.packets[k + 1:]
    f = b"".join(cases.logical(a, 0x500) + cases.logical(b, 0x501, packets=cut) + cases.logical(c, 0x502))
    an = vorbis_amd.Analyzer(a.blob)
    try:
        an.keep_partial = True
        got, status = an.decode_ogg([f], a.headers[2], with_status=True, follow_links=True)
        assert status[0] == PARTIAL and same(got[0], cases.expected(f)[0])
        an.keep_partial = False
        got, status = an.decode_ogg([f, cases.files()["two_links"][0]], a.headers[2], with_status=True, follow_links=True)
        assert status[0] & 16 and got[0].shape[1] == 0  # STATUS_TRUNCATED: the flagged link flags its file
        assert status[1] == 0 and same(got[1], cases.expected(cases.files()["two_links"][0])[0])  # ... and no other
    finally:
        an.close()


def test_policy_off_flags_a_chained_file():
    import vorbis_amd
    a = cases.stream()
    F = cases.files()
    got, status = vorbis_amd.decode_ogg(a.blob, [F["two_links"][0], F["foreign_bos_first"][0]], a.headers[2], with_status=True)
    assert list(status) == [BADPAGE, BADPAGE] and all(g.shape[1] == 0 for g in got)
    got, status = vorbis_amd.decode_ogg(a.blob, [F["two_links"][0], F["other_setup"][0]], a.headers[2], with_status=True, follow_links=True)
    assert list(status) == [0, cases.STATUS_BADHEADER] and same(got[0], cases.expected(F["two_links"][0])[0])
    assert np.asarray(got[1].shape).tolist() == [2, 0]
