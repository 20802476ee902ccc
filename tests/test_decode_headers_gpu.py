"""GPU: the decoder made from a stream's own headers (vamd_create_decoder; Analyzer.from_headers, read_ogg_headers,
decode_ogg_files) -- every decode entry on such a context against libvorbis' decoder under the same headers, bit for bit, and
against the blob context's output; headers no encoder here wrote (tests/setup_header_cases.py: explicit value lists,
non-integer steps, q_sequencep, another quantlist order), which take k_synth_values; the refusals; files of several setups
in one call."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref
from tests import decode_cases, decode_live_host as live, ogg_demux_cases as cases, ogg_framing, ref_host, setup_header_cases as shc, synth_host
from tests.feed_cases import Q4, same_bits

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")]
EIMPL = -130
VALUE_KINDS = ("explicit", "scaled", "sequence", "permuted")
_want = {}


def from_headers(headers):
    import vorbis_amd
    return vorbis_amd.Analyzer.from_headers(headers[0], headers[2])


def reference(headers, packets, end):
    key = (bytes(headers[2]), tuple(packets), end)
    if key not in _want:
        w = ref_host.reference_decode(list(headers) + list(packets), [-1] * (len(packets) - 1) + [end])
        w.setflags(write=False)
        _want[key] = w
    return _want[key]


def assert_streams(got, status, headers, streams, ends, what):
    assert len(got) == len(streams)
    for s, (packets, end) in enumerate(zip(streams, ends)):
        want, g = reference(headers, packets, end), got[s].cpu().numpy()
        assert status[s] == 0 and g.shape == want.shape, (what, s, int(status[s]), g.shape, want.shape)
        assert same_bits(g, want), (what, s, int((g.view(np.uint32) != want.view(np.uint32)).sum()))


@pytest.mark.parametrize("name", synth_host.FEED_SETUPS)
def test_feed_setups_equal_the_reference_and_the_blob_context(name):
    """the four base streams (some 20 packets each, both block sizes) and, for the stereo setup, the short streams: one-frame
    streams and end granules that cut the last block"""
    import vorbis_amd
    blob, headers, _, base = decode_cases.base_streams(name, 1)
    streams, ends = [p for p, _ in base], [e for _, e in base]
    a, b = from_headers(headers), vorbis_amd.Analyzer(blob)
    try:
        assert "value_books=0" in a.L.vamd_config_string(a.h).decode()  # every genuine book is a lattice book: k_synth as ever
        got, status = a.decode_streams(streams, ends, with_status=True)
        assert_streams(got, status, headers, streams, ends, name)
        for x, y in zip(got, b.decode_streams(streams, ends)):
            assert same_bits(x.cpu().numpy(), y.cpu().numpy())
        assert (a.channels, a.blocksizes) == (b.channels, b.blocksizes)
        assert [a.L.vamd_submaps(a.h, W) for W in (0, 1)] == [b.L.vamd_submaps(b.h, W) for W in (0, 1)]
        assert [a.L.vamd_residue_capacity(a.h, W) for W in (0, 1)] == [b.L.vamd_residue_capacity(b.h, W) for W in (0, 1)]
        if name == Q4:
            g = decode_cases.short_streams(24)
            got, status = a.decode_streams(g.streams, g.ends, with_status=True)
            decode_cases.check(g, [(int(status[s]), got[s].cpu().numpy()) for s in range(len(got))])
    finally:
        a.close(), b.close()


@pytest.mark.parametrize("name", tuple(shc.EXTRA))
def test_setups_no_blob_is_shipped_for(name):
    enc = shc.encoder(name)
    headers = ref_host.encoder_headers(shc.encoder(name))
    from tests.signals import gated_noise
    recs = enc.encode_stream(gated_noise(enc.channels, enc.rate, 6000, 77))
    packets, end = [r["packet"] for r in recs], recs[-1]["granulepos"]
    a = from_headers(headers)
    try:
        got, status = a.decode_streams([packets], [end], with_status=True)
        assert_streams(got, status, headers, [packets], [end], name)
    finally:
        a.close()


@pytest.mark.parametrize("kind", VALUE_KINDS)
@pytest.mark.parametrize("name", ("44k_stereo_q4", "44k_mono_q5", "44k_51_q3"))
def test_value_path_equals_the_reference(name, kind):
    """type 2, type 1 and two submaps under headers whose residue books are no lattice books: k_synth_values"""
    _, headers, _, base = decode_cases.base_streams(name, 1)
    hv = shc.variant(headers, kind)
    streams, ends = [p for p, _ in base], [e for _, e in base]
    a = from_headers(hv)
    try:
        assert "value_books=0" not in a.L.vamd_config_string(a.h).decode()
        got, status = a.decode_streams(streams, ends, with_status=True)
        assert_streams(got, status, hv, streams, ends, (name, kind))
        if kind == "explicit":  # the same values written out: the original's PCM
            assert_streams(got, status, headers, streams, ends, (name, kind, "original"))
    finally:
        a.close()


def test_mutated_packets_under_an_explicit_header():
    """clean streams among decode_cases' mutations: statuses and classes as under the original header"""
    g = decode_cases.with_clean(decode_cases.cases(Q4, 24), 8)
    a = from_headers(shc.variant(g.headers, "explicit"))
    try:
        got, status = a.decode_streams(g.streams, g.ends, with_status=True)
        decode_cases.check(g, [(int(status[s]), got[s].cpu().numpy()) for s in range(len(got))])
    finally:
        a.close()


def test_refusals():
    import torch
    import vorbis_amd
    headers = ref_host.encoder_headers(ref_host.encoder(Q4))
    for h, word in ((shc.variant(headers, "modes3"), "3 modes"), (shc.variant(headers, "residue0"), "residue type 0"), (shc.ident_8192(headers), "8192")):
        with pytest.raises(vorbis_amd.VamdError) as e:
            from_headers(h)
        assert e.value.code == EIMPL and word in str(e.value), str(e.value)
    with pytest.raises(vorbis_amd.VamdError) as e:
        from_headers([headers[0], headers[1], headers[2][:-40]])
    assert e.value.code == vorbis_amd.VAMD_EBADHEADER
    with pytest.raises(vorbis_amd.VamdError) as e:
        from_headers([b"\x01vorbiz" + headers[0][7:], headers[1], headers[2]])
    assert e.value.code == vorbis_amd.VAMD_ENOTVORBIS
    # every encode entry of the C ABI refuses a decode-only context before it looks at an argument (null ones here), the
    # binding's methods raise, and the context decodes on
    from vorbis_amd.abi import PROTOTYPES
    guarded = ("vamd_reserve", "vamd_mdct_forward_batch", "vamd_analyze_batch", "vamd_analyze_batch_synth", "vamd_synth_streams",
               "vamd_analyze_batch_managed", "vamd_analyze_stream", "vamd_analyze_stream_mixed", "vamd_analyze_streams_mixed",
               "vamd_analyze_streams_mixed_managed", "vamd_bitrate_init_states", "vamd_bitrate_walk", "vamd_analyze_block_managed",
               "vamd_analyze_block", "vamd_analyze_block_res", "vamd_encode_block", "vamd_encode_blocks", "vamd_envelope_search",
               "vamd_envelope_search_batch", "vamd_plan_streams", "vamd_plan_streams_whole", "vamd_plan_streams_whole_v")
    _, _, _, base = decode_cases.base_streams(Q4, 1)
    a = from_headers(headers)
    try:
        for name in guarded:
            r = getattr(a.L, name)(a.h, *[t() for t in PROTOTYPES[name][1][1:]])
            assert r == EIMPL and "decode-only context" in a.L.vamd_last_error(a.h).decode(), (name, r)
        live_plan = a.L.vamd_live_plan  # (the feed's entry: not among the binding's prototypes)
        live_plan.restype, live_plan.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_long, C.c_long, C.c_long, C.c_void_p, C.c_int] + [C.c_void_p] * 2 + [
            C.c_long] + [C.c_void_p] * 3
        assert live_plan(a.h, None, 0, 0, 0, None, 0, None, None, 0, None, None, None) == EIMPL
        pcm = torch.zeros((2, 2, 2048), dtype=torch.float32, device="cuda")
        host = np.zeros((2, 2048), np.float32)
        calls = [lambda: a.analyze(pcm, W=1, want=("mdct",)), lambda: a.analyze(pcm, W=1, want=("mdct", "synth")), lambda: a.mdct_forward(1, pcm),
                 lambda: a.analyze_block(host), lambda: a.encode_block(host), lambda: a.envelope_search(np.zeros((2, 4096), np.float32), 8),
                 lambda: a.analyze_block_managed(host), lambda: a.plan_streams(torch.zeros((1, 2, 8192), dtype=torch.float32, device="cuda")),
                 lambda: a.envelope_search_batch(torch.zeros((1, 2, 8192), dtype=torch.float32, device="cuda"), 8)]
        for k, call in enumerate(calls):
            with pytest.raises(vorbis_amd.VamdError) as e:
                call()
            assert e.value.code == EIMPL and "decode-only context" in str(e.value), (k, str(e.value))
        got, status = a.decode_streams([base[0][0]], [base[0][1]], with_status=True)
        assert_streams(got, status, headers, [base[0][0]], [base[0][1]], "after the refusals")
    finally:
        a.close()
    # a device that does not exist: the reason comes through vamd_last_error(NULL)
    h = C.c_void_p()
    L = vorbis_amd.load_library()
    assert L.vamd_create_decoder(C.byref(h), bytes(headers[0]), len(headers[0]), bytes(headers[2]), len(headers[2]), 9999) == vorbis_amd.VAMD_EFAULT
    assert "device" in L.vamd_last_error(None).decode()


def test_block_sizes_64_and_128_and_a_single_entry_book():
    """setup_header_cases.small_blocks: the short transforms, floors of range 32 and 64, posts read through a book of one
    entry -- packets of random bits, held to the reference"""
    hv, streams = shc.small_blocks(ref_host.encoder_headers(ref_host.encoder(Q4)))
    a = from_headers(hv)
    try:
        assert a.blocksizes == (64, 128)
        got, status = a.decode_streams(streams, [-1] * len(streams), with_status=True)
        assert_streams(got, status, hv, streams, [-1] * len(streams), "small blocks")
    finally:
        a.close()


def test_files_of_three_setups_and_a_damaged_header():
    import vorbis_amd
    names = ("44k_stereo_q4", "44k_mono_q5", "44k_51_q3")
    per = {n: cases.base_files(n, "shared") for n in names}
    files, who = [], []
    for i in range(2):
        for n in names:
            files.append(per[n][2][i]), who.append(n)
    bad = bytearray(per[Q4][2][2])
    at = bytes(bad).find(per[Q4][1][2][:32]) + 9  # inside the first codebook's sync pattern
    bad[at] ^= 0xff
    files.insert(3, bytes(bad)), who.insert(3, None)
    assert vorbis_amd.read_ogg_headers(files[0]) == tuple(bytes(h) for h in per[Q4][1])
    lens = (C.c_int64 * 3)()  # a buffer too small: the sizes needed, nothing written
    assert vorbis_amd.load_library().vamd_ogg_read_headers(files[0], len(files[0]), None, 0, lens) == vorbis_amd.VAMD_EINVAL
    assert list(lens) == [len(h) for h in per[Q4][1]]
    with pytest.raises(vorbis_amd.VamdError) as e:
        vorbis_amd.read_ogg_headers(files[0][:100])
    assert e.value.code == vorbis_amd.VAMD_EBADHEADER
    got, status = vorbis_amd.decode_ogg_files(files, with_status=True)
    for s, (f, n) in enumerate(zip(files, who)):
        if n is None:
            assert status[s] == vorbis_amd.STATUS_BADHEADER and tuple(got[s].shape) == (0, 0)
            continue
        want = cases.expected(f)[2]
        assert status[s] == 0 and same_bits(got[s].cpu().numpy(), want), (s, n, int(status[s]))
    # a file of another setup through a header-made context's decode_ogg: flagged, and alone
    a = from_headers(per[Q4][1])
    try:
        other = cases.base_files("44k_stereo_q9", "shared")[2][0]
        got, status = a.decode_ogg([per[Q4][2][0], other, per[Q4][2][1]], with_status=True)
        assert list(status) == [0, vorbis_amd.STATUS_BADHEADER, 0] and got[1].shape[1] == 0
        assert same_bits(got[2].cpu().numpy(), cases.expected(per[Q4][2][1])[2])
    finally:
        a.close()


def test_the_other_entries_on_a_header_made_context():
    """a live decoder over four streams in three pieces, a live Ogg decoder with a byte cut inside a page, an index and two
    windows: each equals the whole decode"""
    _, headers, _, base = decode_cases.base_streams(Q4, 1)
    streams, ends = [p for p, _ in base], [e for _, e in base]
    files = cases.base_files(Q4, "shared")[2]
    a = from_headers(headers)
    try:
        whole = [t.cpu().numpy() for t in a.decode_streams(streams, ends)]
        assert all(same_bits(w, reference(headers, p, e)) for w, p, e in zip(whole, streams, ends))
        dec = a.live_decoder(4)
        calls, who = live.rounds(streams, [[len(p) // 3, 2 * len(p) // 3] for p in streams], ends, None)
        res = []
        for slots, pieces, close, granules in calls:
            got, status = dec.write(slots, pieces, close, granules, with_status=True)
            res.append([(int(status[i]), got[i].cpu().numpy()) for i in range(len(got))])
        for (st, pcm), w in zip(live.join(res, who, 4, a.channels), whole):
            assert st == 0 and same_bits(pcm, w)
        f = files[0]
        pages = ogg_framing.demux(f)[0]
        cut = pages[len(pages) // 2]["offset"] + pages[len(pages) // 2]["bytes"] // 2  # inside a page
        odec = a.live_ogg_decoder(1)
        p1, s1 = odec.write([0], [f[:cut]], with_status=True)
        p2, s2 = odec.write([0], [f[cut:]], close=[0], with_status=True)
        joined = np.concatenate([p1[0].cpu().numpy(), p2[0].cpu().numpy()], axis=1)
        assert not s1.any() and not s2.any() and same_bits(joined, cases.expected(f)[2])
        x = a.ogg_index(files[:2])
        got, status = x.decode([0, 1], [1000, 4321], [2048, 777], with_status=True)
        assert not status.any()
        assert same_bits(got[0].cpu().numpy(), cases.expected(files[0])[2][:, 1000:1000 + 2048])
        assert same_bits(got[1].cpu().numpy(), cases.expected(files[1])[2][:, 4321:4321 + 777])
        x.close()
        got, status = a.decode_window(streams, ends, [2], [500], [3000], with_status=True)
        assert not status.any() and same_bits(got[0].cpu().numpy(), whole[2][:, 500:3500])
    finally:
        a.close()
