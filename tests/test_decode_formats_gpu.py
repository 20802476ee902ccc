"""GPU: the decoded signal in the caller's format (vamd_decode_output, vamd_pcm_convert; Analyzer.pcm_dtype /
.pcm_interleaved, the dtype= / interleaved= keywords) -- int16 as ov_read converts, fp16, bf16, and [frames, ch] -- through
every kind of decode entry: k_lap_as, k_lap_window_as and k_lap_segments_as in k_lap's place.  Expectations are libvorbis'
floats (ref_host.reference_decode, or the case modules' own readers) converted by tests/decode_formats_cases.py's
formulas and compared as bits; tests/test_decode_formats_cpu.py has taken the same bodies through the host build."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref
from tests import decode_links_cases as links, decode_live_host as live, ogg_demux_cases, ref_host, synth_host
from tests.decode_formats_cases import DTYPES, TORCH, differ, edge_table, tensor_bits, want_bits
from tests.feed_cases import Q4, same_bits
from tests.signals import gated_streams

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")]
EINVAL = -131
FORMATS = [(d, il) for d in DTYPES for il in (False, True)]
_rows = {}


def analyzer(name):
    import vorbis_amd
    return vorbis_amd.Analyzer(ref_host.encoder(name).pack_setup())


def reference_rows(name):
    """streams of SHORT_LENGTHS frames, 0.3 s and 0.7 s through the reference encoder and decoder, once per process
    -> per stream (packets, end granule, libvorbis' floats [ch][frames])"""
    if name not in _rows:
        ch = synth_host.SETUPS[name][0]
        rng = np.random.default_rng(3)
        parts = [((rng.random((n, ch), dtype=np.float32) - 0.5) * 0.8).astype(np.float32) for n in synth_host.SHORT_LENGTHS]
        parts += gated_streams(name, (0.3, 0.7), 11)
        headers = ref_host.encoder_headers(ref_host.encoder(name))
        out = []
        for p in parts:
            recs = ref_host.encoder(name).encode_stream(np.ascontiguousarray(p.T))
            packets, granules = [r["packet"] for r in recs], [r["granulepos"] for r in recs]
            want = ref_host.reference_decode(headers + packets, granules)
            assert want.shape == (ch, len(p))
            want.setflags(write=False)
            out.append((packets, granules[-1], want))
        _rows[name] = out
    return _rows[name]


def expect(want, dtype, il):
    """libvorbis' floats [ch][frames] -> the elements the format holds, in the tensor's shape"""
    return want_bits(np.ascontiguousarray(want.T) if il else want, dtype)


def assert_same(t, want, dtype, il, what):
    got = tensor_bits(t, dtype)
    exp = expect(want, dtype, il)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    assert not differ(got, exp, dtype).any(), (what, int(differ(got, exp, dtype).sum()))


@pytest.mark.parametrize("name", ["44k_stereo_q4", "44k_mono_q5", "44k_51_q3"])
def test_streams_in_every_format(name):
    rows = reference_rows(name)
    packets, ends = [r[0] for r in rows], [r[1] for r in rows]
    an = analyzer(name)
    try:
        for d, il in FORMATS:
            got, status = an.decode_streams(packets, ends, with_status=True, dtype=TORCH[d], interleaved=il)
            assert not status.any() and an.pcm_dtype == TORCH["f32"] and an.pcm_interleaved is False  # (per call: the context's stands)
            for s, (t, r) in enumerate(zip(got, rows)):
                assert t.is_cuda and t.dtype == TORCH[d]
                assert_same(t, r[2], d, il, (name, d, il, s))
    finally:
        an.close()


@pytest.mark.parametrize("d,il", [("s16", True), ("f16", False), ("f32", True), ("bf16", False)])
def test_odd_offsets_and_guards_through_ctypes(d, il):
    """vamd_decode_plan + vamd_decode_streams as a C caller drives them: the streams 5 or 7 elements apart from an odd first
    offset, every element that is no stream's still the fill afterwards"""
    import torch
    import vorbis_amd
    from vorbis_amd.abi import _PcmFormat
    rows = reference_rows(Q4)
    an = analyzer(Q4)
    try:
        prep = an.decode_prepare([r[0] for r in rows], [r[1] for r in rows])
        ns = len(rows)
        frames, nblocks = np.zeros(ns, np.int64), np.zeros(2, np.int64)
        vp = C.c_void_p
        assert an.L.vamd_decode_plan(an.h, C.byref(prep["desc"]), vp(frames.ctypes.data), vp(nblocks.ctypes.data)) == 0
        assert [int(f) for f in frames] == [r[2].shape[1] for r in rows]
        off, at = np.zeros(ns, np.int64), 3
        for s in range(ns):
            off[s] = at
            at += 2 * int(frames[s]) + (5 if s % 2 else 7)
        assert any(int(o) % 2 for o in off) and any(int(o) % 8 not in (0, 4) for o in off)
        fill = {"f32": 7.5, "s16": 0x5a5a, "f16": 7.5, "bf16": 7.5}[d]
        pcm = torch.full((at + 9,), fill, dtype=TORCH[d], device=an._dev())
        before = tensor_bits(pcm, d).copy()
        status = np.zeros(ns, np.uint8)
        fmt = _PcmFormat(DTYPES.index(d), 1 if il else 0)
        assert an.L.vamd_decode_output(an.h, C.byref(fmt)) == 0
        an._bind_stream()
        assert an.L.vamd_decode_streams(an.h, C.byref(prep["desc"]), vp(off.ctypes.data), vp(pcm.data_ptr()), vp(status.ctypes.data)) == 0
        torch.cuda.synchronize()
        assert not status.any()
        got = tensor_bits(pcm, d)
        mine = np.zeros(got.size, bool)
        for s, r in enumerate(rows):
            a, n = int(off[s]), 2 * int(frames[s])
            exp = expect(r[2], d, il).reshape(-1)
            assert not differ(got[a:a + n], exp, d).any(), (s, int(differ(got[a:a + n], exp, d).sum()))
            mine[a:a + n] = True
        assert np.array_equal(got[~mine], before[~mine]) and (~mine).sum() >= 3 + 5 * ns
    finally:
        an.close()


def test_s16_clips_as_ov_read():
    """a full-scale square wave at the lowest quality decodes beyond full scale on both sides: ov_read's clip is at work"""
    name = "44k_stereo_qm1"
    t = np.arange(6000)
    sq = np.sign(np.sin(2 * np.pi * t * 441 / 44100.0)).astype(np.float32)
    x = np.clip(np.stack([sq, -sq]), -1.0, 32767 / 32768.0).astype(np.float32)
    recs = ref_host.encoder(name).encode_stream(np.ascontiguousarray(x))
    packets, granules = [r["packet"] for r in recs], [r["granulepos"] for r in recs]
    want = ref_host.reference_decode(ref_host.encoder_headers(ref_host.encoder(name)) + packets, granules)
    assert want.shape == (2, 6000) and (want > 32767 / 32768.0).sum() > 100 and (want < -1.0).sum() > 100  # (the reference's floats alone)
    an = analyzer(name)
    try:
        for il in (False, True):
            got, status = an.decode_streams([packets], [granules[-1]], with_status=True, dtype=TORCH["s16"], interleaved=il)
            assert not status.any()
            assert_same(got[0], want, "s16", il, il)
            g = got[0].cpu().numpy()
            assert (g == 32767).sum() > 100 and (g == -32768).sum() > 100
    finally:
        an.close()


def test_a_chained_file_in_s16_interleaved():
    """vamd_decode_ogg under follow_links on a three-link file: several rows for k_lap_segments_as, end to end in one
    [frames, ch] tensor; a plain file beside it"""
    import vorbis_amd
    F, a = links.files(), links.stream(links.STEREO, 0)
    files = [F["three_links"][0], F["plain"][0], F["trim_k3_below"][0]]
    assert len(links.expected(files[0])[1]) == 3
    an = vorbis_amd.Analyzer(a.blob)
    try:
        got, status = an.decode_ogg(files, a.headers[2], with_status=True, follow_links=True, dtype=TORCH["s16"], interleaved=True)
        assert not status.any()
        for f, t in zip(files, got):
            assert_same(t, links.expected(f)[0], "s16", True, "links")
        got = an.decode_ogg(files, a.headers[2], follow_links=True, dtype=TORCH["bf16"])
        for f, t in zip(files, got):
            assert_same(t, links.expected(f)[0], "bf16", False, "links planar")
    finally:
        an.close()
    whole = vorbis_amd.decode_ogg_files(files[:2], follow_links=True, dtype=TORCH["s16"], interleaved=True)
    for f, t in zip(files, whole):
        assert_same(t, links.expected(f)[0], "s16", True, "decode_ogg_files")


def test_crops_and_windows():
    """OggIndex.crops interleaved: [n, length, ch], the valid part bit-equal, the tail exactly zero; windows at unaligned
    starts; a channel stride under an interleaved format is refused before anything is enqueued"""
    import torch
    import vorbis_amd
    blob, headers, files = ogg_demux_cases.base_files(Q4, "seeded")
    wants = [ogg_demux_cases.expected(f)[2] for f in files]
    Ts = [w.shape[1] for w in wants]
    length = 1500
    stream = [0, 1, 2, 3, 0, 1, 2]
    start = [0, Ts[1] - 1500, Ts[2] - 1499, Ts[3] - 1, 4321, Ts[1], Ts[2] + 9]
    valid_want = [1500, 1500, 1499, 1, 1500, 0, 0]
    an = vorbis_amd.Analyzer(blob)
    try:
        x = an.ogg_index(files, headers[2])
        for d, il in (("s16", True), ("f32", True), ("f16", True), ("bf16", False)):
            pcm, valid = x.crops(stream, start, length, dtype=TORCH[d], interleaved=il)
            assert tuple(pcm.shape) == ((len(stream), length, 2) if il else (len(stream), 2, length)) and pcm.dtype == TORCH[d]
            assert [int(v) for v in valid] == valid_want
            got = tensor_bits(pcm, d)
            for w, (s, a) in enumerate(zip(stream, start)):
                n = valid_want[w]
                head, tail = (got[w][:n], got[w][n:]) if il else (got[w][:, :n], got[w][:, n:])
                assert not differ(head, expect(wants[s][:, a:a + n], d, il), d).any(), (d, il, w)
                assert not tail.any(), (d, il, w)
        windows = [(0, 1, 9), (1, 4321, 1237), (2, 333, 2051), (3, Ts[3] - 5, 100)]
        got, status = x.decode([w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows], with_status=True,
                               dtype=TORCH["s16"], interleaved=True)
        assert not status.any()
        for (s, a, n), t in zip(windows, got):
            assert_same(t, wants[s][:, a:min(a + n, Ts[s])], "s16", True, (s, a, n))
        # channel_stride names rows of a planar layout
        an.pcm_interleaved = True
        pcm = torch.full((2 * 2 * length,), 7.5, dtype=torch.float32, device=an._dev())
        with pytest.raises(vorbis_amd.VamdError) as e:
            x._run([0, 1], [0, 5], [length, length], pcm=pcm, stride=length)
        assert e.value.code == EINVAL and "channel_stride" in str(e.value)
        torch.cuda.synchronize()
        assert (pcm == 7.5).all()
        an.pcm_interleaved = False
        ok, valid = x.crops(stream[:2], start[:2], length)
        assert same_bits(ok[0].cpu().numpy(), wants[0][:, :length])
    finally:
        an.close()


def test_live_pieces():
    """a live decoder's pieces laid end to end are the whole-stream call, in S16; and with the format switched from piece
    to piece (the carry between pieces stays fp32)"""
    rows = [reference_rows(Q4)[k] for k in (8, 9, 6)]
    packets, ends, want = [r[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows]
    rng = np.random.default_rng(5)
    cuts = [sorted(set(int(v) for v in rng.integers(1, len(p), 3))) for p in packets]
    calls, who = live.rounds(packets, cuts, ends)
    assert len(calls) >= 3
    an = analyzer(Q4)
    try:
        whole = an.decode_streams(packets, ends, dtype=TORCH["s16"])
        whole = [w.cpu().numpy() for w in whole]
        for s in range(len(rows)):
            assert np.array_equal(whole[s], want_bits(want[s], "s16"))
        dec = an.live_decoder(len(rows))
        for switch in (False, True):
            seq = [("s16", False)] * len(calls) if not switch else [FORMATS[(3 * r + 2) % len(FORMATS)] for r in range(len(calls))]
            at, parts = [0] * len(rows), [[] for _ in rows]
            for (slots, pieces, close, granules), live_rows, (d, il) in zip(calls, who, seq):
                an.pcm_dtype, an.pcm_interleaved = TORCH[d], il
                got, status = dec.write(slots, pieces, close, granules, with_status=True)
                assert not status.any()
                for i, t in zip(live_rows, got):
                    n = t.shape[0] if il else t.shape[1]
                    assert_same(t, want[i][:, at[i]:at[i] + n], d, il, (switch, i, at[i], d, il))
                    at[i] += n
                    if not switch:
                        parts[i].append(t.cpu().numpy())
            assert at == [w.shape[1] for w in want]
            if not switch:
                for s in range(len(rows)):
                    assert np.array_equal(np.concatenate(parts[s], axis=1), whole[s])
            assert len(set(seq)) >= (3 if switch else 1)
    finally:
        an.close()


def test_pcm_convert_on_the_edge_table():
    import torch
    import vorbis_amd
    x = edge_table()
    x = np.concatenate([x, x[:(-len(x)) % 6]]) if len(x) % 6 else x
    an = analyzer(Q4)
    try:
        for ch in (1, 2, 6):
            src = np.ascontiguousarray(x.reshape(ch, -1))
            dev = torch.from_numpy(src).to(an._dev())
            for d, il in FORMATS:
                out = an.pcm_convert(dev, TORCH[d], il)
                assert tuple(out.shape) == (src.shape[::-1] if il else src.shape)
                got, exp = tensor_bits(out, d), expect(src, d, il)
                bad = differ(got, exp, d)
                assert not bad.any(), (ch, d, il, [(float(v), int(g), int(w)) for v, g, w in zip((src.T if il else src)[bad], got[bad], exp[bad])])
        s16 = dict(zip([repr(float(v)) for v in x], tensor_bits(an.pcm_convert(torch.from_numpy(x[None]).to(an._dev()), torch.int16), "s16")[0]))
        assert s16["65536.0"] == 32767 and s16["-65536.0"] == -32768 and s16["inf"] == 32767 and s16["-inf"] == -32768 and s16["nan"] == 0
        with pytest.raises(ValueError):
            an.pcm_convert(dev, torch.int8)
    finally:
        an.close()
    out = vorbis_amd.pcm_convert(torch.from_numpy(x[None].copy()).cuda(), torch.float16, interleaved=True)
    assert not differ(tensor_bits(out, "f16"), expect(x[None], "f16", True), "f16").any()


def test_the_default_is_unchanged_and_bad_formats_are_refused():
    import torch
    import vorbis_amd
    from vorbis_amd.abi import _PcmFormat
    rows = reference_rows(Q4)
    packets, ends = [r[0] for r in rows], [r[1] for r in rows]
    vp = C.c_void_p
    an = analyzer(Q4)
    try:
        before = [t.cpu().numpy() for t in an.decode_streams(packets, ends)]
        for g, r in zip(before, rows):
            assert same_bits(g, r[2])
        an.pcm_dtype, an.pcm_interleaved = torch.int16, True
        assert an.pcm_dtype == torch.int16 and an.pcm_interleaved is True
        assert an.decode_streams(packets, ends)[-1].dtype == torch.int16
        assert an.L.vamd_decode_output(an.h, None) == 0
        an._pcm_dtype, an._pcm_interleaved = torch.float32, False   # (the call above went past the binding's mirror)
        after = [t.cpu().numpy() for t in an.decode_streams(packets, ends)]
        assert all(a.dtype == np.float32 and same_bits(a, b) for a, b in zip(after, before))
        # an unknown dtype: refused, and the format stands
        for bad in (4, -1, 17):
            assert an.L.vamd_decode_output(an.h, C.byref(_PcmFormat(bad, 0))) == EINVAL
        with pytest.raises(ValueError):
            an.pcm_dtype = torch.float64
        assert all(same_bits(t.cpu().numpy(), b) for t, b in zip(an.decode_streams(packets, ends), before))
        # a pcm of another dtype; a pcm off its element's alignment
        prep = an.decode_prepare(packets, ends)
        total = sum(2 * r[2].shape[1] for r in rows)
        an.pcm_dtype = torch.int16
        with pytest.raises(ValueError):
            an.decode_run(prep, pcm=torch.zeros(total + 4, dtype=torch.float32, device=an._dev()))
        buf = torch.full((2 * total + 16,), 0x5a, dtype=torch.uint8, device=an._dev())
        off, status = np.zeros(len(rows), np.int64), np.zeros(len(rows), np.uint8)
        off[1:] = np.cumsum([2 * r[2].shape[1] for r in rows])[:-1]
        an._bind_stream()
        assert an.L.vamd_decode_streams(an.h, C.byref(prep["desc"]), vp(off.ctypes.data), vp(buf.data_ptr() + 1), vp(status.ctypes.data)) == EINVAL
        assert b"aligned" in an.L.vamd_last_error(an.h)
        an.pcm_dtype = torch.float32
        big = torch.full((4 * total + 16,), 0x5a, dtype=torch.uint8, device=an._dev())
        assert an.L.vamd_decode_streams(an.h, C.byref(prep["desc"]), vp(off.ctypes.data), vp(big.data_ptr() + 2), vp(status.ctypes.data)) == EINVAL
        torch.cuda.synchronize()
        assert (buf == 0x5a).all() and (big == 0x5a).all()
        # the context still works
        assert all(same_bits(t.cpu().numpy(), b) for t, b in zip(an.decode_streams(packets, ends), before))
        got = an.decode_streams(packets, ends, dtype=torch.float16, interleaved=True)
        assert_same(got[-1], rows[-1][2], "f16", True, "afterwards")
    finally:
        an.close()
