"""GPU: the decoded feed (VAMD_FEED_DECODED, vamd_feed_decoded; include/vorbis_amd.h "the decoded feed") -- per stream the
signal on the device against libvorbis' decoder run over the feed's own packets with their granule positions
(tests/ref_host.py: vorbis_synthesis + vorbis_synthesis_blockin + vorbis_synthesis_pcmout), bit for bit."""
import numpy as np
import pytest

from oracle import ref
from tests import ref_host, synth_host
from tests.feed_cases import Q4, decoded_feed_of as feed_of, same_bits, small_arena
from tests.signals import gated_noise, gated_streams as streams

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built (needs /root/reference)")]
EINVAL, EIMPL = -131, -130


def wrote(feed, parts):
    slot, buf = feed.buffer(parts[0].shape[1])
    flat = np.concatenate([p.reshape(-1) for p in parts])
    buf[:flat.size] = flat
    feed.wrote(slot, len(parts), np.array([len(p) for p in parts], np.int64))
    return slot


def collect(feed, slot, ns, ogg=False):
    """-> the group's record, rows, files, decoded tensors (on the host) and status; the slot released"""
    r = feed.packets(slot)
    out = dict(r=r, rows=feed._rows(r, ns))
    if ogg:
        o = feed.ogg(slot)
        out["files"] = [bytes(o["bytes"][int(o["stream_offset"][s]):int(o["stream_offset"][s + 1])]) for s in range(ns)]
    if feed.is_decoded:
        dec, out["status"] = feed.decoded(slot, with_status=True)
        out["device"] = [d.device.index for d in dec]
        out["dec"] = [d.cpu().numpy() for d in dec]
    feed.release(slot)
    return out


def group(feed, parts, ogg=False):
    return collect(feed, wrote(feed, parts), len(parts), ogg)


def reference_decode_rows(headers, row):
    return ref_host.reference_decode(headers + [p for p, _, _, _ in row], [gp for _, gp, _, _ in row])


def check_against_decoder(name, parts, got, skip=()):
    headers = ref_host.encoder_headers(ref_host.encoder(name))
    for s, p in enumerate(parts):
        if s in skip:
            continue
        want = reference_decode_rows(headers, got["rows"][s])
        assert want.shape == (p.shape[1], len(p)), (s, want.shape)
        assert got["status"][s] == 0
        assert same_bits(got["dec"][s], want), "stream %d: %d samples differ" % (
            s, int((got["dec"][s].view(np.uint32) != want.view(np.uint32)).sum()) if got["dec"][s].shape == want.shape else -1)


@pytest.mark.parametrize("name", synth_host.FEED_SETUPS)
def test_decoded_equals_the_reference_decoder(name):
    parts = streams(name, (0.3, 0.7, 1.1, 1.5), 11)
    feed = feed_of(name, parts)
    try:
        got = group(feed, parts)
    finally:
        feed.close()
    enc = ref_host.encoder(name)
    if enc.blocksize(0) != enc.blocksize(1):  # long/long, long/short, short/long, short/short
        assert set().union(*[synth_host.lap_cases([W for _, _, W, _ in row]) for row in got["rows"]]) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    for s, p in enumerate(parts):  # the packets are the reference encoder's (as tests/test_feed.py checks)
        want = ref_host.encoder(name).encode_stream(np.ascontiguousarray(p.T))
        assert [(w["packet"], w["granulepos"], w["W"], w["eos"]) for w in want] == got["rows"][s], "stream %d's packets" % s
    check_against_decoder(name, parts, got)


def test_short_streams():
    rng = np.random.default_rng(3)
    parts = [((rng.random((n, 2), dtype=np.float32) - 0.5) * 0.8).astype(np.float32) for n in synth_host.SHORT_LENGTHS]
    feed = feed_of(Q4, parts)
    try:
        got = group(feed, parts)
    finally:
        feed.close()
    assert [d.shape for d in got["dec"]] == [(2, n) for n in synth_host.SHORT_LENGTHS]
    check_against_decoder(Q4, parts, got)


@pytest.mark.parametrize("arena", [None, "4096"])
def test_the_flag_changes_nothing_else(arena, monkeypatch):
    """the same group through a feed with and without the flag, and through an Ogg feed with and without it: packets,
    granule positions, info and files byte for byte; arena: the packet arena starts at 4096 bytes and has to grow"""
    small_arena(monkeypatch, arena)
    parts = streams(Q4, (0.4, 0.25, 0.6), 21)
    headers = ref_host.reference_headers(2, 44100, 0.4)
    res = {}
    for key, kw in (("plain", dict(decoded=False)), ("decoded", dict()), ("ogg", dict(decoded=False, ogg_headers=headers)),
                    ("ogg_decoded", dict(ogg_headers=headers))):
        feed = feed_of(Q4, parts, **kw)
        try:
            res[key] = group(feed, parts, ogg="ogg" in key)
        finally:
            feed.close()
    assert not arena or res["plain"]["r"]["total_bytes"] > 4096
    for key in ("decoded", "ogg", "ogg_decoded"):
        for k in ("nstreams", "nblocks", "total_bytes"):
            assert res[key]["r"][k] == res["plain"]["r"][k], (key, k)
        for k in ("stream_start", "offset", "bits", "granulepos", "info", "bytes"):
            assert np.array_equal(res[key]["r"][k], res["plain"]["r"][k]), (key, k)
    assert res["ogg_decoded"]["files"] == res["ogg"]["files"] and all(len(f) > 1000 for f in res["ogg"]["files"])
    check_against_decoder(Q4, parts, res["decoded"])
    check_against_decoder(Q4, parts, res["ogg_decoded"])


def test_device_fed_group():
    """a bf16 (streams, channels, frames) tensor that is a strided view, through roundtrip_tensors: the decoded tensors are
    those of a host-fed float group of the same values, lie on the lane's device, and survive release and the next group"""
    import torch
    frames = 20000
    x = np.stack([gated_noise(2, 44100, 2 * frames, 40 + s) for s in range(3)])
    wide = torch.from_numpy(x).cuda().to(torch.bfloat16)
    view = wide[:, :, ::2]
    assert not view.is_contiguous()
    parts = [np.ascontiguousarray(view[s].float().cpu().numpy().T) for s in range(3)]
    feed = feed_of(Q4, parts)
    try:
        rows, dec = feed.roundtrip_tensors(view)
        assert all(d.is_cuda and d.device.index == feed.device(0) and d.shape == (2, frames) for d in dec)
        saved = [d.cpu().numpy() for d in dec]
        host = group(feed, parts)
        other = group(feed, [p[::-1].copy() for p in parts])  # the next group on the slot
        torch.cuda.synchronize()
        assert all(np.array_equal(d.cpu().numpy().view(np.uint32), s.view(np.uint32)) for d, s in zip(dec, saved))
    finally:
        feed.close()
    assert rows == host["rows"] and all(len(r) > 10 for r in rows)
    assert all(same_bits(a, b) for a, b in zip(saved, host["dec"]))
    assert not same_bits(other["dec"][0], host["dec"][0])
    check_against_decoder(Q4, parts, host)


def test_two_groups_in_flight():
    a, b = streams(Q4, (0.5, 0.3), 51), streams(Q4, (0.2, 0.6, 0.4), 61)
    feed = feed_of(Q4, b, lanes_per_device=2)
    try:
        slot_a = wrote(feed, a)
        slot_b = wrote(feed, b)
        assert slot_a != slot_b
        got_b = collect(feed, slot_b, len(b))
        got_a = collect(feed, slot_a, len(a))
    finally:
        feed.close()
    check_against_decoder(Q4, a, got_a)
    check_against_decoder(Q4, b, got_b)


def test_a_non_finite_sample_costs_its_stream_the_signal():
    import vorbis_amd
    parts = streams(Q4, (0.4, 0.4, 0.3), 71)
    parts[1][5000, 0] = np.nan
    feed = feed_of(Q4, parts)
    try:
        got = group(feed, parts)
    finally:
        feed.close()
    assert got["status"][1] == vorbis_amd.api.STATUS_NONFINITE and got["dec"][1].shape == (2, 0)
    assert any(p is None for p, _, _, _ in got["rows"][1])
    check_against_decoder(Q4, parts, got, skip=(1,))


def test_errors():
    import vorbis_amd
    parts = streams(Q4, (0.1,), 81)
    plain = feed_of(Q4, parts, decoded=False)
    try:
        slot = wrote(plain, parts)
        with pytest.raises(vorbis_amd.VamdError) as e:
            plain.decoded(slot)
        assert e.value.code == EINVAL and "VAMD_FEED_DECODED" in plain.L.vamd_feed_last_error(plain.h).decode()
        plain.packets(slot)
        plain.release(slot)
    finally:
        plain.close()
    feed = feed_of(Q4, parts)
    try:
        slot, _ = feed.buffer(2)
        with pytest.raises(vorbis_amd.VamdError) as e:
            feed.decoded(slot)  # nothing was written: as packets() treats it
        assert e.value.code == EINVAL
        feed.release(slot)
    finally:
        feed.close()
    managed = ref.RefEncoder(2, 44100, managed=(-1, 128000, -1)).pack_setup()
    for blob, kw, word in ((managed, dict(), "bitrate-managed"), (ref_host.encoder(Q4).pack_setup(), dict(write_frames=1024), "live")):
        with pytest.raises(vorbis_amd.VamdError) as e:
            vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=4096, fmt=vorbis_amd.FEED_F32, decoded=True, **kw)
        assert e.value.code == EIMPL and word in str(e.value) and "VAMD_FEED_DECODED" in str(e.value), e.value
