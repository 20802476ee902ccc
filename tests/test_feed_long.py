"""GPU suite: whole streams of any length.  The stream walk (k_plan_streams) reads its marks through a sliding window in LDS
(MarkWindow, k_blockout.h), so a whole-stream feed no longer refuses a stream whose marks do not fit a workgroup's LDS.
With the test knob VAMD_PLAN_WINDOW the window is a few dozen marks and slides hundreds of times over streams of a few tens
of thousands of frames: packets, plans and managed groups must be what the default window gives and what the reference's
application loop emits.  Without any knob, an 11 M-frame stream -- past the 10.48 M frames the walk's LDS used to hold --
goes through a whole-stream Ogg feed and comes back as the reference's packets in the host mux's file."""
import functools

import numpy as np
import pytest

from tests import bitrate_host as bh
from tests import checker
from tests import ogg_host as oh
from tests import plan_window_host as pwh
from tests import ref_host as rh
from tests.feed_cases import diff, planar, record_rows as records
from tests.signals import s16_streams

pytestmark = pytest.mark.gpu

LENGTHS = [90000, 40000, 12345, 700, 1]
KINDS = ["gated", "clicks", "noise", "sine", "noise"]
PRIME = 367  # a window a few hundred marks above the minimum, and no multiple of anything the walk steps by


def _ref():
    from oracle import ref
    if not ref.available():
        pytest.skip("needs the reference build")
    return ref


@functools.lru_cache(maxsize=None)
def minimum():
    """plan_window_min of the shipped setups' block sizes, from the shipped header"""
    return pwh.PlanWindow(pwh.build(), (256, 2048)).minimum


def window_of(which):
    lo = minimum()
    assert lo + 200 < PRIME < lo + 400
    return {"minimum": lo, "prime": PRIME}[which]


@functools.lru_cache(maxsize=None)
def group(setup):
    """-> (the streams, the reference's records of each, the feed's rows with the default window); made once per setup"""
    ref = _ref()
    ch, rate, q = checker.SETUPS[setup]
    rng = np.random.default_rng(14)
    parts = [s16_streams(rng, ch, n, [k])[0] for n, k in zip(LENGTHS, KINDS)]
    want = [records(ref.RefEncoder(ch, rate, q), x) for x in parts]
    return parts, want, feed_rows(setup, parts)


def feed_rows(setup, parts):
    import vorbis_amd
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob(setup), lanes_per_device=1, max_streams=8, max_frames=max(LENGTHS))
    try:
        return feed.encode(parts)
    finally:
        feed.close()


def set_window(monkeypatch, marks):
    monkeypatch.setenv("VAMD_TEST_KNOBS", "1")
    monkeypatch.setenv("VAMD_PLAN_WINDOW", str(marks))


@pytest.mark.parametrize("which", ["minimum", "prime"])
@pytest.mark.parametrize("setup", ["44k_stereo_q4", "44k_mono_q5"])
def test_small_window_against_the_reference(setup, which, monkeypatch):
    """Five streams of 90 000 to 1 frames in one vamd_feed_wrote_v group, the window refilled every `window` marks
    (90 000 frames: some 1400 marks)."""
    import vorbis_amd
    parts, want, default = group(setup)
    marks = window_of(which)
    set_window(monkeypatch, marks)
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(setup), 0)
    assert "VAMD_PLAN_WINDOW=%d" % marks in an.config_string().split()
    got = feed_rows(setup, parts)
    assert len(got[0]) > 60 and got[-1][-1][3] == 1
    bad = []
    for s in range(len(parts)):
        bad += diff(want[s], got[s], s)
        assert [tuple(g) for g in got[s]] == [tuple(g) for g in default[s]], "stream %d: the window shows" % s
    assert not bad, "\n".join(bad)


def test_a_knob_without_the_test_switch_is_ignored(monkeypatch):
    import vorbis_amd
    monkeypatch.delenv("VAMD_TEST_KNOBS", raising=False)
    monkeypatch.setenv("VAMD_PLAN_WINDOW", "100")
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob("44k_stereo_q4"), 0)
    assert "VAMD_PLAN_WINDOW" not in an.config_string()


def test_plan_streams_not_whole(monkeypatch):
    """vamd_plan_streams (streams that go on: no ends, no padding) shares the walk: four stereo streams of 60 000 samples,
    one silent, planned with the minimum window, the prime one and the default -- the same plan."""
    import torch
    import vorbis_amd
    rng = np.random.default_rng(60)
    n = 60000
    x = np.stack([planar(s16_streams(rng, 2, n, [k])[0]) for k in ("gated", "clicks", "silence", "noise")])

    def lists():
        an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob("44k_stereo_q4"), 0)
        plan, _ = an.plan_streams(torch.from_numpy(x).cuda())
        L = an.plan_lists(plan)
        torch.cuda.synchronize()
        return L
    default = lists()
    assert all(len(default["lW"][W]) > 50 for W in (0, 1))
    assert np.all(np.diff(default["stream_start"]) > 20)
    for which in ("minimum", "prime"):
        set_window(monkeypatch, window_of(which))
        got = lists()
        assert np.array_equal(got["order"], default["order"]) and np.array_equal(got["stream_start"], default["stream_start"]), which
        for k in ("lW", "nW", "blocktype", "src"):
            for W in (0, 1):
                assert np.array_equal(got[k][W], default[k][W]), (which, k, W)


def test_managed_group_with_a_small_window(monkeypatch):
    """A bitrate-managed (ABR) group of 26 000 and 9 000 frames: the slices of a managed group and the walk's window are
    independent of each other."""
    import vorbis_amd
    ref = _ref()
    name, ch, rates, kind = bh.CONFIGS[0]
    lengths = [26000, 9000]
    parts = [np.clip(np.round(bh.signal(kind, ch, n, 70 + i).T * 32768.0), -32768, 32767).astype(np.int16) for i, n in enumerate(lengths)]
    set_window(monkeypatch, window_of("minimum"))
    feed = vorbis_amd.Feed(bh.managed_blob(ch, rates), lanes_per_device=1, max_streams=2, max_frames=max(lengths))
    try:
        got = feed.encode(parts)
    finally:
        feed.close()
    bad = []
    for s, x in enumerate(parts):
        bad += diff(records(ref.RefEncoder(ch, 44100, managed=rates), x), got[s], s)
    assert not bad, "\n".join(bad)


def test_past_the_old_cap_ogg_file():
    """A mono 44.1 kHz stream of 11 M frames (about 250 s; its 171 875 marks are past the 163 836 a workgroup's LDS held)
    through a whole-stream Ogg feed, no knobs: the reference's packets, in the file the host mux makes of them.  (The
    reference's own encode of 250 s takes most of the time.)"""
    import vorbis_amd
    ref = _ref()
    frames, serial = 11_000_000, 0x14c0ffee
    rng = np.random.default_rng(250)
    t = np.arange(frames)
    x = (rng.random(frames) - 0.5) * np.where((t % 44100) < 9000, 0.6, 0.01) + 0.3 * np.sin(2 * np.pi * 220.0 / 44100.0 * t)
    x = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)[:, None]
    del t
    ch, rate, q = checker.SETUPS["44k_mono_q5"]
    headers = rh.reference_headers(ch, rate, q)
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob("44k_mono_q5"), lanes_per_device=1, max_streams=1, max_frames=frames,
                           ogg_headers=headers)
    try:
        slot, buf = feed.buffer(ch)
        buf[:frames] = x.reshape(-1)
        feed.ogg_serials(slot, [serial])
        feed.wrote(slot, 1, frames)
        o = feed.ogg(slot)
        rows = feed._rows(feed.packets(slot), 1)[0]
        feed.release(slot)
    finally:
        feed.close()
    assert o["status"][0] == 0
    f = bytes(o["bytes"][int(o["stream_offset"][0]):int(o["stream_offset"][1])])
    want = records(ref.RefEncoder(ch, rate, q), x)
    bad = diff(want, rows)
    assert not bad, "\n".join(bad)
    assert len(rows) > 10_000 and rows[-1][3] == 1 and rows[-1][1] == frames
    host = oh.HostOgg()
    assert f == host.mux(headers, [r[0] for r in rows], [r[1] for r in rows], serial), "the file is not the host mux's of these packets"
