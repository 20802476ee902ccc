"""The checks and drivers several test modules (and the tools) share: what a feed's packets, files and decoded signal are
held against, and the few lines that drive a feed or pick a checker."""
import os
import re

import numpy as np

from tests import checker
from tests import ogg_framing as fr
from tests import ref_host

LIB = os.path.join(checker.ROOT, "vorbis_amd", "libvorbis_amd.so")
# VAMD_ABI_VERSION of the header: what a caller compiled against it hands vamd_create() (the macro does it for C callers)
ABI = int(re.search(r"#define VAMD_ABI_VERSION (\d+)", open(os.path.join(checker.ROOT, "include", "vorbis_amd.h")).read()).group(1))
Q4 = "44k_stereo_q4"
FLOOR_KEYS = ("mdct", "logmask", "post_valid", "nonzero", "iwork")  # (+ posts: compare_block takes them when both sides have them)
FLOOR_WANT = FLOOR_KEYS + ("posts",)
MANAGED_KEYS = ("m_post_valid", "m_iwork", "m_nonzero", "m_posts")


# ---- comparisons ----
def planar(x):
    """[frames, ch] as an application holds it (16-bit or float) -> float32 [ch, frames] as the reference's loop reads it"""
    return np.ascontiguousarray((x.astype(np.float32) / np.float32(32768.0)).T if x.dtype == np.int16 else x.T)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def diff(want, got, s=0):
    if len(want) != len(got):
        return ["stream %d: %d packets, the reference %d" % (s, len(got), len(want))]
    for k, (w, g) in enumerate(zip(want, got)):
        if w != tuple(g):
            return ["stream %d packet %d/%d: bytes %s granulepos %d/%d W %d/%d eos %d/%d" % (
                s, k, len(want), "equal" if w[0] == g[0] else "DIFFER", g[1], w[1], g[2], w[2], g[3], w[3])]
    return []


def managed_same(a, b):
    """-> the first of MANAGED_KEYS in which two managed taps differ, or None"""
    for k in MANAGED_KEYS:
        x, y = a[k], b[k]
        if k == "m_posts":  # reference rows are 65 wide, ours 32; only `posts` entries are meaningful
            x, y = x[:, :, :29], y[:, :, :29]
        if not np.array_equal(x, y):
            return k
    return None


def check_state(st, want, ch):
    """EnvelopeState (history form) against the reference's rings (already rolled oldest-first)."""
    def bits(a):
        return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert st.stretch == want["stretch"]
    amp = np.array(st.amp_hist, np.float32).reshape(8, 16, 8)[:ch]
    near = np.array(st.near_hist, np.float32).reshape(8, 30)[:ch]
    # reference keeps 17 amplitudes / 15 near-DC terms; the histories keep 16 / 30
    assert np.array_equal(bits(amp[:, :, :7].transpose(0, 2, 1)), bits(want["amp"][:, :, 1:]))
    assert np.array_equal(bits(near[:, 15:]), bits(want["near"]))


# ---- the reference's application loop ----
def reference_packets(setup, pcm_s16):
    """The reference's application loop over one stream's samples [frames, ch] int16."""
    from oracle import ref
    ch, rate, q = checker.SETUPS[setup]
    return ref.RefEncoder(ch, rate, q).encode_stream(planar(pcm_s16))


def reference_records(ref, ch, q, x, managed=None):
    return ref.RefEncoder(ch, 44100, q, managed=managed).encode_stream(planar(x))


def records(enc, x):
    """the reference's application loop over one stream, written 1024 frames at a time"""
    return enc.encode_stream(planar(x), write_frames=1024)


def record_rows(enc, x, write_frames=1024):
    """records() as the rows a feed returns: (bytes, granulepos, W, e_o_s) per packet"""
    return [(w["packet"], w["granulepos"], w["W"], w["eos"]) for w in enc.encode_stream(planar(x), write_frames=write_frames)]


# ---- files ----
def check_file(host, headers, want, rows, f, frames, serial, npages):
    """want: the reference's records of the stream; rows: the feed's packet records of it; f: its file"""
    pages, got = fr.demux(f)                                 # (asserts every CRC and the continued flags)
    assert got[:3] == list(headers)
    assert got[3:] == [w["packet"] for w in want], "the file's packets are not the reference's"
    assert got[3:] == [r[0] for r in rows], "the file's packets are not the ones vamd_feed_packets reports"
    assert [r[1] for r in rows] == [w["granulepos"] for w in want]
    assert f == host.mux(headers, [r[0] for r in rows], [r[1] for r in rows], serial), "the device's pages are not the host mux's"
    assert len(pages) == npages
    assert pages[0]["bytes"] == 58 and pages[0]["flags"] == 2 and pages[0]["granule"] == 0
    assert all(p["serial"] == serial for p in pages)
    fr.check_policy(pages, next(i for i, p in enumerate(pages) if sum(q["done"] for q in pages[:i + 1]) == 3) + 1)
    assert pages[-1]["flags"] & 4 and pages[-1]["granule"] == frames
    dec = ref_host.reference_decode(got, fr.page_granules(pages, len(want)))
    assert dec.shape[1] == frames, "the reference decoder returns %d frames of %d" % (dec.shape[1], frames)
    return pages


def whole_file(groups):
    """a stream's pieces laid end to end; every piece a whole number of pages (their checksums verified), as many as npages says"""
    for g in groups:
        assert len(fr.pages_of(g["bytes"])) == g["npages"]
    return b"".join(g["bytes"] for g in groups)


def rows_of(groups):
    return [r for g in groups for r in g["rows"]]


# ---- driving a feed ----
def small_arena(monkeypatch, arena):
    """arena (a string, or None): VAMD_FEED_OUT_BYTES (a test knob) -- every lane's packet arena starts that small, so a
    group whose packets take more has to grow it (the VBR retry, the growth between a managed group's slices, the Ogg
    mirror's)."""
    if arena:
        monkeypatch.setenv("VAMD_TEST_KNOBS", "1")
        monkeypatch.setenv("VAMD_FEED_OUT_BYTES", arena)


def spy_totals(feed):
    """-> a list that receives total_bytes of every group feed.packets() returns from now on"""
    totals, packets = [], feed.packets

    def spy(slot, copy=True):
        r = packets(slot, copy)
        totals.append(r["total_bytes"])
        return r
    feed.packets = spy
    return totals


def run_live(feed, streams, cuts):
    """Feed streams [frames_s, ch] to a one-lane live feed in rounds: in round r stream s gets cuts[s][r] frames and is closed
    with its last piece (a stream whose cuts ran out gets nothing).  -> per stream its packets over all rounds."""
    got = [[] for _ in streams]
    pos = [0] * len(streams)
    for r in range(max(len(c) for c in cuts)):
        pieces, close = [], []
        for s, x in enumerate(streams):
            n = cuts[s][r] if r < len(cuts[s]) else 0
            pieces.append(x[pos[s]:pos[s] + n])
            pos[s] += n
            close.append(r == len(cuts[s]) - 1)
        for s, row in enumerate(feed.encode_live(pieces, close)):
            got[s] += row
    assert pos == [len(x) for x in streams]
    return got


def decoded_feed_of(name, parts, **kw):
    """a float-fed feed of the setup's own blob that hands the decoded signal back (decoded=False: one that does not)"""
    import vorbis_amd
    kw.setdefault("lanes_per_device", 1)
    kw.setdefault("decoded", True)
    return vorbis_amd.Feed(ref_host.encoder(name).pack_setup(), max_streams=len(parts), max_frames=max(len(p) for p in parts),
                           fmt=vorbis_amd.FEED_F32, **kw)


# ---- the block checker of any shipped setup ----
_checkers = {}


class SurroundChecker:
    """checker.Checker for the setups it has no entry for (checker.SURROUND): the reference where it is built, else the port."""

    def __init__(self, name):
        from oracle import port, ref
        ch, rate, q = checker.SURROUND[name]
        if ref.available():
            self.enc, self.kind = ref.RefEncoder(ch, rate, q), "reference"
        else:
            blob = np.fromfile(os.path.join(checker.ROOT, "vorbis_amd", "data", "setup_%s.bin" % name), dtype=np.uint8)
            self.enc, self.kind = port.PortEncoder(blob), "port"

    def tap_block(self, pcm, lW=1, W=1, nW=1, blocktype=1, ampmax_in=-9999.0):
        return self.enc.tap_block(pcm, lW, W, nW, blocktype, ampmax_in)


def chk_for(name):
    if name not in _checkers:
        _checkers[name] = checker.Checker(name) if name in checker.SETUPS else SurroundChecker(name)
    return _checkers[name]


def channels(name):
    return (checker.SETUPS.get(name) or checker.SURROUND[name])[0]
