"""The signals several test modules (and the tools) share, and the tables of cuts and packet sizes they are run over.
Everything is deterministic in its arguments."""
import numpy as np

from tests import bitrate_host as bh
from tests import checker

N_HEAD = 3072  # (2048 / 1024 + 1) * 1024: where the example's cadence runs the backward extrapolation
MANAGED_RATES = (-1, 128000, -1)  # the setup tests/test_feed_decoded.py::test_errors builds: ABR 128 kb/s


# ---- 16-bit streams [frames, ch], as an application hands them to the feed ----
def s16_streams(rng, ch, frames, kinds):
    out = []
    t = np.arange(frames)
    for kind in kinds:
        if kind == "noise":
            x = (rng.random((frames, ch)) - 0.5) * 0.8
        elif kind == "gated":
            gate = np.where((t % 9000) < 700, 0.5, 0.0005)[:, None]
            x = (rng.random((frames, ch)) - 0.5) * 2 * gate
        elif kind == "sine":
            x = 0.6 * np.sin(2 * np.pi * 440.0 / 44100.0 * t)[:, None] * np.ones((1, ch)) + (rng.random((frames, ch)) - 0.5) * 1e-3
        elif kind == "clicks":
            x = (rng.random((frames, ch)) - 0.5) * 0.002
            x[::4001] = 0.9
        elif kind == "silence":
            x = np.zeros((frames, ch))
        else:
            raise ValueError(kind)
        out.append(np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16))
    return np.stack(out)


def random_cuts(rng, frames, special=()):
    """piece lengths summing to `frames`: random cut points (and those in `special`), a few empty pieces in between"""
    points = set(int(p) for p in special if 0 < p < frames)
    for _ in range(frames // 5000 + 3):
        if frames > 1:
            points.add(int(rng.integers(1, frames)))
    edges = [0] + sorted(points) + [frames]
    cuts = [b - a for a, b in zip(edges, edges[1:])]
    for k in sorted(rng.choice(len(cuts), size=min(3, len(cuts)), replace=False))[::-1]:
        cuts.insert(int(k), 0)
    return cuts


def mixed_streams(rng, ch):
    """the cases of a live lane: long streams cut at random (one piece ending exactly at n_head, 1-frame pieces), a stream
    shorter than n_head, a 1-frame stream, a stream opened and closed in one piece, a close on an empty piece"""
    lengths = [31000, 24000, 2500, 1, 9000, 17000]
    kinds = ["gated", "noise", "sine", "noise", "clicks", "gated"]
    streams = [s16_streams(rng, ch, n, [k])[0] for n, k in zip(lengths, kinds)]
    cuts = [random_cuts(rng, 31000, [N_HEAD, N_HEAD + 1]),
            [1, 1, 1000, 1, 0] + random_cuts(rng, 22997, [N_HEAD - 1003]),
            [100, 2400],
            [1],
            [0, 0, 9000],
            random_cuts(rng, 17000) + [0]]
    return streams, cuts


def managed_s16_streams(lengths, kind="music"):
    """the bitrate manager's signals (tests/bitrate_host.py) as 16-bit stereo streams"""
    return [np.clip(np.round(bh.signal(kind, 2, n, 40 + i).T * 32768.0), -32768, 32767).astype(np.int16) for i, n in enumerate(lengths)]


# ---- float streams ----
def gated_noise(ch, rate, frames, seed):
    """[ch, frames]: bursts, so that the detector switches (tests/test_rates.py::test_hybrid_encode)"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)
    x = (rng.random((ch, frames), dtype=np.float32) - 0.5) * 2 * np.where((t % (rate // 4)) < rate // 40, 0.5, 0.0005)
    return np.ascontiguousarray(x, dtype=np.float32)


def gated_streams(name, seconds, seed):
    """gated noise, one [frames, ch] float32 array per stream"""
    ch, rate, _, _ = checker.ENCODERS[name]
    return [np.ascontiguousarray(gated_noise(ch, rate, int(rate * sec) + 7 * i + 1, seed + i).T) for i, sec in enumerate(seconds)]


def managed_streams(seconds=(0.3, 0.7, 1.1, 1.5), seed=11):
    """-> (setup blob, headers, per stream (packets, granules)) of the reference's managed encoder over the gated-noise
    streams of tests/test_feed_decoded.py"""
    from oracle import ref
    from tests import ref_host
    out = []
    for i, sec in enumerate(seconds):
        enc = ref.RefEncoder(2, 44100, managed=MANAGED_RATES)
        recs = enc.encode_stream(gated_noise(2, 44100, int(44100 * sec) + 7 * i + 1, seed + i))
        out.append(([r["packet"] for r in recs], [r["granulepos"] for r in recs]))
    enc = ref.RefEncoder(2, 44100, managed=MANAGED_RATES)
    return enc.pack_setup(), ref_host.encoder_headers(ref.RefEncoder(2, 44100, managed=MANAGED_RATES)), out


def gated(ch, frames, seed, period=5000, on=700):
    """[ch, frames]: the detector tests' bursts"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)
    g = np.where((t % period) < on, 0.6, 0.004).astype(np.float32)
    return ((rng.random((ch, frames), dtype=np.float32) - 0.5) * 2 * g).astype(np.float32)


def dropin_stream(ch, seconds, kind, seed):
    """[ch, frames] at 44.1 kHz: what the drop-in tests write into the application loop"""
    rng = np.random.default_rng(seed)
    frames = int(44100 * seconds)
    x = (rng.random((ch, frames), dtype=np.float32) - 0.5)
    if kind == "gated":   # transients -> short blocks, transitions (SURVEY.md 8d "C5")
        t = np.arange(frames)
        x *= 2 * np.where((t % 11025) < 1102, 0.5, 0.0005).astype(np.float32)
    elif kind == "s16":   # encoder_example.c:197-202: s16 samples / 32768
        x = np.round(x * 32767).astype(np.int16).astype(np.float32) / 32768.0
    return np.ascontiguousarray(x, dtype=np.float32)


# ---- packet sizes and cuts for the Ogg host's tests ----
HB = [30, 89, 4140]

# size lists no real encoder gives, for the whole-file walk and mux
WHOLE_SIZE_LISTS = {
    "empty_packets": [0, 0, 0],
    "one": [1],
    "254": [254],
    "255": [255],
    "256": [256],
    "510": [510],
    "65025": [65025],
    "70000": [70000],
    "70000_then_small": [70000, 10, 20, 5000, 30, 40, 50],
    "300_one_byte": [1] * 300,
    "254_one_byte_then_300": [1] * 254 + [300],
    "fill_rule": [1500, 1500, 1500, 1500, 1500, 10, 10, 10, 10, 5000, 10],
    "three_big": [3000, 3000, 3000],
    "mixed": [0, 255, 1, 510, 0, 4097, 2, 2, 2, 2, 2, 765, 0],
}


def _live_size_lists():
    rng = np.random.default_rng(17)
    return {
        "random": [int(v) for v in rng.integers(0, 1201, 70)] + [5000, 3, 4100, 2],
        "400_one_byte": [1] * 400,
        "multiples_of_255": [int(v) for v in rng.choice([0, 255, 510, 765, 1020], 60)],
        "70000_among_small": [10, 20, 70000, 30, 5000, 40, 50, 60],
        "254_one_byte_then_2000": [1] * 254 + [2000] * 6,
    }


LIVE_SIZE_LISTS = _live_size_lists()  # for the mux in pieces


def cuts_of(name, n, rng):
    """-> lists of group sizes (packets per group; the last group closes the stream)"""
    out = [[i, n - i] for i in range(n + 1)]                       # after every packet index in turn
    out.append([1] * n)                                             # single packets
    for _ in range(6):                                              # random cuts with empty groups, a close on an empty group
        points = sorted(int(v) for v in rng.integers(0, n + 1, int(rng.integers(1, 9))))
        edges = [0] + points + [n]
        groups = [b - a for a, b in zip(edges, edges[1:])]
        groups.insert(int(rng.integers(0, len(groups) + 1)), 0)
        out.append(groups + [0])
    return out


def sized_comment(nbytes, title, vendor="vorbis_amd tests"):
    """A comment header of exactly nbytes: a TITLE and a PAD tag that takes up the rest (printable, so that
    vorbis_comment_query hands it back whole).  -> (packet, tags)"""
    import vorbis_amd
    base = len(vorbis_amd.comment_packet([("TITLE", title), ("PAD", "")], vendor))
    assert nbytes >= base, (nbytes, base)
    rng = np.random.default_rng(nbytes)
    pad = bytes(rng.integers(0x30, 0x7b, nbytes - base, dtype=np.uint8)).decode("ascii")
    tags = [("TITLE", title), ("PAD", pad)]
    packet = vorbis_amd.comment_packet(tags, vendor)
    assert len(packet) == nbytes
    return packet, tags
