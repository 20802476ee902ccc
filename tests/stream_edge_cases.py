"""The case table of the stream-end tests (tests/test_stream_ends_cpu.py, tests/test_stream_ends_gpu.py): whole float streams
at the edges of the input domain, the setups they run on, the lengths either side of every line the reference draws when
it extrapolates a stream's two ends (lib/block.c:417-458, :474-512), the reference's records of them (computed once per
process) and where a block's samples lie: in the extrapolated head room, among the real samples, or in the extrapolated
tail.  Everything is deterministic in its arguments; nothing here is a test."""
import zlib

import numpy as np

# name -> (channels, rate, quality, (blocksizes[0], blocksizes[1])); the block sizes are the reference's (asserted by
# the CPU module): 512/4096 has the largest head span and a 12 288-sample tail, 512/512 one size class, 44k_51_q3 six
# channels (nstreams * ch waves in the two extrapolation kernels)
SETUPS = {
    "44k_stereo_q4": (2, 44100, 0.4, (256, 2048)),
    "44k_stereo_qm1": (2, 44100, -0.1, (512, 4096)),
    "8k_mono_q3": (1, 8000, 0.3, (512, 512)),
    "22k_stereo_q4": (2, 22050, 0.4, (512, 1024)),
    "44k_51_q3": (6, 44100, 0.3, (256, 2048)),
}
# two to three long blocks past n_head
FULL_FRAMES = {2048: 9000, 4096: 11000, 1024: 6001, 512: 5000}
WRITE_FRAMES = 1024  # the example's cadence: what the feed reproduces (lib/block.c:524-528 runs after such a write)

NOISE_AMPS = ("1e-7", "3e-7", "1e-6", "3e-6", "1e-5", "1e-4", "0.4")  # around Levinson-Durbin's `error < epsilon` (3e-7 .. 1e-6)
KINDS = tuple("noise_" + a for a in NOISE_AMPS) + (
    "denormal_noise", "signed_zeros", "gated_over_40dB", "steady_over_50dB", "impulses_on_denormals", "dc", "dc_ramp",
    "sine_period_64", "square_period_100", "quiet_burst_at_end", "quiet_burst_at_start", "last_sample_only", "antiphase",
    "silent_channel", "floor_at_both_ends")
LENGTH_KINDS = ("noise_0.4", "sine_period_64")  # these also run at edge_lengths()
TINY = (1e-45, -1e-45, 3e-39, -1.2e-38, 1e-30)  # single denormals / tiny normals among signed zeros
FLT_MIN = np.float32(1.17549435e-38)


def n_head(bs1, write_frames=WRITE_FRAMES):
    """how many of a stream's first samples the backward extrapolation sees when they arrive write_frames at a time"""
    return (bs1 // write_frames + 1) * write_frames


def edge_lengths(bs1):
    """stream lengths either side of: order * 2 = 32 (head) and 64 (tail) samples, half a long block, a long block, n_head"""
    nh = n_head(bs1)
    return sorted(set([1, 31, 32, 33, 64, 65, 100, bs1 // 2 - 1, bs1 // 2 + 1, bs1 - 1, bs1 + 1, nh - 1, nh, nh + 1]))


def _noise(rng, ch, frames, amp):
    return (rng.random((ch, frames)) - 0.5) * 2 * amp


def signal(kind, ch, frames, bs1):
    """-> float32 [ch, frames]"""
    rng = np.random.default_rng(zlib.crc32(("%s/%d/%d/%d" % (kind, ch, frames, bs1)).encode()))
    t = np.arange(frames)
    if kind.startswith("noise_"):
        x = _noise(rng, ch, frames, float(kind[6:]))
    elif kind == "denormal_noise":
        x = _noise(rng, ch, frames, 1e-40)
    elif kind == "signed_zeros":
        x = np.where(rng.random((ch, frames)) < 0.5, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
        nh = n_head(bs1)
        for i, p in enumerate((5, nh - 1, nh, frames - 40, frames - 1)):
            if 0 <= p < frames:
                x[i % ch, p] = np.float32(TINY[i])
    elif kind == "gated_over_40dB":
        x = _noise(rng, ch, frames, 1.0) * np.where((t % 3000) < 300, 100.0, 0.05)
    elif kind == "steady_over_50dB":
        x = _noise(rng, ch, frames, 316.0)
    elif kind == "impulses_on_denormals":
        x = (rng.random((ch, frames)) - 0.5) * 1e-39
        x[:, 700::1777] = 2e4 * np.where(rng.random((ch, len(t[700::1777]))) < 0.5, -1.0, 1.0)
    elif kind == "dc":
        x = np.full((ch, frames), 0.25)
    elif kind == "dc_ramp":  # opposite slopes per channel
        x = 0.1 + 0.4 * np.linspace(-1, 1, frames)[None, :] * np.where(np.arange(ch) & 1, -1.0, 1.0)[:, None]
    elif kind == "sine_period_64":  # one period tiled: exactly periodic in float32
        one = (0.5 * np.sin(2 * np.pi * np.arange(64) / 64.0)).astype(np.float32)
        x = np.tile(one, frames // 64 + 1)[None, :frames] * np.ones((ch, 1), np.float32)
    elif kind == "square_period_100":
        x = np.where((t % 100) < 50, 1.0, -1.0)[None, :] * np.ones((ch, 1))
    elif kind == "quiet_burst_at_end":
        x = _noise(rng, ch, frames, 1e-4)
        x[:, max(0, frames - 200):] = _noise(rng, ch, min(200, frames), 0.8)
    elif kind == "quiet_burst_at_start":
        x = _noise(rng, ch, frames, 1e-4)
        x[:, :150] = _noise(rng, ch, min(150, frames), 0.8)
    elif kind == "last_sample_only":
        x = np.zeros((ch, frames))
        x[0, frames - 1] = 0.5
    elif kind == "antiphase":
        x = _noise(rng, 1, frames, 0.4) * np.where(np.arange(ch) & 1, -1.0, 1.0)[:, None]
    elif kind == "silent_channel":
        x = _noise(rng, ch, frames, 0.4)
        x[ch - 1] = 0
    elif kind == "floor_at_both_ends":
        # noise whose first and last 48 frames lie at 1e-35: the fits see the noise, the predictors start from the floor, so
        # their outputs are denormal within the 256 samples of head room and tail that a 512-sample block shows
        x = _noise(rng, ch, frames, 0.4)
        x[:, :48] = _noise(rng, ch, min(48, frames), 1e-35)
        x[:, max(0, frames - 48):] = _noise(rng, ch, min(48, frames), 1e-35)
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(x, dtype=np.float32)


def case_list(setup):
    """-> [(kind, frames)]: every kind at the full length first, then LENGTH_KINDS at the edge lengths"""
    bs1 = SETUPS[setup][3][1]
    return [(k, FULL_FRAMES[bs1]) for k in KINDS] + [(k, n) for k in LENGTH_KINDS for n in edge_lengths(bs1)]


def full_cases(setup):
    """the indices into case_list() of the full-length kinds"""
    return list(range(len(KINDS)))


def case_id(setup, i):
    return "%s[%d]" % case_list(setup)[i]


_SIGNALS, _RECORDS = {}, {}


def signals(setup):
    """-> the float32 [ch, frames] arrays of case_list(setup); made once, to be left unchanged"""
    if setup not in _SIGNALS:
        ch, _, _, bs = SETUPS[setup]
        _SIGNALS[setup] = [signal(k, ch, n, bs[1]) for k, n in case_list(setup)]
        for x in _SIGNALS[setup]:
            x.setflags(write=False)
    return _SIGNALS[setup]


def encoder(setup):
    from oracle import ref
    ch, rate, q, _ = SETUPS[setup]
    return ref.RefEncoder(ch, rate, q)


def records(setup):
    """-> per case the reference's application loop over it (oracle/ref.py: encode_stream, 1024 frames per write, errors
    recorded, not raised); computed once per process, to be left unchanged"""
    if setup not in _RECORDS:
        _RECORDS[setup] = [encoder(setup).encode_stream(x, write_frames=WRITE_FRAMES, tolerate=True) for x in signals(setup)]
    return _RECORDS[setup]


def rows_of(recs):
    """records as the rows a feed returns"""
    return [(w["packet"], w["granulepos"], w["W"], w["eos"]) for w in recs]


def begins_of(recs, bs):
    """where every block of a stream begins in the stream's buffer [bs[1]/2 of head room | frames | tail], from the
    reference's block sizes alone: the first block is centred at bs[1]/2, a block's centre lies a quarter of its size and
    a quarter of its successor's behind it (lib/block.c:566-571, :682-683)"""
    out, centre = [], bs[1] // 2
    for k, b in enumerate(recs):
        n = bs[b["W"]]
        if k:
            centre += bs[recs[k - 1]["W"]] // 4 + n // 4
        out.append(centre - n // 2)
    return out


def regions(begin, n, frames, bs1):
    """-> (head, tail): slices of a block's n samples that lie in the extrapolated head room / behind the last real sample"""
    head, eof = bs1 // 2, bs1 // 2 + frames
    return slice(0, max(0, min(n, head - begin))), slice(max(0, min(n, eof - begin)), n)


def is_denormal(a):
    a = np.abs(a)
    return (a > 0) & (a < FLT_MIN)


def where_of(begin, i, frames, bs1):
    """sample i of a block that begins at `begin` -> ("head room" | "real samples" | "tail", its index there)"""
    p, head = begin + i, bs1 // 2
    if p < head:
        return "head room", p
    if p < head + frames:
        return "real samples", p - head
    return "tail", p - head - frames
