"""Mutated streams for the packet decoder's tests (tests/test_unpack_cpu.py on the one-lane host build,
tests/test_decode_gpu.py on the GPU): packets no encoder wrote -- posts outside their range, phrase words and classes no
real block uses, codewords from the far end of a book, a packet that stops being read long before it ends -- each
classified BY THE REFERENCE ALONE, so that what the decoder is held to does not come from the decoder.

Per setup four base streams of the reference encoder over gated noise; case s is base stream s % 4 with exactly one
packet replaced, the kind of mutation cycling over
  0  one bit flipped anywhere in the packet,
  1  one bit flipped inside the first 12 bytes (the head and the floors),
  2  every byte from a random position >= 1 to the end replaced by random bytes
(the mode bits are not spared; the last case mutates the last packet of its stream, so that a group's final bytes are a
mutated packet).  The mutated packet's class, from vorbis_synthesis() on it alone (ref_host.BlockDecoder.synthesis):
  notaudio  it returns nonzero;
  complete  the packet alone and the packet followed by 16 more bytes -- of 0x00, of 0xff, and of the other fills of
            PADS -- give the same vb->pcm bits: the reference never needed a bit beyond the packet's end;
  ranout    anything else (libvorbis stops working where the packet ends; the decoder flags the packet: k_unpack.h).

Everything is deterministic in (setup, cases, seed) and computed once per process."""
import numpy as np

from tests import ref_host
from tests.feed_cases import same_bits
from tests.signals import gated_noise
from tests.synth_host import SETUPS, SHORT_LENGTHS
from tests.unpack_host import STATUS_BADCODE, STATUS_NOTAUDIO, STATUS_TRUNCATED

KINDS = ("flip", "flip_head", "random_tail")
CLASSES = ("complete", "ranout", "notaudio")
HEAD_BYTES, PAD = 12, 16
# what follows the packet when the reference is asked whether it needs more: zeros and ones -- and, because both are
# codewords of "nothing coded here" in some phrase books (a short packet turned long by its mode bit came out of 0x00 and
# 0xff as it came out of no padding at all, and of 0x55 otherwise: 2 of 768 cases), two alternating and two random fills
PADS = tuple(bytes([v]) * PAD for v in (0x00, 0xff, 0x55, 0xaa)) + tuple(
    np.random.default_rng(v).integers(0, 256, PAD, dtype=np.uint8).tobytes() for v in (16, 17))
_groups, _bases = {}, {}


def base_frames(name, v):
    """some 20 packets: at 44.1 kHz 9000 + 100 v frames (19 or 20 packets of 256 / 2048, 11 of 512 / 4096), both block
    sizes among them; the 8 kHz setup has one block size, 512, and 5000 + 100 v frames are 21 packets of it"""
    rate = SETUPS[name][1]
    return (9000 if rate >= 44100 else 5000) + 100 * v


def base_streams(name, seed):
    """-> (setup blob, headers, block sizes, [(packets, end granule)] x 4)"""
    if (name, seed) not in _bases:
        enc = ref_host.encoder(name)
        out, Ws = [], set()
        for v in range(4):
            e = ref_host.encoder(name)
            recs = e.encode_stream(gated_noise(e.channels, e.rate, base_frames(name, v), 1000 * seed + v))
            out.append(([r["packet"] for r in recs], recs[-1]["granulepos"]))
            Ws |= {r["W"] for r in recs}
            assert recs[-1]["granulepos"] == base_frames(name, v) and len(recs) >= 8
        bs = (enc.blocksize(0), enc.blocksize(1))
        assert bs[0] == bs[1] or Ws == {0, 1}, (name, Ws)  # a setup with two block sizes: both are in the base streams
        _bases[name, seed] = (enc.pack_setup(), ref_host.encoder_headers(ref_host.encoder(name)), bs, out)
    return _bases[name, seed]


def mutate(packet, kind, rng):
    p = bytearray(packet)
    if kind == "random_tail":
        at = int(rng.integers(1, len(p)))
        p[at:] = rng.integers(0, 256, len(p) - at, dtype=np.uint8).tobytes()
        if bytes(p) == bytes(packet):  # (one chance in 256 for a tail of one byte)
            p[-1] ^= 0x80
    else:
        bit = int(rng.integers(0, 8 * (len(p) if kind == "flip" else min(len(p), HEAD_BYTES))))
        p[bit >> 3] ^= 1 << (bit & 7)
    return bytes(p)


def classify(dec, packet):
    """the mutated packet's class by the reference alone"""
    r, pcm = dec.synthesis(packet)
    if r:
        return "notaudio"
    for pad in PADS:
        r2, pcm2 = dec.synthesis(packet + pad)
        if r2 or not same_bits(pcm, pcm2):
            return "ranout"
    return "complete"


class Group:
    """streams: lists of packets; ends: per stream the last packet's granule position; cls: per stream "clean" or the
    mutated packet's class; where: per stream (base stream, packet, kind) or None"""

    def __init__(self, name, blob, headers, channels):
        self.name, self.blob, self.headers, self.channels = name, blob, headers, channels
        self.streams, self.ends, self.cls, self.where = [], [], [], []
        self._want = {}

    def want(self, s):
        """the reference decoder over stream s: the end granule on the last packet, none on the others -- what a caller of
        the decoder can hand over (vamd_decode_desc::end_granule), and all that is consistent once a mutated head names
        another block size.  Once per distinct stream."""
        key = (tuple(self.streams[s]), self.ends[s])
        if key not in self._want:
            w = ref_host.reference_decode(self.headers + self.streams[s], [-1] * (len(self.streams[s]) - 1) + [self.ends[s]])
            w.setflags(write=False)
            self._want[key] = w
        return self._want[key]

    def shares(self):
        return {c: sum(x == c for x in self.cls) for c in CLASSES}


def cases(name, n, seed=1):
    """the group of n case streams of a setup (no clean ones)"""
    if (name, n, seed) in _groups:
        return _groups[name, n, seed]
    blob, headers, bs, base = base_streams(name, seed)
    g = Group(name, blob, headers, SETUPS[name][0])
    rng = np.random.default_rng(seed)
    dec = ref_host.BlockDecoder(headers)
    for s in range(n):
        packets, end = base[s % 4]
        kind = KINDS[s % 3]
        usable = [k for k, p in enumerate(packets) if len(p) >= 2]
        k = usable[int(rng.integers(0, len(usable)))]
        if s == n - 1:
            k = len(packets) - 1
            assert len(packets[k]) >= 2
        m = mutate(packets[k], kind, rng)
        assert m != packets[k] and len(m) == len(packets[k])
        g.streams.append(packets[:k] + [m] + packets[k + 1:])
        g.ends.append(end)
        g.cls.append(classify(dec, m))
        g.where.append((s % 4, k, kind))
    dec.close()
    # a run must not pass by skipping: the reference itself decodes at least half of the cases in full
    assert 2 * g.shares()["complete"] >= n, (name, g.shares())
    _groups[name, n, seed] = g
    return g


def with_clean(g, clean, seed=1):
    """g's cases with `clean` untouched base streams spread among them (never behind the last case) -> a new Group"""
    _, _, _, base = base_streams(g.name, seed)
    out = Group(g.name, g.blob, g.headers, g.channels)
    out._want = g._want
    n = len(g.streams)
    at = {(i * n) // clean: i for i in range(clean)}
    for s in range(n):
        if s in at:
            packets, end = base[at[s] % 4]
            out.streams.append(list(packets)), out.ends.append(end), out.cls.append("clean"), out.where.append(None)
        out.streams.append(g.streams[s]), out.ends.append(g.ends[s]), out.cls.append(g.cls[s]), out.where.append(g.where[s])
    return out


END_FRAMES = (9000, 3073, 700)
END_COUNTS_9000 = (8000, 8000, 8000, 8000, 8001, 9000, 9023, 9024, 9024, 9024)  # F = 9024, step = 1024, in end_granules()'s order


def end_granules(name="44k_stereo_q4"):
    """The plan's rule for the last block -- frames -= min(frames - end_granule, step), vorbis_synthesis_blockin's for a
    stream that began at granule 0 -- at its edges: streams of END_FRAMES frames, each with the end granules 0, 1,
    F-step-1, F-step, F-step+1, the true length, F-1, F, F+1 and none (F: the frames with no granule position; step: what
    the last block adds), a stream per granule.  -> a Group (cls "clean") whose want() gives the granule to the reference
    on the last packet and -1 on the others; .F and .step per stream"""
    if ("ends", name) in _groups:
        return _groups["ends", name]
    enc = ref_host.encoder(name)
    bs = (enc.blocksize(0), enc.blocksize(1))
    g = Group(name, enc.pack_setup(), ref_host.encoder_headers(ref_host.encoder(name)), enc.channels)
    g.F, g.step = [], []
    for frames in END_FRAMES:
        e = ref_host.encoder(name)
        recs = e.encode_stream(gated_noise(e.channels, e.rate, frames, frames))
        packets, Ws = [r["packet"] for r in recs], [r["W"] for r in recs]
        assert recs[-1]["granulepos"] == frames and len(packets) >= 2
        F = sum(bs[a] // 4 + bs[b] // 4 for a, b in zip(Ws[:-1], Ws[1:]))
        step = bs[Ws[-2]] // 4 + bs[Ws[-1]] // 4
        ends = [0, 1, F - step - 1, F - step, F - step + 1, frames, F - 1, F, F + 1, None]
        assert F - step < frames <= F and all(v is None or v >= 0 for v in ends), (frames, F, step)
        for v in ends:
            g.streams.append(packets), g.ends.append(-1 if v is None else v), g.cls.append("clean"), g.where.append(None)
            g.F.append(F), g.step.append(step)
    _groups["ends", name] = g
    return g


def short_streams(count, name="44k_stereo_q4"):
    """count streams: the eight of SHORT_LENGTHS, a few packets each, again and again -> a Group (cls "clean";
    the reference decodes each distinct one once)"""
    if ("short", name, count) in _groups:
        return _groups["short", name, count]
    enc = ref_host.encoder(name)
    g = Group(name, enc.pack_setup(), ref_host.encoder_headers(ref_host.encoder(name)), enc.channels)
    eight = []
    for frames in SHORT_LENGTHS:
        e = ref_host.encoder(name)
        recs = e.encode_stream(gated_noise(e.channels, e.rate, frames, frames))
        eight.append(([r["packet"] for r in recs], recs[-1]["granulepos"]))
    for s in range(count):
        g.streams.append(eight[s % 8][0]), g.ends.append(eight[s % 8][1]), g.cls.append("clean"), g.where.append(None)
    _groups["short", name, count] = g
    return g


def check(g, results):
    """results: per stream (status, pcm [ch][frames] as numpy).  What both builds of the decoder are held to, against the
    reference: a complete case and a clean stream decode as libvorbis decodes them, bit for bit; a packet that is no audio
    packet is flagged as one; a packet libvorbis ran out of is flagged as truncated (or as a bad codeword), and nothing is
    compared: the documented deviation (k_unpack.h)."""
    assert len(results) == len(g.streams)
    for s, (status, pcm) in enumerate(results):
        what = (g.name, s, g.cls[s], g.where[s])
        if g.cls[s] in ("clean", "complete"):
            want = g.want(s)
            assert status == 0, what + (status,)
            assert pcm.shape == want.shape, what + (pcm.shape, want.shape)
            assert same_bits(pcm, want), what + (int((pcm.view(np.uint32) != want.view(np.uint32)).sum()),)
        elif g.cls[s] == "notaudio":
            assert status == STATUS_NOTAUDIO and pcm.shape == (g.channels, 0), what + (status, pcm.shape)
        else:
            assert status and not status & ~(STATUS_TRUNCATED | STATUS_BADCODE) and pcm.shape == (g.channels, 0), what + (status, pcm.shape)
