"""Cut and mutated packets for the keep policy's tests (vamd_decode_partial: tests/test_unpack_partial_cpu.py on the one-lane
host build, tests/test_decode_partial_gpu.py on the GPU).  Each case is classified BY THE REFERENCE ALONE
(ref_host.BlockDecoder.synthesis: vorbis_synthesis()'s return value and vb->pcm; ref_host.reference_decode, which calls
vorbis_synthesis_blockin exactly when vorbis_synthesis returns 0), so that what the decoder is held to does not come from
the decoder.  Everything is deterministic and computed once per process."""
import numpy as np

from tests import decode_cases, ref_host
from tests.signals import gated_noise

_memo = {}


def _once(key, make):
    if key not in _memo:
        _memo[key] = make()
    return _memo[key]


class Setup:
    """blob, headers, bs, channels of a setup of checker.ENCODERS"""

    def __init__(self, name):
        enc = ref_host.encoder(name)
        self.name, self.blob, self.channels = name, enc.pack_setup(), enc.channels
        self.headers = ref_host.encoder_headers(ref_host.encoder(name))
        self.bs = (enc.blocksize(0), enc.blocksize(1))


def setup(name):
    return _once(("setup", name), lambda: Setup(name))


def stereo_streams():
    """the 700-frame and the 3073-frame 44k_stereo_q4 streams of decode_cases.END_FRAMES -> [(packets, frames)] in that
    order; the second holds both block sizes"""
    g = decode_cases.end_granules()
    at = {f: 10 * i for i, f in enumerate(decode_cases.END_FRAMES)}  # (ten end granules per stream, the same packets)
    out = [(list(g.streams[at[f]]), f) for f in (700, 3073)]
    Ws = {(p[0] >> 1) & 1 for p in out[1][0]}
    assert Ws == {0, 1}, Ws
    return out


def stream_of(name, frames=3073):
    """the reference encoder of `name` over gated noise -> (packets, frames)"""
    def make():
        e = ref_host.encoder(name)
        recs = e.encode_stream(gated_noise(e.channels, e.rate, frames, frames))
        assert recs[-1]["granulepos"] == frames
        return [r["packet"] for r in recs], frames
    return _once(("stream", name, frames), make)


HEAD, STEP, TAIL = 40, 5, 12


def thinned(length):
    """The fixed rule by which a long packet's cuts are thinned (44k_51_q3, 44k_mono_q5): every length up to HEAD (the
    head and the floors lie there), the last TAIL lengths (where the last submap's residue ends), and every STEP-th
    between."""
    return [n for n in range(1, length) if n <= HEAD or n >= length - TAIL or n % STEP == 0]


def every(length):
    return list(range(1, length))


def cuts(packets, rule):
    """-> [(packet index, length, the cut packet)]"""
    return [(k, n, p[:n]) for k, p in enumerate(packets) for n in rule(len(p))]


def classify(headers, packets):
    """-> per packet (vorbis_synthesis()'s return value, vb->pcm or None), read-only"""
    dec = ref_host.BlockDecoder(headers)
    out = []
    for p in packets:
        r, pcm = dec.synthesis(p)
        if pcm is not None:
            pcm.setflags(write=False)
        out.append((r, pcm))
    dec.close()
    return out


def stereo_cut_cases():
    """every cut of every packet of the two stereo streams -> (setup, [(stream, packet, length, cut)], their classes)"""
    def make():
        S = setup("44k_stereo_q4")
        cases = [(s, k, n, c) for s, (packets, _) in enumerate(stereo_streams()) for k, n, c in cuts(packets, every)]
        return S, cases, classify(S.headers, [c for _, _, _, c in cases])
    return _once("stereo_cuts", make)


def damaged_streams():
    """The stream tests' group, from the 3073-frame stereo stream P and the 700-frame one Q: a packet cut to half its
    length in first, middle and last place, two cut packets in one stream, clean neighbours between them.
    -> (setup, streams, end granules, which streams are damaged, what the reference decodes each to)"""
    def make():
        S = setup("44k_stereo_q4")
        (Q, fq), (P, fp) = stereo_streams()
        assert len(P) >= 5 and all(len(p) >= 4 for p in P)
        half = lambda p: p[:len(p) // 2]
        mid = len(P) // 2
        first = [half(P[0])] + P[1:]
        middle = P[:mid] + [half(P[mid])] + P[mid + 1:]
        last = P[:-1] + [half(P[-1])]
        two = P[:1] + [half(P[1])] + P[2:mid + 1] + [half(P[mid + 1])] + P[mid + 2:]
        streams = [P, first, Q, middle, last, P, two, Q]
        ends = [fp, fp, fq, fp, fp, fp, fp, fq]
        damaged = [False, True, False, True, True, False, True, False]
        want = []
        for packets, end in zip(streams, ends):
            w = ref_host.reference_decode(S.headers + packets, [-1] * (len(packets) - 1) + [end])
            w.setflags(write=False)
            want.append(w)
        # the end granule cuts the last block, and the damage is heard: no damaged stream decodes to the clean one's samples
        assert want[0].shape == (2, fp) and want[2].shape == (2, fq)
        assert all(w.shape == (2, fp) and not np.array_equal(w, want[0]) for w, d in zip(want, damaged) if d)
        return S, streams, ends, damaged, want
    return _once("damaged", make)


def mutations(name, flips, randoms, seed=32):
    """seeded single-bit flips of a base stream's packets (decode_cases.mutate) and packets of random bytes, half of which
    pass for audio -> (setup, packets, their classes)"""
    def make():
        S = setup(name)
        _, _, _, base = decode_cases.base_streams(name, 1)
        pool = [p for packets, _ in base for p in packets if len(p) >= 2]
        rng = np.random.default_rng(seed)
        out = []
        for k in range(flips):
            out.append(decode_cases.mutate(pool[int(rng.integers(0, len(pool)))], "flip" if k % 2 else "flip_head", rng))
        for k in range(randoms):
            p = bytearray(rng.integers(0, 256, int(rng.integers(1, 400)), dtype=np.uint8).tobytes())
            if k & 1:
                p[0] &= 0xfe
            out.append(bytes(p))
        return S, out, classify(S.headers, out)
    return _once(("mutations", name, flips, randoms, seed), make)


def value_list_cases():
    """One rewritten-header setup whose residue books are no lattice (setup_header_cases' "scaled": non-integer values, the
    k_synth_values path) and every cut of one long and one short packet of the 3073-frame stereo stream
    -> (headers, bs, [(packet, length, cut)], their classes under those headers)"""
    def make():
        from tests import setup_header_cases as shc
        S = setup("44k_stereo_q4")
        hv = shc.variant(S.headers, "scaled")
        P, _ = stereo_streams()[1]
        long_ = max((p for p in P if (p[0] >> 1) & 1), key=len)
        short = max((p for p in P if not (p[0] >> 1) & 1), key=len)
        cases = [(k, n, p[:n]) for k, p in enumerate((long_, short)) for n in every(len(p))]
        return hv, S.bs, cases, classify(hv, [c for _, _, c in cases])
    return _once("value_list", make)


def _decode_all(headers, streams):
    out = []
    for packets in streams:
        w = ref_host.reference_decode(list(headers) + list(packets), [-1] * len(packets))
        w.setflags(write=False)
        out.append(w)
    return out


def cut_streams():
    """stereo_cut_cases() as streams for a whole decode call, one per cut: the cut packet between its two neighbours in its
    stream (the first and the last packet have one), no end granule -> (setup, streams, what the reference decodes each to)"""
    def make():
        S, cases_, classes = stereo_cut_cases()
        assert all(r == 0 for r, _ in classes)  # (a cut of a byte or more leaves the head whole)
        base = [packets for packets, _ in stereo_streams()]
        streams = [base[s][max(k - 1, 0):k] + [c] + base[s][k + 1:k + 2] for s, k, _, c in cases_]
        return S, streams, _decode_all(S.headers, streams)
    return _once("cut_streams", make)


def value_list_streams():
    """value_list_cases() as streams: each cut between two whole long packets -> (headers, streams, the reference's)"""
    def make():
        hv, _, cases_, _ = value_list_cases()
        P, _ = stereo_streams()[1]
        whole = max((p for p in P if (p[0] >> 1) & 1), key=len)
        streams = [[whole, c, whole] for _, _, c in cases_]
        return hv, streams, _decode_all(hv, streams)
    return _once("value_list_streams", make)


# ---- rewritten headers that reach the stops genuine setups cannot (tests/setup_header_cases.py parses and emits) ----
HEADER_KINDS = ("spare_phrase", "empty_phrase", "empty_floor", "empty_value")


def _empty_copy(S, k):
    """a copy of book k without used entries, appended -> its number"""
    c = dict(S["books"][k])
    c["lengths"], c["enc"] = [0] * c["entries"], "sparse"
    S["books"].append(c)
    return len(S["books"]) - 1


def rewritten_headers(name, kind):
    """the genuine headers of `name` with the setup header changed:
      spare_phrase  every residue's phrase book gets one entry more than classes^dim: its shortest codeword is split in two,
                    and the new half names no classes (libvorbis: temp >= partvals, eopbreak with the reader where it stands)
      empty_phrase  the short blocks' residue reads its phrase words from a book without used entries
      empty_floor   the first sub-book of the short blocks' floor that is in use is a book without used entries
      empty_value   the first value book of the short blocks' residue is a book without used entries"""
    def make():
        from tests import setup_header_cases as shc
        ident, comment, genuine = (bytes(h) for h in setup(name).headers)
        S = shc.parse(genuine, ident[11])
        short = S["maps"][S["modes"][0][3]]["sub"][0]  # (time, floor, residue) of the short blocks' first submap
        if kind == "spare_phrase":
            for k in sorted({r["groupbook"] for r in S["residues"]}):
                c = S["books"][k]
                assert c["maptype"] == 0 and c["entries"] == len(S["residues"][0]["cascade"]) ** c["dim"] or len(S["residues"]) > 2
                at = c["lengths"].index(min(c["lengths"]))
                c["lengths"][at] += 1
                c["lengths"].append(c["lengths"][at])
                c["entries"], c["enc"] = c["entries"] + 1, "plain"
        elif kind == "empty_phrase":
            r = S["residues"][short[2]]
            r["groupbook"] = _empty_copy(S, r["groupbook"])
        elif kind == "empty_floor":
            f = S["floors"][short[1]]
            c = next(c for c in (f["cls"][i] for i in f["classes"]) if any(c["subbooks"]))
            at = next(i for i, v in enumerate(c["subbooks"]) if v)
            c["subbooks"][at] = _empty_copy(S, c["subbooks"][at] - 1) + 1  # (the header holds the book's number plus one)
        elif kind == "empty_value":
            r = dict(S["residues"][short[2]])
            r["books"] = [_empty_copy(S, r["books"][0])] + r["books"][1:]
            S["residues"][short[2]] = r
        else:
            raise ValueError(kind)
        out = [ident, comment, shc.emit(S)]
        assert ref_host._headerin(ref_host._reflib(), out)[0] == [0, 0, 0], kind  # the reference takes the headers
        return out
    return _once(("headers", name, kind), make)


def rewritten_cases(name, kind, flips=60, seed=5):
    """the genuine packets of a 3073-frame stream of `name`, and seeded bit flips of them, under rewritten_headers(name, kind)
    -> (headers, bs, channels, packets, their classes under those headers)"""
    def make():
        hv = rewritten_headers(name, kind)
        P, _ = stream_of(name) if name != "44k_stereo_q4" else stereo_streams()[1]
        rng = np.random.default_rng(seed)
        packets = list(P) + [decode_cases.mutate(P[int(rng.integers(0, len(P)))], "flip", rng) for _ in range(flips)]
        S = setup(name)
        return hv, S.bs, S.channels, packets, classify(hv, packets)
    return _once(("rewritten", name, kind, flips, seed), make)
