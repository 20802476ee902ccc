"""Audio packets written under a made setup (tests/setup_maker.py), from Vorbis I 4.3 (the packet's head and the order of
its parts), 7.2.3 (floor 1) and 8.6 (the residues): the mode, a long block's two window flags; per channel the floor-used
bit, the two range posts, and per partition the class word and the sub-book words; per submap, stage by stage, the phrase
words (in the first stage) and the entries of every partition whose class has a book in that stage -- per channel for
type 1, once for type 2, for the channels that are decoded after the coupling steps have spread "used".

Every entry is drawn uniformly over the USED entries of its book, so codewords of any depth are written (random bits reach
a codeword of 32 bits once in 2 ** 32 draws).  write_packet returns the packet with its exact length in bits; self_check
holds each written packet to the reference alone: vorbis_synthesis returns 0, has consumed exactly those bits, and reads
nothing beyond them (decode_cases.classify)."""
import ctypes as C

import numpy as np

from tests.setup_header_cases import ilog

QUANT_Q = (256, 128, 86, 64)
P_UNUSED = 0.2


class BitWriter:
    """oggpack_write: the first bit written is bit 0 of byte 0"""

    def __init__(self):
        self.acc, self.n, self.out, self.total = 0, 0, bytearray(), 0

    def write(self, value, bits):
        assert 0 <= value < (1 << bits) or bits == 0, (value, bits)
        self.acc |= value << self.n
        self.n += bits
        self.total += bits
        if self.n >= 1024:
            k = self.n // 8
            self.out += (self.acc & ((1 << (8 * k)) - 1)).to_bytes(k, "little")
            self.acc >>= 8 * k
            self.n -= 8 * k

    def bytes(self):
        return bytes(self.out) + self.acc.to_bytes((self.n + 7) // 8, "little")


def codewords(lengths):
    """Vorbis I 3.2.1: entries in order take the lowest free codeword of their length -> per entry the word as the writer
    hands it to BitWriter (the tree's first branch in bit 0), None for an unused entry.  The tree must come out complete."""
    out = [None] * len(lengths)
    marker = [0] * 34
    for e, n in enumerate(lengths):
        if n <= 0:
            continue
        word = marker[n]
        assert n == 32 or not word >> n, "an over-populated tree"
        out[e] = int(format(word, "0%db" % n)[::-1], 2)
        for j in range(n, 0, -1):  # (lib/sharedbook.c:_make_words' walk, which is the specification's rule)
            if marker[j] & 1:
                marker[j] = marker[j - 1] << 1 if j > 1 else marker[j] + 1
                break
            marker[j] += 1
        for j in range(n + 1, 33):
            if marker[j] >> 1 != word:
                break
            word = marker[j]
            marker[j] = (marker[j - 1] << 1) & 0xffffffff
    assert abs(sum(2.0 ** -n for n in lengths if n > 0) - 1.0) < 1e-12, "the tree is not complete"
    return out


def _book(S, bi):
    """-> (the used entries, their words, the lengths) of book bi of the setup S, worked out once and kept with S"""
    kept = S.setdefault("_words", {})
    if bi not in kept:
        c = S["books"][bi]
        words = codewords(c["lengths"])
        kept[bi] = (np.array([e for e, w in enumerate(words) if w is not None]), words, c["lengths"])
    return kept[bi]


def mode_plan(nmodes, count, rng):
    """-> [(mode, (previous flag, next flag))] of a stream of `count` packets: with two modes at least two packets of mode
    0 and a long block with each of the four flag pairs, in a seeded order; the flags of a short block are not written"""
    if nmodes == 1:
        return [(0, (0, 0))] * count
    plan = [(1, (a, b)) for a in (0, 1) for b in (0, 1)] + [(0, (0, 0))] * 2
    while len(plan) < count:
        plan.append((1, (int(rng.integers(0, 2)), int(rng.integers(0, 2)))) if rng.integers(0, 2) else (0, (0, 0)))
    return [plan[int(k)] for k in rng.permutation(len(plan))]


def write_packet(S, bs, rng, mode, flags, force=None):
    """One audio packet of mode `mode` under the parsed setup S -> dict(packet, bits: its exact length, mode, flags,
    at: the bit at which the floors, the first phrase word and the first residue entry begin (None: none written),
    deep: the (book, entry) written through a codeword of 32 bits or as entry 65 534, longest: the longest codeword,
    dirtied: the channels without a floor that a coupling step made decoded all the same).
    force: {book: [entries]} to be written, in order, the first times that book is used."""
    force = force if force is not None else {}
    out = BitWriter()
    note = dict(mode=mode, flags=flags, at=dict(floor=None, phrase=None, residue=None), deep=set(), longest=0)

    def entry(bi, what=None):
        used, words, lengths = _book(S, bi)
        e = force[bi].pop(0) if force.get(bi) else int(used[int(rng.integers(0, len(used)))])
        assert words[e] is not None
        if what and note["at"][what] is None:
            note["at"][what] = out.total
        out.write(words[e], lengths[e])
        note["longest"] = max(note["longest"], lengths[e])
        if lengths[e] == 32 or e == 65534:
            note["deep"].add((bi, e))
        return e

    out.write(0, 1)
    out.write(mode, ilog(len(S["modes"]) - 1))
    W, _, _, mapping = S["modes"][mode]
    if W:
        out.write(flags[0], 1), out.write(flags[1], 1)
    m = S["maps"][mapping]
    ch, n2 = S["channels"], bs[W] // 2
    mux = m["mux"] or [0] * ch
    note["at"]["floor"] = out.total
    nonzero = []
    for c in range(ch):
        f = S["floors"][m["sub"][mux[c]][1]]
        used = rng.random() >= P_UNUSED
        out.write(int(used), 1)
        nonzero.append(bool(used))
        if not used:
            continue
        q = QUANT_Q[f["mult"]]
        out.write(int(rng.integers(0, q)), ilog(q - 1)), out.write(int(rng.integers(0, q)), ilog(q - 1))
        for p in f["classes"]:
            k = f["cls"][p]
            cval = entry(k["book"]) if k["subs"] else 0
            for _ in range(k["dim"]):
                book = k["subbooks"][cval & ((1 << k["subs"]) - 1)]
                cval >>= k["subs"]
                if book:
                    entry(book - 1)
    floors_used = list(nonzero)
    for mag, ang in m["coupling"] or ():
        if nonzero[mag] or nonzero[ang]:
            nonzero[mag] = nonzero[ang] = True
    note["dirtied"] = [c for c in range(ch) if nonzero[c] and not floors_used[c]]  # no floor, yet decoded: through a coupling step
    for sm, (_, _, rn) in enumerate(m["sub"]):
        r = S["residues"][rn]
        chans = [c for c in range(ch) if mux[c] == sm]
        if r["type"] == 2:
            streams, span = (1 if any(nonzero[c] for c in chans) else 0), n2 * len(chans)
        else:
            streams, span = sum(nonzero[c] for c in chans), n2
        grouping, nclasses = r["grouping"] + 1, len(r["cascade"])
        partvals = max(min(r["end"], span) - r["begin"], 0) // grouping
        books, at = [], 0
        for low, _, high in r["cascade"]:
            bits = low | high << 3
            books.append({s: r["books"][at + bin(bits & ((1 << s) - 1)).count("1")] for s in range(8) if bits >> s & 1})
            at += bin(bits).count("1")
        stages = max((max(b) + 1 for b in books if b), default=0)
        pdim = S["books"][r["groupbook"]]["dim"]
        cls = [[0] * (partvals + pdim) for _ in range(streams)]
        for s in range(stages if streams else 0):
            i = 0
            while i < partvals:
                if s == 0:
                    for j in range(streams):
                        e = entry(r["groupbook"], "phrase")
                        for k in range(pdim):
                            cls[j][i + k] = e // nclasses ** (pdim - 1 - k) % nclasses
                for _ in range(pdim):
                    if i >= partvals:
                        break
                    for j in range(streams):
                        bi = books[cls[j][i]].get(s)
                        if bi is not None:
                            for _ in range(grouping // S["books"][bi]["dim"]):
                                entry(bi, "residue")
                    i += 1
    note["packet"], note["bits"] = out.bytes(), out.total
    return note


# ---- the writer against the reference ----
def _decoder(headers, S):
    """ref_host.BlockDecoder whose synthesis() takes the block's size from the setup's own mode field (with one mode there
    is no mode bit), and the bits vorbis_synthesis consumed"""
    from tests import ref_host

    class Decoder(ref_host.BlockDecoder):
        def synthesis(self, packet):
            r = self._synthesis(packet)
            if r:
                return r, None
            mode = (packet[0] >> 1) & ((1 << ilog(len(S["modes"]) - 1)) - 1)
            return 0, self._pcm(S["modes"][mode][0])

        def consumed(self):
            """oggpack_bits(&vb->opb): opb is vorbis_block's second field, behind float **pcm"""
            return int(self.L.oggpack_bits(C.byref(self.vb, C.sizeof(C.c_void_p))))
    dec = Decoder(headers)
    assert hasattr(dec.L, "oggpack_bits"), "the oracle library does not export oggpack_bits: the writer would go unchecked"
    dec.L.oggpack_bits.restype, dec.L.oggpack_bits.argtypes = C.c_long, [C.c_void_p]
    return dec


def self_check(case):
    """every packet of every stream of a setup_maker.Case: vorbis_synthesis returns 0, has consumed exactly the bits the
    writer wrote, and gives the same block whatever follows the packet -> the number of packets"""
    from tests import decode_cases
    dec = _decoder(case.headers, case.M.S)
    count = 0
    try:
        for s, notes in enumerate(case.notes):
            for k, n in enumerate(notes):
                r, _ = dec.synthesis(n["packet"])
                assert r == 0, (case.name, s, k, r)
                assert dec.consumed() == n["bits"], (case.name, s, k, dec.consumed(), n["bits"])
                assert len(n["packet"]) == (n["bits"] + 7) // 8
                assert decode_cases.classify(dec, n["packet"]) == "complete", (case.name, s, k)
                count += 1
    finally:
        dec.close()
    return count


def coverage(case):
    """from the written choices: (the modes, the flag pairs of the long blocks) that occur"""
    notes = [n for row in case.notes for n in row]
    return {n["mode"] for n in notes}, {n["flags"] for n in notes if case.W(n)}
