"""Setups written from a description, for the header-made decoder's tests (tests/test_setup_maker_cpu.py,
tests/test_setup_maker_gpu.py): where tests/setup_header_cases.py changes one thing in a genuine header, this writes the three
header packets of shapes no encoder here produces -- equal block sizes, one mode, the pair 64 / 4096, eight channels in two
interleaved submaps under a coupling chain, floors of 65 posts, residues with holes in their cascades, codewords of 32 bits,
books of 65 535 and 65 536 entries -- all inside the covered shape header_build_image (vorbis_amd/csrc/vamd_headers.h) states.

Every book is a complete code tree, so whatever tests/packet_writer.py writes under such a setup is parseable; a phrase
book has exactly classes ** dim entries.  CASES names the hand-made setups, random_setup(seed) draws every field inside the
limits.  case(name) / seeded(seed) -> a Case: the headers, the parsed setup the writer reads, and the written streams."""
import os
import subprocess

import numpy as np

from tests import packet_writer
from tests.setup_header_cases import emit, float32_pack, ilog, lookup1_values

STREAMS = 4
_memo = {}


# ---- the packets around the setup ----
def identification(channels, rate, bs):
    """Vorbis I 4.2.2: 30 bytes"""
    b0, b1 = (int(v).bit_length() - 1 for v in bs)
    assert (1 << b0, 1 << b1) == tuple(bs)
    return (b"\x01vorbis" + (0).to_bytes(4, "little") + bytes([channels]) + int(rate).to_bytes(4, "little") + bytes(12)
            + bytes([b0 | b1 << 4, 1]))


def comment(vendor=b"tests/setup_maker.py"):
    return b"\x03vorbis" + len(vendor).to_bytes(4, "little") + vendor + (0).to_bytes(4, "little") + b"\x01"


# ---- code trees ----
def _tree(n):
    """the lengths of a complete tree of n >= 2 leaves on two neighbouring depths, in rising order"""
    assert n >= 2
    k = n.bit_length() - 1
    deep = 2 * (n - (1 << k))
    return [k] * (n - deep) + [k + 1] * deep


def flat(entries, dim=1):
    return dict(dim=dim, entries=entries, enc="plain", lengths=_tree(entries), maptype=0)


def ordered(entries, dim=1):
    """the same tree written run by run"""
    return dict(flat(entries, dim), enc="ordered")


def comb32(dim=1):
    """33 entries of lengths 1, 2, ..., 31, 32, 32: the two deepest codewords have 32 bits"""
    return dict(dim=dim, entries=33, enc="plain", lengths=list(range(1, 32)) + [32, 32], maptype=0)


def sparse(entries, used, rng, dim=1):
    """`used` of the entries, spread by rng, hold a complete tree; the others are unused"""
    lengths = [0] * entries
    tree = _tree(used)
    for at, k in zip(sorted(int(v) for v in rng.choice(entries, used, replace=False)), rng.permutation(used)):
        lengths[at] = tree[int(k)]
    return dict(dim=dim, entries=entries, enc="sparse", lengths=lengths, maptype=0)


def big16(entries=65535, dim=1):
    """65 534 entries of length 16 behind one of length 15, written as two runs"""
    assert entries == 65535
    return dict(dim=dim, entries=entries, enc="ordered", lengths=[15] + [16] * 65534, maptype=0)


# ---- value mappings ----
def lattice(c, delta=1):
    """lookup type 1 over the centred integers, in the order libvorbisenc's books list them: 0, -1, +1, -2, ... times delta"""
    qv = lookup1_values(c["dim"], c["entries"])
    ze = qv >> 1
    quant = [ze - ((d + 1) >> 1) if d & 1 else ze + (d >> 1) for d in range(qv)]
    return dict(c, maptype=1, q_min=float32_pack(-ze * delta), q_delta=float32_pack(delta), q_bits=max(1, ilog(qv - 1)), q_seq=0, quant=quant)


def listed(c, rng, maptype, bits, q_min=-0.5, q_delta=1.0 / 64, seq=0):
    """lookup type 1 (a list of lookup1_values multiplicands) or 2 (one per scalar of every entry) of seeded multiplicands
    `bits` wide; q_delta shrinks with the width, so that a value stays near one"""
    count = lookup1_values(c["dim"], c["entries"]) if maptype == 1 else c["entries"] * c["dim"]
    quant = [int(v) for v in rng.integers(0, 1 << bits, count)]
    return dict(c, maptype=maptype, q_min=float32_pack(q_min), q_delta=float32_pack(q_delta * 2.0 ** (4 - bits)), q_bits=bits, q_seq=seq, quant=quant)


class Setup:
    """the setup packet's sections as tests/setup_header_cases.py parses and emits them, filled in piece by piece"""

    def __init__(self, channels, bs, rate=44100):
        self.S = dict(channels=channels, books=[], times=[0], floors=[], residues=[], maps=[], modes=[])
        self.channels, self.bs, self.rate = channels, tuple(bs), rate

    def book(self, c):
        self.S["books"].append(c)
        assert len(self.S["books"]) <= 255
        return len(self.S["books"]) - 1

    def floor(self, rangebits, mult, classes, partitions, x):
        """classes: [(dim, sub-class bits, class book or None, [sub-book or None] x (1 << bits))]; partitions: the class of
        each; x: the places of the posts behind the two end posts, in the order written"""
        cls = []
        for dim, subs, book, subbooks in classes:
            assert len(subbooks) == 1 << subs and (book is not None) == (subs > 0) and 1 <= dim <= 8
            cls.append(dict(dim=dim, subs=subs, book=book, subbooks=[0 if s is None else s + 1 for s in subbooks]))
        assert max(partitions, default=-1) == len(cls) - 1 and len(partitions) <= 31 and len(x) == sum(cls[p]["dim"] for p in partitions) <= 63
        assert len(set(x)) == len(x) and all(0 < v < (1 << rangebits) for v in x)
        self.S["floors"].append(dict(classes=list(partitions), cls=cls, mult=mult - 1, rangebits=rangebits, x=[int(v) for v in x]))
        return len(self.S["floors"]) - 1

    def residue(self, kind, begin, end, grouping, phrase, classes):
        """classes: per class {stage: book}; phrase: the phrase book, of len(classes) ** dim entries"""
        books = self.S["books"]
        assert books[phrase]["entries"] == len(classes) ** books[phrase]["dim"] and books[phrase]["dim"] <= 16
        cascade, order = [], []
        for c in classes:
            bits = sum(1 << s for s in c)
            cascade.append((bits & 7, 1 if bits >> 3 else 0, bits >> 3))
            for s in sorted(c):
                assert books[c[s]]["maptype"] and grouping % books[c[s]]["dim"] == 0 and books[c[s]]["entries"] <= 65535
                order.append(c[s])
        self.S["residues"].append(dict(type=kind, begin=begin, end=end, grouping=grouping - 1, groupbook=phrase, cascade=cascade, books=order))
        return len(self.S["residues"]) - 1

    def mapping(self, subs, mux=None, coupling=None):
        """subs: [(floor, residue)]; mux: the channels' submaps where there are two; coupling: [(magnitude, angle)]"""
        assert (mux is None) == (len(subs) == 1)
        self.S["maps"].append(dict(submaps=len(subs) if len(subs) > 1 else None, coupling=list(coupling) if coupling else None,
                                   mux=list(mux) if mux else None, sub=[(0, f, r) for f, r in subs]))
        return len(self.S["maps"]) - 1

    def modes(self, *mappings):
        """mode i has block flag i"""
        self.S["modes"] = [(i, 0, 0, m) for i, m in enumerate(mappings)]

    def headers(self):
        return [identification(self.channels, self.rate, self.bs), comment(), emit(self.S)]


# ---- pieces drawn by an rng ----
def floor_book(M, rng, kind=None):
    """a book a floor reads posts or class words with: at most 64 entries, so that a post stays inside the smallest range
    (quant_q = 64 of multiplier 4) whatever entry is drawn"""
    kind = kind or ("flat", "ordered", "sparse", "comb32")[int(rng.integers(0, 4))]
    n = int(rng.integers(2, 65))
    if kind == "comb32":
        return M.book(comb32())
    if kind == "sparse":
        n = min(n, 40)
        return M.book(sparse(n + int(rng.integers(1, 25)), n, rng))
    return M.book(flat(n) if kind == "flat" else ordered(n))


def draw_floor(M, rng, rangebits, mult, dims, subs=None):
    """a floor of 2 + sum(dims) posts: a class per entry of dims, with subs[i] sub-class bits (drawn where None), sub-books
    of which some are "no book" wherever a class has more than one, and an X list in no order"""
    classes = []
    for i, dim in enumerate(dims):
        sb = int(rng.integers(0, 4)) if subs is None else subs[i]
        subbooks = [floor_book(M, rng) for _ in range(1 << sb)]
        if sb:
            subbooks[int(rng.integers(0, 1 << sb))] = None
        classes.append((dim, sb, floor_book(M, rng) if sb else None, subbooks))
    count = sum(dims)
    assert count < (1 << rangebits)
    x = rng.choice(np.arange(1, 1 << rangebits), count, replace=False)
    return M.floor(rangebits, mult, classes, list(range(len(dims))), x)


def value_book(M, rng, dim, entries=None, kind=None):
    """a residue book: a lattice book, or one with a value list of either lookup type"""
    kind = kind or ("lattice", "list1", "list2", "list1_seq", "sparse2")[int(rng.integers(0, 5))]
    entries = entries or int(rng.integers(2, 90))
    bits = int(rng.integers(1, 17))
    if kind == "lattice":
        qv = int(rng.integers(2, 6)) if dim > 1 else entries
        return M.book(lattice(flat(max(2, min(qv ** dim, 4096)), dim)))
    if kind == "sparse2":
        return M.book(listed(sparse(entries + int(rng.integers(1, 60)), entries, rng, dim), rng, 2, bits))
    return M.book(listed(flat(entries, dim) if rng.integers(0, 2) else ordered(entries, dim), rng, 1 if kind.startswith("list1") else 2, bits,
                         seq=1 if kind.endswith("seq") else 0))


def phrase_book(M, rng, classes, dim):
    n = classes ** dim
    return M.book(flat(n, dim) if rng.integers(0, 2) else ordered(n, dim))


# ---- the named cases ----
def _equal_64_one_mode(rng):
    M = Setup(1, (64, 64))
    f = draw_floor(M, rng, 5, 2, [2, 3, 1], [0, 1, 2])
    r = M.residue(1, 0, 32, 8, phrase_book(M, rng, 2, 2), [{0: value_book(M, rng, 2, kind="lattice")}, {0: value_book(M, rng, 4, kind="list1"), 1: value_book(M, rng, 1, kind="list2")}])
    M.modes(M.mapping([(f, r)]))
    return M


def _equal_2048(rng):
    M = Setup(2, (2048, 2048))
    f = draw_floor(M, rng, 10, 1, [3, 4, 2, 1], [1, 2, 0, 1])
    classes = [{}, {0: value_book(M, rng, 4, kind="lattice")}, {0: value_book(M, rng, 2, kind="lattice"), 2: value_book(M, rng, 8, kind="list2")}]
    r = M.residue(2, 0, 2048, 32, phrase_book(M, rng, 3, 3), classes)  # 64 partitions under phrase words of 3
    m = M.mapping([(f, r)], coupling=[(0, 1)])
    M.modes(m, m)
    return M


def _one_mode_short(rng):
    M = Setup(2, (256, 2048))
    f = draw_floor(M, rng, 7, 3, [2, 2, 5], [0, 2, 1])
    r = M.residue(1, 0, 128, 8, phrase_book(M, rng, 3, 2), [{}, {0: value_book(M, rng, 2, kind="lattice")}, {0: value_book(M, rng, 8, kind="list1"), 1: value_book(M, rng, 1, kind="lattice")}])
    M.modes(M.mapping([(f, r)]))
    return M


def _far_64_4096(rng):
    M = Setup(2, (64, 4096))
    f0 = draw_floor(M, rng, 5, 4, [2, 2], [1, 0])
    f1 = draw_floor(M, rng, 11, 2, [4, 6, 3], [2, 1, 0])
    # one residue for both sizes: its end, 4096, is clipped to the 64 values of a short stereo block
    r = M.residue(2, 0, 4096, 16, phrase_book(M, rng, 3, 2), [{}, {0: value_book(M, rng, 2, kind="lattice")}, {0: value_book(M, rng, 4, kind="list2"), 1: value_book(M, rng, 2, kind="lattice")}])
    M.modes(M.mapping([(f0, r)], coupling=[(0, 1)]), M.mapping([(f1, r)], coupling=[(0, 1)]))
    return M


EIGHT_MUX = [0, 1, 0, 0, 1, 0, 1, 0]  # submap 1 holds channels 1, 4 and 6
EIGHT_COUPLING = [(0, 1), (0, 2), (5, 3), (4, 7)]  # a chain on channel 0 (its first step across the submaps), a reversed pair, 4 -> 7 across


def _eight_ch_max(rng):
    M = Setup(8, (512, 4096))
    fs = draw_floor(M, rng, 8, 3, [3, 5, 2], [1, 0, 2])
    fl0 = draw_floor(M, rng, 11, 4, [6, 8, 4, 7], [2, 3, 0, 1])
    fl1 = draw_floor(M, rng, 10, 3, [5, 2, 2], [1, 1, 0])  # a range of 1024 inside the 2048 bins of a long block
    # type 1 over the bundle of 5: 8 stages; long blocks: (2048 - 8) / 20 = 102 partitions, x 5 = 510 slots; short: 12 x 5
    all8 = {s: value_book(M, rng, (1, 2, 4, 5, 2, 1, 4, 5)[s], kind=("lattice", "list1", "list2", "lattice")[s % 4]) for s in range(8)}
    r0 = M.residue(1, 8, 2048, 20, phrase_book(M, rng, 4, 3), [{}, all8, {0: value_book(M, rng, 5, kind="lattice")}, {1: value_book(M, rng, 4, kind="list1_seq"), 7: value_book(M, rng, 2, kind="lattice")}])
    # type 2 over the bundle of 3: the header's end lies beyond the 3 x 2048 values, which are 512 partitions of 12
    r1 = M.residue(2, 0, 7000, 12, phrase_book(M, rng, 3, 4), [{}, {0: value_book(M, rng, 3, kind="lattice"), 1: value_book(M, rng, 6, kind="list2")}, {0: value_book(M, rng, 4, kind="lattice"), 2: value_book(M, rng, 3, kind="sparse2")}])
    M.modes(M.mapping([(fs, r0), (fs, r1)], EIGHT_MUX, EIGHT_COUPLING), M.mapping([(fl0, r0), (fl1, r1)], EIGHT_MUX, EIGHT_COUPLING))
    return M


def _floor_shapes(rng):
    M = Setup(2, (256, 1024))
    # 65 posts in a range of 128: class dimensions 8, 8, 7 and 1; 3, 0, 2 and 1 sub-class bits
    classes = []
    for dim, sb in ((8, 3), (8, 0), (7, 2), (1, 1)):
        subbooks = [floor_book(M, rng) for _ in range(1 << sb)]
        if sb:
            subbooks[1] = None
        if sb == 3:
            subbooks[6] = None
        classes.append((dim, sb, floor_book(M, rng) if sb else None, subbooks))
    partitions = [0, 1, 0, 1, 2, 0, 1, 2, 3]
    x = rng.choice(np.arange(1, 128), 63, replace=False)
    assert list(x) != sorted(x)
    fa = M.floor(7, 1, classes, partitions, x)
    fb = draw_floor(M, rng, 7, 2, [1, 2, 1], [1, 0, 2])  # 6 posts in a range of 128, drawn into the 512 bins of a long block
    r = M.residue(1, 0, 512, 16, phrase_book(M, rng, 2, 3), [{}, {0: value_book(M, rng, 2, kind="lattice"), 1: value_book(M, rng, 4, kind="list1")}])
    M.modes(M.mapping([(fa, r)]), M.mapping([(fa, r), (fb, r)], [0, 1]))
    return M


def _book_shapes(rng):
    M = Setup(2, (128, 512))
    comb = M.book(comb32())
    M.comb_value = M.book(listed(comb32(2), rng, 1, 16))  # lookup1_values(2, 33) = 5 multiplicands of 16 bits
    M.big = M.book(listed(big16(), rng, 1, 5))
    spars = M.book(listed(sparse(300, 11, rng, 2), rng, 2, 7))
    f = M.floor(6, 2, [(2, 1, comb, [comb, None]), (3, 0, None, [floor_book(M, rng, "flat")])], [0, 1, 0], rng.choice(np.arange(1, 64), 7, replace=False))
    # short blocks: (128 - 8) / 4 = 30 partitions under phrase words of 16, from a book of 2 ** 16 entries
    r0 = M.residue(2, 8, 128, 4, M.book(ordered(65536, 16)), [{0: value_book(M, rng, 2, 9, kind="lattice")}, {0: M.big, 1: spars}])
    # long blocks: 33 classes under comb32 as the phrase book: 512 / 8 = 64 partitions under phrase words of 1
    pool = (M.comb_value, spars, value_book(M, rng, 4, kind="lattice"), value_book(M, rng, 8, kind="list2"))
    classes = [{0: pool[c % 4]} if c % 3 != 1 else {} for c in range(33)]
    classes[32] = {0: M.comb_value, 1: M.big}
    r1 = M.residue(2, 0, 512, 8, comb, classes)
    M.modes(M.mapping([(f, r0)], coupling=[(1, 0)]), M.mapping([(f, r1)], coupling=[(1, 0)]))
    M.force = {M.comb_value: [32, 31], M.big: [65534], comb: [32]}
    return M


def _cascade_holes(rng):
    M = Setup(1, (1024, 2048))
    f0 = draw_floor(M, rng, 9, 1, [2, 3], [1, 0])
    f1 = draw_floor(M, rng, 10, 4, [4, 1, 2], [0, 2, 1])
    holes = {0: value_book(M, rng, 8, kind="lattice"), 2: value_book(M, rng, 5, kind="list1"), 5: value_book(M, rng, 7, kind="list2"), 7: value_book(M, rng, 1, kind="lattice")}
    # begin 16, end 900: one partition of 280 in a short block (its end clipped to 512), three in a long one (end < 1024)
    r = M.residue(1, 16, 900, 280, phrase_book(M, rng, 3, 2), [holes, {0: value_book(M, rng, 2, kind="list1_seq")}, {}])
    M.modes(M.mapping([(f0, r)]), M.mapping([(f1, r)]))
    return M


def posts65():
    """the narrowest setup with a floor of all 65 posts (VAMD_POSIT): mono, one mode, 128 / 128"""
    rng = np.random.default_rng(65)
    M = Setup(1, (128, 128))
    book = M.book(flat(8))
    f = M.floor(6, 1, [(8, 0, None, [book]), (7, 0, None, [book])], [0] * 7 + [1], rng.permutation(np.arange(1, 64)))
    r = M.residue(1, 0, 64, 8, M.book(flat(2)), [{}, {0: M.book(lattice(flat(9, 2)))}])
    M.modes(M.mapping([(f, r)]))
    return M


CASES = {"equal_64_one_mode": _equal_64_one_mode, "equal_2048": _equal_2048, "one_mode_short": _one_mode_short, "far_64_4096": _far_64_4096,
         "eight_ch_max": _eight_ch_max, "floor_shapes": _floor_shapes, "book_shapes": _book_shapes, "cascade_holes": _cascade_holes}


# ---- the seeded family ----
def _divisors(n, top):
    return [d for d in range(1, top + 1) if n % d == 0]


def random_setup(seed):
    """A setup drawn inside the limits of header_build_image: 1 .. 8 channels; one or two submaps; up to 4 coupling steps;
    one mode (a seed in five) or two; any block-size pair of 64 .. 4096, equal ones every fourth seed; floors with a range
    up to half the block, of 2 .. 50 posts in up to 6 classes with up to 3 sub-class bits, or (one in four, where the range
    holds them) of all 65 posts in up to 16 classes; residues of type 1 and 2 with any begin and an end inside or beyond the
    span, up to 8 stages, at most 512 slots a block, 2 .. 5 classes or (one in four) 6 .. 64 -- all 64 in seeds 5, 13, 21 --, phrase words of up to 16
    dimensions from books of up to 4 096 entries, value books of under 150 entries or (one in eight) up to 2 000.  What the
    family leaves to the named cases: books of 65 535 / 65 536 entries and 32-bit codewords outside floors."""
    rng = np.random.default_rng(1000 + seed)
    ch = int(rng.integers(1, 9))
    b0 = int(rng.integers(6, 13))
    b1 = int(rng.integers(b0, 13)) if seed % 4 else b0
    M = Setup(ch, (1 << b0, 1 << b1), rate=int(rng.choice([8000, 22050, 44100, 48000, 192000])))
    nmodes = 1 if seed % 5 == 3 else 2
    submaps = 2 if ch >= 2 and rng.integers(0, 2) else 1
    mux = None
    if submaps == 2:
        mux = [int(v) for v in rng.integers(0, 2, ch)]
        mux[int(rng.integers(0, ch))] = 0
        mux[(mux.index(0) + 1 + int(rng.integers(0, ch - 1))) % ch] = 1
    coupling = []
    for _ in range(int(rng.integers(0, 5)) if ch >= 2 else 0):
        a, b = (int(v) for v in rng.choice(ch, 2, replace=False))
        coupling.append((a, b))
    maps = []
    for W in range(nmodes):
        n2 = M.bs[W] // 2
        subs = []
        for sm in range(submaps):
            bundle = ch if mux is None else mux.count(sm)
            rangebits = int(rng.integers(max(4, ilog(n2) - 4), ilog(n2)))  # 1 << rangebits <= n2
            mult = int(rng.integers(1, 5))
            if rangebits >= 6 and rng.integers(0, 4) == 0:  # all 63 places behind the end posts, in 8 .. 16 classes
                dims = [int(v) for v in rng.integers(1, 9, int(rng.integers(8, 17)))]
                while sum(dims) > 63:
                    dims[dims.index(max(dims))] -= 1
                while sum(dims) < 63:
                    dims[dims.index(min(dims))] += 1
                f = draw_floor(M, rng, rangebits, mult, dims, [int(v) for v in rng.integers(0, 2, len(dims))])
            else:
                dims = [int(rng.integers(1, 9)) for _ in range(int(rng.integers(0, 7)))]
                while sum(dims) > min(63, (1 << rangebits) - 1):
                    dims.pop()
                f = draw_floor(M, rng, rangebits, mult, dims) if dims else M.floor(rangebits, mult, [], [], [])
            kind = int(rng.integers(1, 3))
            span = n2 * bundle if kind == 2 else n2
            unit = bundle if kind == 2 else 1
            streams = 1 if kind == 2 else bundle
            least = -(-span // (512 // streams))  # the smallest partition size that keeps the slots at 512
            grouping = unit * int(rng.integers(-(-least // unit), max(-(-least // unit), min(32, span // unit // 2)) + 1))
            begin = unit * int(rng.integers(0, (span - grouping) // unit // 3 + 1))
            end = begin + grouping + int(rng.integers(0, span)) if rng.integers(0, 3) else span + int(rng.integers(0, 999))
            full = seed % 8 == 5 and (W, sm) == (0, 0)  # all 64 classes: in one residue of seeds 5, 13 and 21
            many = full or rng.integers(0, 4) == 0
            nclasses = 64 if full else int(rng.integers(6, 65)) if many else int(rng.integers(2, 6))
            pdim = int(rng.integers(1, min(16, int(np.log(4096) / np.log(nclasses) + 1e-9)) + 1))
            pool, classes = {}, []
            for _ in range(nclasses):
                stages = [s for s in range(8) if rng.integers(0, 12 if many else 4) == 0]
                books = {}
                for s in stages:
                    dim = int(rng.choice(_divisors(grouping, 8)))
                    if many:  # (255 books a setup: the many classes share a book per dimension)
                        if dim not in pool:
                            pool[dim] = value_book(M, rng, dim)
                        books[s] = pool[dim]
                    else:
                        books[s] = value_book(M, rng, dim, int(rng.integers(150, 2001)) if rng.integers(0, 8) == 0 else None)
                classes.append(books)
            subs.append((f, M.residue(kind, begin, end, grouping, phrase_book(M, rng, nclasses, pdim), classes)))
        maps.append(M.mapping(subs, mux, coupling))
    M.modes(*maps)
    return M


class Case:
    """headers; M (the Setup: .S, .bs, .channels); streams [[packet]]; notes [[packet_writer's record]] beside them;
    wanted: what the reference decodes a stream of its packets to (reference(), below), kept with the case"""

    def __init__(self, name, M, seed, nstreams=STREAMS):
        self.name, self.M, self.headers, self.wanted = name, M, M.headers(), {}
        self.bs, self.channels = M.bs, M.channels
        rng = np.random.default_rng(seed)
        force = {k: list(v) for k, v in getattr(M, "force", {}).items()}
        self.streams, self.notes = [], []
        for s in range(nstreams):
            count = int(rng.integers(10, 15))
            modes = packet_writer.mode_plan(len(M.S["modes"]), count, rng)
            notes = [packet_writer.write_packet(M.S, M.bs, rng, mode, flags, force) for mode, flags in modes]
            self.streams.append([n["packet"] for n in notes]), self.notes.append(notes)
        assert not any(force.values()), force

    def W(self, note):
        return self.M.S["modes"][note["mode"]][0]

    def size_classes(self, s):
        return [self.W(n) for n in self.notes[s]]

    def centres(self, s):
        Ws, out = self.size_classes(s), [0]
        for a, b in zip(Ws[:-1], Ws[1:]):
            out.append(out[-1] + self.bs[a] // 4 + self.bs[b] // 4)
        return out


def case(name):
    if name not in _memo:
        _memo[name] = Case(name, CASES[name](np.random.default_rng(sorted(CASES).index(name))), 100 + sorted(CASES).index(name))
    return _memo[name]


NAMES = tuple(CASES)


def get(name):
    """a named case, or "seed<k>" of the seeded family"""
    return seeded(int(name[4:])) if name.startswith("seed") else case(name)


def seeded(seed):
    if ("seed", seed) not in _memo:
        _memo["seed", seed] = Case("seed%d" % seed, random_setup(seed), 500 + seed, nstreams=2)
    return _memo["seed", seed]


# ---- what the cases are held to, and the keep policy's cuts ----
def reference(c, packets):
    """libvorbis' decoder over a stream of a Case's packets under its headers, no end granule; once per stream, read-only"""
    from tests import ref_host
    key = tuple(packets)
    if key not in c.wanted:
        w = ref_host.reference_decode(list(c.headers) + list(packets), [-1] * len(packets))
        w.setflags(write=False)
        c.wanted[key] = w
    return c.wanted[key]


def keep_streams(c, every=200, seeded_cuts=24):
    """The keep policy's streams of a Case: its longest short and its longest long packet, each cut at every byte (packets
    of up to `every` bytes) or at `seeded_cuts` seeded bytes and just inside its floors, its phrase words and its residue
    entries (the writer's section offsets); every cut between two whole packets, as a stream of its own"""
    notes = [n for row in c.notes for n in row]
    picks = [max((n for n in notes if c.W(n) == W), key=lambda n: n["bits"], default=None) for W in (0, 1)]
    anchor = max(notes, key=lambda n: n["bits"])["packet"]
    streams = []
    for n in picks:
        if n is None or len(n["packet"]) < 2:
            continue
        p = n["packet"]
        if len(p) <= every:
            cuts = range(1, len(p))
        else:
            rng = np.random.default_rng(len(p))
            inside = [at // 8 + 1 for at in n["at"].values() if at is not None]
            cuts = sorted({int(v) for v in rng.integers(1, len(p), seeded_cuts)} | {v for v in inside if 1 <= v < len(p)})
        streams += [[anchor, p[:k], anchor] for k in cuts]
    assert streams
    return streams


# ---- the one-lane host build of the default policy ----
def host_decode(exe, tmp, c, streams):
    """tests/c/decode_headers_host.cpp's `streams` over a Case's headers -> ([(status, pcm)], lattice books, value-list
    books); a setup the library refuses fails here, with the library's reason.  host_decode.lds: the program's second line
    of the last run, (k_synth's LDS bytes per size class, res_off_ints per size class)"""
    from tests.unpack_host import _streams_job
    paths = {}
    for name, data in (("id", c.headers[0]), ("setup", c.headers[2])):
        paths[name] = os.path.join(str(tmp), name)
        with open(paths[name], "wb") as f:
            f.write(bytes(data))
    out = os.path.join(str(tmp), "streams.out")
    r = subprocess.run([exe, "streams", paths["id"], paths["setup"], _streams_job(tmp, streams, [-1] * len(streams)), out], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (c.name, r.stdout[-3000:] + r.stderr[-4000:])
    raw, at, res = np.fromfile(out, np.int32), 0, []
    for _ in streams:
        status, frames = int(raw[at]), int(raw[at + 1])
        res.append((status, raw[at + 2:at + 2 + c.channels * frames].view(np.float32).reshape(c.channels, frames)))
        at += 2 + c.channels * frames
    assert at == raw.size
    words = r.stdout.split()
    lattice, table = (int(v) for v in words[1:3])
    assert words[3] == "lds" and words[6] == "off", words[:9]
    host_decode.lds = ((int(words[4]), int(words[5])), (int(words[7]), int(words[8])))
    return res, lattice, table


def synth_lds_bytes(ch, n2, off_ints):
    """An independent expectation of k_synth.h's synth_lds_words(ch, n2, ch waves, off_ints), in bytes: the spectrum, then
    the larger of a butterfly vector per wave (n2 + n2 / 16 floats, rounded up to 4) and the residue walk's tables (8
    channel slots + 512 class slots + 2 off_ints ints), rounded up to 4 words"""
    a, b = ch * ((n2 + (n2 >> 4) + 3) & ~3), 8 + 512 + 2 * off_ints
    return 4 * (ch * n2 + ((max(a, b) + 3) & ~3))
