"""Setup headers no encoder here wrote, for the header-made decoder's tests (tests/test_decode_headers_cpu.py,
tests/test_decode_headers_gpu.py): a bit reader / writer for the Vorbis I setup header (4.2.4), written from the format,
that takes a genuine header (ref_host.encoder_headers) apart and puts it together again with ONE thing changed.  The code
trees are never touched, so the stream's genuine packets stay parseable under every variant and the reference decodes each of
them: what a variant is held to is ref_host.reference_decode under the changed headers, nothing of the code under test.

  identity   re-emitted as parsed: byte for byte the original (this checks the helper)
  cover      books rewritten into another of the three length encodings (ordered, unordered, unordered with unused
             entries), lengths unchanged: decodes as the original.  The genuine headers of the tests' setups hold all
             three between them (assert_encodings); this moves them to other books
  explicit   every lookup-1 residue book as lookup type 2, the same multiplicands written out per entry: the same values
  scaled     q_delta of every residue book 0.75 x, q_min moved by 0.5: non-integer values
  sequence   q_sequencep set on the residue books of one class
  permuted   one lookup-1 residue book's quantlist in reverse order
  small_blocks()  a setup of block sizes 64 and 128 whose floors read two posts through a single-entry book (one codeword of
             one bit, which the reference reads from a bit of either value), with packets of random bits behind their mode bits
and three that are to be refused:  modes3 (a third mode appended), residue0 (a residue's type field 0), and ident_8192()
(the long block size 8192 in the identification header)."""
import math

VARIANTS = ("identity", "cover", "explicit", "scaled", "sequence", "permuted")
SHAPES = ("modes3", "residue0")
# setups no blob is shipped for: one more per rate family of lib/modes/setup_*.h that checker.ENCODERS does not touch, and a
# 3-channel one -- (channels, rate, quality) of ref.RefEncoder
EXTRA = {"11k_mono_q3": (1, 11025, .3), "16k_stereo_q5": (2, 16000, .5), "22k_stereo_q6": (2, 22050, .6), "32k_stereo_q7": (2, 32000, .7),
         "48k_stereo_q7": (2, 48000, .7), "96k_mono_q4": (1, 96000, .4), "44k_3ch_q5": (3, 44100, .5)}


def encoder(name):
    """the reference encoder of a setup of EXTRA or of checker.ENCODERS"""
    from oracle import ref
    from tests import ref_host
    return ref.RefEncoder(*EXTRA[name]) if name in EXTRA else ref_host.encoder(name)


def ilog(v):
    return int(v).bit_length()


class Bits:
    def __init__(self, data=b""):
        self.v, self.pos, self.n = int.from_bytes(data, "little"), 0, 8 * len(data)

    def read(self, bits):
        assert self.pos + bits <= self.n, "the header ends early"
        r = (self.v >> self.pos) & ((1 << bits) - 1)
        self.pos += bits
        return r

    def write(self, value, bits):
        assert 0 <= value < (1 << bits) or bits == 0, (value, bits)
        self.v |= value << self.pos
        self.pos += bits

    def bytes(self):
        return self.v.to_bytes((self.pos + 7) // 8, "little")


def lookup1_values(dim, entries):
    v = int(math.floor(entries ** (1.0 / dim)))
    while v ** dim > entries:
        v -= 1
    while (v + 1) ** dim <= entries:
        v += 1
    return v


def float32_unpack(x):
    mant, exp = x & 0x1fffff, (x >> 21) & 0x3ff
    return math.ldexp(-mant if x & 0x80000000 else mant, exp - 788)


def float32_pack(val):
    """exact for the values the variants make (a few bits of mantissa)"""
    if val == 0:
        return 0
    sign, val = (0x80000000, -val) if val < 0 else (0, val)
    exp = int(math.floor(math.log2(val)))
    mant = math.ldexp(val, 20 - exp)
    assert mant == int(mant) and int(mant) < (1 << 21), val
    out = sign | ((exp + 768) << 21) | int(mant)
    assert float32_unpack(out) == (-val if sign else val)
    return out


# ---- parse ----
def _book(b):
    assert b.read(24) == 0x564342
    c = dict(dim=b.read(16), entries=b.read(24))
    n = c["entries"]
    if b.read(1):
        c["enc"], length, lens = "ordered", b.read(5) + 1, []
        while len(lens) < n:
            lens += [length] * b.read(ilog(n - len(lens)))
            length += 1
    elif b.read(1):
        c["enc"], lens = "sparse", [b.read(5) + 1 if b.read(1) else 0 for _ in range(n)]
    else:
        c["enc"], lens = "plain", [b.read(5) + 1 for _ in range(n)]
    c["lengths"] = lens
    c["maptype"] = b.read(4)
    if c["maptype"]:
        c["q_min"], c["q_delta"], c["q_bits"], c["q_seq"] = b.read(32), b.read(32), b.read(4) + 1, b.read(1)
        count = lookup1_values(c["dim"], n) if c["maptype"] == 1 else n * c["dim"]
        c["quant"] = [b.read(c["q_bits"]) for _ in range(count)]
    return c


def _floor1(b):
    f = dict(classes=[b.read(4) for _ in range(b.read(5))], cls=[])
    for _ in range(max(f["classes"], default=-1) + 1):
        c = dict(dim=b.read(3) + 1, subs=b.read(2))
        c["book"] = b.read(8) if c["subs"] else None
        c["subbooks"] = [b.read(8) for _ in range(1 << c["subs"])]
        f["cls"].append(c)
    f["mult"], f["rangebits"] = b.read(2), b.read(4)
    f["x"] = [b.read(f["rangebits"]) for _ in range(sum(f["cls"][c]["dim"] for c in f["classes"]))]
    return f


def _residue(b):
    r = dict(type=b.read(16), begin=b.read(24), end=b.read(24), grouping=b.read(24), groupbook=None, cascade=[])
    nparts = b.read(6) + 1
    r["groupbook"] = b.read(8)
    for _ in range(nparts):
        low, flag = b.read(3), b.read(1)
        r["cascade"].append((low, flag, b.read(5) if flag else 0))
    r["books"] = [b.read(8) for _ in range(sum(bin(low | high << 3).count("1") for low, _, high in r["cascade"]))]
    return r


def _mapping(b, channels):
    assert b.read(16) == 0
    m = dict(submaps=b.read(4) + 1 if b.read(1) else None, coupling=None)
    if b.read(1):
        w = ilog(channels - 1)
        m["coupling"] = [(b.read(w), b.read(w)) for _ in range(b.read(8) + 1)]
    assert b.read(2) == 0
    n = m["submaps"] or 1
    m["mux"] = [b.read(4) for _ in range(channels)] if n > 1 else None
    m["sub"] = [(b.read(8), b.read(8), b.read(8)) for _ in range(n)]
    return m


def parse(setup, channels):
    b = Bits(setup)
    assert b.read(8) == 5 and bytes(b.read(8) for _ in range(6)) == b"vorbis"
    S = dict(channels=channels)
    S["books"] = [_book(b) for _ in range(b.read(8) + 1)]
    S["times"] = [b.read(16) for _ in range(b.read(6) + 1)]
    S["floors"] = []
    for _ in range(b.read(6) + 1):
        assert b.read(16) == 1
        S["floors"].append(_floor1(b))
    S["residues"] = [_residue(b) for _ in range(b.read(6) + 1)]
    S["maps"] = [_mapping(b, channels) for _ in range(b.read(6) + 1)]
    S["modes"] = [(b.read(1), b.read(16), b.read(16), b.read(8)) for _ in range(b.read(6) + 1)]
    assert b.read(1) == 1 and b.n - b.pos < 8 and b.read(b.n - b.pos) == 0
    return S


# ---- emit ----
def _emit_book(b, c):
    b.write(0x564342, 24), b.write(c["dim"], 16), b.write(c["entries"], 24)
    lens, n = c["lengths"], c["entries"]
    if c["enc"] == "ordered":
        assert all(v > 0 for v in lens) and lens == sorted(lens)
        b.write(1, 1), b.write(lens[0] - 1, 5)
        done, length = 0, lens[0]
        while done < n:
            k = lens.count(length)
            b.write(k, ilog(n - done))
            done, length = done + k, length + 1
    elif c["enc"] == "sparse":
        b.write(0, 1), b.write(1, 1)
        for v in lens:
            b.write(1 if v else 0, 1)
            if v:
                b.write(v - 1, 5)
    else:
        assert all(v > 0 for v in lens)
        b.write(0, 1), b.write(0, 1)
        for v in lens:
            b.write(v - 1, 5)
    b.write(c["maptype"], 4)
    if c["maptype"]:
        b.write(c["q_min"], 32), b.write(c["q_delta"], 32), b.write(c["q_bits"] - 1, 4), b.write(c["q_seq"], 1)
        assert len(c["quant"]) == (lookup1_values(c["dim"], n) if c["maptype"] == 1 else n * c["dim"])
        for q in c["quant"]:
            b.write(q, c["q_bits"])


def emit(S):
    b = Bits()
    b.write(5, 8)
    for ch in b"vorbis":
        b.write(ch, 8)
    b.write(len(S["books"]) - 1, 8)
    for c in S["books"]:
        _emit_book(b, c)
    b.write(len(S["times"]) - 1, 6)
    for t in S["times"]:
        b.write(t, 16)
    b.write(len(S["floors"]) - 1, 6)
    for f in S["floors"]:
        b.write(1, 16), b.write(len(f["classes"]), 5)
        for c in f["classes"]:
            b.write(c, 4)
        for c in f["cls"]:
            b.write(c["dim"] - 1, 3), b.write(c["subs"], 2)
            if c["subs"]:
                b.write(c["book"], 8)
            for s in c["subbooks"]:
                b.write(s, 8)
        b.write(f["mult"], 2), b.write(f["rangebits"], 4)
        for x in f["x"]:
            b.write(x, f["rangebits"])
    b.write(len(S["residues"]) - 1, 6)
    for r in S["residues"]:
        b.write(r["type"], 16), b.write(r["begin"], 24), b.write(r["end"], 24), b.write(r["grouping"], 24)
        b.write(len(r["cascade"]) - 1, 6), b.write(r["groupbook"], 8)
        for low, flag, high in r["cascade"]:
            b.write(low, 3), b.write(flag, 1)
            if flag:
                b.write(high, 5)
        for k in r["books"]:
            b.write(k, 8)
    b.write(len(S["maps"]) - 1, 6)
    for m in S["maps"]:
        b.write(0, 16)
        b.write(1 if m["submaps"] else 0, 1)
        if m["submaps"]:
            b.write(m["submaps"] - 1, 4)
        b.write(1 if m["coupling"] else 0, 1)
        if m["coupling"]:
            b.write(len(m["coupling"]) - 1, 8)
            w = ilog(S["channels"] - 1)
            for mag, ang in m["coupling"]:
                b.write(mag, w), b.write(ang, w)
        b.write(0, 2)
        for v in m["mux"] or ():
            b.write(v, 4)
        for t, f, r in m["sub"]:
            b.write(t, 8), b.write(f, 8), b.write(r, 8)
    b.write(len(S["modes"]) - 1, 6)
    for flag, window, transform, mapping in S["modes"]:
        b.write(flag, 1), b.write(window, 16), b.write(transform, 16), b.write(mapping, 8)
    b.write(1, 1)
    return b.bytes()


# ---- the variants ----
def residue_books(S):
    return sorted({k for r in S["residues"] for k in r["books"]})


def encodings(S):
    return {c["enc"] for c in S["books"]}


def assert_encodings(all_headers):
    """the genuine headers of the tests' setups hold, between them, a book in each of the three length encodings"""
    seen = set()
    for h in all_headers:
        seen |= encodings(parse(bytes(h[2]), h[0][11]))
    assert seen == {"ordered", "plain", "sparse"}, seen


def _cover(S):
    """books written in ANOTHER length encoding, the lengths as they are: a book without unused entries with a flag per
    entry (and one that has the flags without them); an ordered book entry by entry, and a book whose lengths do not
    decrease as an ordered one, where the setup has such books"""
    books = S["books"]
    full = [c for c in books if all(v > 0 for v in c["lengths"])]
    plain = [c for c in full if c["enc"] == "plain"]
    assert plain, "no book to rewrite"
    plain[0]["enc"] = "sparse"
    for c in full:
        if c["enc"] == "sparse" and c is not plain[0]:
            c["enc"] = "plain"
            break
    ordered = [c for c in full if c["enc"] == "ordered"]
    for c in ordered[:1]:
        c["enc"] = "plain"
    for c in full:
        if c["enc"] != "ordered" and c not in ordered[:1] and c is not plain[0] and c["lengths"] == sorted(c["lengths"]):
            c["enc"] = "ordered"
            break


def variant(headers, kind):
    """[identification, comment, setup] of a genuine stream -> the same with the setup header changed as `kind` names"""
    ident, comment, setup = (bytes(h) for h in headers)
    S = parse(setup, ident[11])
    books = S["books"]
    rb = residue_books(S)
    lookup1 = [k for k in rb if books[k]["maptype"] == 1]
    if kind == "identity":
        pass
    elif kind == "cover":
        _cover(S)
    elif kind == "explicit":
        assert lookup1
        for k in lookup1:
            c = books[k]
            qv = len(c["quant"])
            c["quant"] = [c["quant"][(e // qv ** d) % qv] for e in range(c["entries"]) for d in range(c["dim"])]
            c["maptype"] = 2
    elif kind == "scaled":
        for k in rb:
            c = books[k]
            c["q_delta"] = float32_pack(0.75 * float32_unpack(c["q_delta"]))
            c["q_min"] = float32_pack(float32_unpack(c["q_min"]) + 0.5)
    elif kind == "sequence":
        r = max(S["residues"], key=lambda r: len(r["books"]))
        at, mine = 0, None
        for low, _, high in r["cascade"]:  # the books of the first class that has one of two dimensions or more (with one, the flag changes nothing)
            n = bin(low | high << 3).count("1")
            if mine is None and any(books[k]["dim"] > 1 for k in r["books"][at:at + n]):
                mine = r["books"][at:at + n]
            at += n
        assert mine
        for k in set(mine):
            books[k]["q_seq"] = 1
    elif kind == "permuted":
        # (the first residue book of two dimensions or more: of the class the streams use most)
        c = books[next(k for r in S["residues"] for k in r["books"] if books[k]["maptype"] == 1 and books[k]["dim"] > 1)]
        assert len(set(c["quant"])) > 1
        c["quant"] = c["quant"][::-1]
    elif kind == "modes3":
        S["modes"].append(S["modes"][0])
    elif kind == "residue0":
        S["residues"][0]["type"] = 0
    else:
        raise ValueError(kind)
    out = emit(S)
    if kind == "identity":
        assert out == setup, "the helper does not re-emit a header as it parsed it"
    else:
        assert out != setup, kind
    return [ident, comment, out]


def ident_8192(headers):
    """the long block size raised to 8192 in the identification header"""
    ident = bytearray(headers[0])
    ident[28] = (ident[28] & 15) | (13 << 4)
    return [bytes(ident), bytes(headers[1]), bytes(headers[2])]


def small_blocks(headers, seed=1, nstreams=4, npackets=14, packet_bytes=900):
    """Block sizes 64 and 128 and a single-entry book, which no encoder here produces: the genuine stereo setup with the two
    block sizes written into the identification header, a book of one entry of length 1 appended, and each floor replaced by
    one of the block's own range (1 << 5, 1 << 6) with two partitions -- two posts read through the single-entry book, one
    through a genuine floor book.  The residues stay (their ranges are held to the block by every decoder).  The packets
    are random bits behind an audio packet's type bit and a random mode bit, long enough that no decoder meets their end:
    every codebook here is a complete tree, so any bits decode.  -> (headers, [packets] per stream)"""
    import numpy as np
    ident, comment, setup = (bytes(h) for h in headers)
    S = parse(setup, ident[11])
    assert len(S["modes"]) == 2 and len(S["floors"]) == 2
    S["books"].append(dict(dim=1, entries=1, enc="plain", lengths=[1], maptype=0))
    single = len(S["books"]) - 1
    for k, f in enumerate(S["floors"]):
        genuine = next(b for c in f["cls"] for b in c["subbooks"] if b > 0)  # (as written: the book's number + 1)
        bits = 5 + k
        S["floors"][k] = dict(classes=[0, 1], cls=[dict(dim=2, subs=0, book=None, subbooks=[single + 1]), dict(dim=1, subs=0, book=None, subbooks=[genuine])],
                              mult=f["mult"], rangebits=bits, x=[(1 << bits) // 4, (1 << bits) // 2 + 3, 5])
    ident = bytearray(ident)
    ident[28] = 6 | (7 << 4)
    rng = np.random.default_rng(seed)
    streams = []
    for _ in range(nstreams):
        packets = []
        for _ in range(npackets):
            p = bytearray(rng.integers(0, 256, packet_bytes, dtype=np.uint8).tobytes())
            p[0] &= 0xfe
            packets.append(bytes(p))
        streams.append(packets)
    return [bytes(ident), comment, emit(S)], streams
