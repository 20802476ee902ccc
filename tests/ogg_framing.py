"""The oracle for the Ogg CONTAINER and the paging policy, independent of vorbis_amd/csrc/k_ogg.h (this module imports
nothing that was compiled from it).

* From doc/framing.html alone: a bit-serial CRC, the byte table derived from it, and one page reader (capture pattern,
  version, flags, granule position, serial, sequence number, checksum, lacing).  pages_of reads a PIECE of a file: whole
  pages, free to begin with a continued packet and to end inside one.  demux reads a whole file and puts its packets
  together again; Reassembler does that across pieces.  The continued flag must agree with "a packet is open".
* From the policy text of include/vorbis_amd.h ("the Ogg feed", "a flush per write"): the page-level rules over a read
  file (check_policy), and a second implementation of the paging with flush points, a segment at a time, from sizes and
  granule positions alone (PolicyModel)."""
import struct

FILL, MIN_PACKETS = 4096, 4  # the paging policy (include/vorbis_amd.h, "the Ogg feed")


# ---- from framing.html ----
def crc_bitserial(data):
    """polynomial 0x04c11db7, initial value 0, no final XOR, most significant bit first, one bit at a time"""
    r = 0
    for b in bytes(data):
        r ^= b << 24
        for _ in range(8):
            r = ((r << 1) ^ 0x04c11db7) & 0xffffffff if r & 0x80000000 else (r << 1) & 0xffffffff
    return r


_TABLE = [crc_bitserial(bytes([i])) for i in range(256)]  # the bit-serial definition, a byte at a time
_verified = set()


def _crc(data):
    r = 0
    for b in data:
        r = ((r << 8) & 0xffffffff) ^ _TABLE[(r >> 24) ^ b]
    return r


def _read(f, whole):
    """The page reader.  Per page its fields, how many packets it completes (`done`), `open` (its last lacing value is
    255), where it lies, its lacing values and its body."""
    what = "file" if whole else "the piece"
    pos, pages = 0, []
    while pos < len(f):
        assert f[pos:pos + 4] == b"OggS", "capture pattern at %d" % pos
        assert f[pos + 4] == 0, "stream structure version"
        assert len(f) >= pos + 27
        flags = f[pos + 5]
        gp, serial, seq, crc = struct.unpack("<qIII", f[pos + 6:pos + 26])
        n = f[pos + 26]
        lacing = list(f[pos + 27:pos + 27 + n])
        assert len(lacing) == n, "%s ends inside a lacing table" % what
        end = pos + 27 + n + sum(lacing)
        assert end <= len(f), "%s ends inside a page body" % what
        page = f[pos:end]
        if page not in _verified:  # (the same page comes back under every cut)
            assert _crc(page[:22] + b"\0\0\0\0" + page[26:]) == crc, \
                "checksum of page %d" % len(pages) if whole else "checksum of the page at %d" % pos
            _verified.add(page)
        assert not flags & ~7
        pages.append(dict(flags=flags, granule=gp, serial=serial, seq=seq, nseg=n, body=sum(lacing), done=sum(v < 255 for v in lacing),
                          open=bool(lacing) and lacing[-1] == 255, offset=pos, bytes=end - pos, lacing=lacing, data=page[27 + n:]))
        pos = end
    return pages


def pages_of(piece):
    """-> the pages of a piece of a file: it must be a whole number of well-formed pages, each with a correct checksum.
    Unlike demux it may begin with a continued packet and end inside one."""
    return _read(bytes(piece), False)


class Reassembler:
    """The packets a stream's pages (pages_of) complete, page after page; `open` the bytes of a packet not yet completed.
    The continued flag must agree with it (check=False: a run of pages from anywhere in a stream)."""

    def __init__(self, check=True):
        self.packets, self.open, self.is_open, self.check = [], b"", False, check

    def take(self, pages):
        for p in pages:
            if self.check:
                assert bool(p["flags"] & 1) == self.is_open, "continued flag of page %d" % p["seq"]
            o = 0
            for v in p["lacing"]:
                self.open += p["data"][o:o + v]
                o += v
                self.is_open = True
                if v < 255:
                    self.packets.append(self.open)
                    self.open, self.is_open = b"", False


def packets_of(pages):
    """-> the packets a run of pages (pages_of) completes, put together again; what an open last packet holds is dropped"""
    r = Reassembler(check=False)
    r.take(pages)
    return r.packets


def demux(f):
    """-> (pages, packets): every page's fields (and how many packets it completes), the packets put together again.
    Asserts what framing.html asks of a well-formed single stream."""
    pages, r = _read(bytes(f), True), Reassembler()
    r.take(pages)
    assert not r.is_open, "the file ends inside a packet"
    return pages, r.packets


def page_granules(pages, npackets, nheaders=3):
    """Per audio packet the granule position a demuxer can give a decoder: the page's, on the last packet the page
    completes; -1 elsewhere."""
    out = [-1] * npackets
    k = -nheaders
    for p in pages:
        k += p["done"]
        if p["done"] and k > 0:
            out[k - 1] = p["granule"]
    return out


# ---- from the policy text ----
def check_policy(pages, first_audio_page):
    """The policy's page-level rules over a demuxed file's audio pages (or a bare run's pages)."""
    audio = pages[first_audio_page:]
    for i, p in enumerate(audio):
        assert 1 <= p["nseg"] <= 255
        if i + 1 < len(audio):
            assert (p["body"] > FILL and p["done"] >= MIN_PACKETS) or p["nseg"] == 255, (i, _fields(p))
        assert bool(p["flags"] & 4) == (i + 1 == len(audio)), (i, _fields(p))
        if p["done"] == 0:
            assert p["granule"] == -1
    for i, p in enumerate(pages):
        assert p["seq"] == i


def _fields(p):
    return {k: v for k, v in p.items() if k not in ("lacing", "data")}


class PolicyModel:
    """The pages of one stream from packet sizes and granule positions, by the words of include/vorbis_amd.h: a packet of
    n bytes is n / 255 lacing values of 255 and one of n % 255; segments are taken in order; before a segment is taken
    the page is closed if it holds 255 segments; at a packet boundary it is closed once its body holds more than 4096
    bytes and at least four packets have been completed on it; the end of a run closes its page; a flush closes the open
    page if it holds a segment; flags 0x01 / 0x02 / 0x04; a page's granule position is that of the last packet completed
    on it, -1 if none.  group(...) -> the pages that group hands out, each a dict(nseg, body, done, flags, granule, seq,
    flushed)."""

    def __init__(self, header_bytes):
        self.header_bytes, self.seq, self.begun = header_bytes, 0, False
        self._fresh(0)

    def _fresh(self, flags):
        self.lacing, self.done, self.granule, self.flags = [], 0, -1, flags

    def _close(self, out, extra=0, flushed=False):
        out.append(dict(nseg=len(self.lacing), body=sum(self.lacing), done=self.done, flags=self.flags | extra, granule=self.granule,
                        seq=self.seq, flushed=flushed))
        self.seq += 1
        self._fresh(0)

    def _packet(self, out, n, granule):
        if self.lacing and sum(self.lacing) > FILL and self.done >= MIN_PACKETS:
            self._close(out)
        values = [255] * (n // 255) + [n % 255]
        for q, v in enumerate(values):
            if len(self.lacing) == 255:
                self._close(out)
            if not self.lacing and q:
                self.flags |= 1
            self.lacing.append(v)
        self.done, self.granule = self.done + 1, granule

    def _end_run(self, out, eos):
        if self.lacing:
            self._close(out, 4 if eos else 0)

    def group(self, sizes, granules, close, flush):
        out = []
        if not self.begun:
            self.begun, self.seq = True, 0
            if self.header_bytes is not None:
                self._fresh(2)
                self._packet(out, self.header_bytes[0], 0)
                self._end_run(out, False)
                self._packet(out, self.header_bytes[1], 0)
                self._packet(out, self.header_bytes[2], 0)
                self._end_run(out, False)
            self._fresh(0)
        for n, g in zip(sizes, granules):
            self._packet(out, n, g)
        if close:
            self._end_run(out, True)
            self.begun = False
        elif flush and self.lacing:
            self._close(out, flushed=True)
        return out
