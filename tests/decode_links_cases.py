"""Files and mark lists for the tests of the reader's bookkeeping (vamd_decode_follow, vamd_decode_streams_marked:
tests/test_decode_links_cpu.py on the one-lane host build, tests/test_decode_links_gpu.py on the GPU): short streams of the
reference encoder; a page writer that sets serial, sequence, flags and granule per page, with tests/ogg_framing.py's CRC;
chained, multiplexed, trimmed, shifted and damaged files; and what each must decode to -- the reference decoder over what
an independent reader (tests/ogg_framing.py's pages, the link rules of include/vorbis_amd.h restated here) makes of the
file, with the e_o_s flags libogg would give.  Nothing here comes from the code under test.

Also the job files of tests/c/decode_links_host.cpp and a straight restatement of the granule walk (walk())."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from tests import hostbuild, ogg_framing, ref_host
from tests.ogg_demux_cases import STATUS_BADHEADER, STATUS_BADPAGE, packet_granules, page
from tests.signals import gated_noise

STEREO, MONO = "44k_stereo_q4", "44k_mono_q5"
SHIFT = 1000000
LENGTHS = (3500, 3400, 2450, 1500)  # 14, 14, 13 and 12 packets: eleven short blocks at the onset, then long ones; each last block cut
_streams, _files, _want, _same_as = {}, {}, {}, {}


# ---- the reference, with libogg's e_o_s per packet ----
def reference_decode(packets, granules, eos):
    """tests/ref_host.py's reference_decode with an e_o_s list: packets = the three headers, then the audio packets;
    granules[i] / eos[i] of audio packet i.  The caller drains after every packet.  -> float32 [channels, frames]"""
    L = ref_host._reflib()
    vi, vc = ref_host._headers_in(L, packets[:3])
    vd, vb = C.create_string_buffer(4096), C.create_string_buffer(4096)
    L.vorbis_synthesis_read.argtypes = [C.c_void_p, C.c_int]
    assert L.vorbis_synthesis_init(vd, vi) == 0
    L.vorbis_block_init(vd, vb)
    ch = C.cast(vi, C.POINTER(C.c_int))[1]  # vorbis_info.channels
    pcm = C.POINTER(ref_host._f32p)()
    out = [[np.zeros(0, np.float32)] for _ in range(ch)]
    for i in range(3, len(packets)):
        o = ref_host._op(packets[i], i, granules[i - 3], 1 if eos[i - 3] else 0)
        if L.vorbis_synthesis(vb, C.byref(o)) == 0:
            L.vorbis_synthesis_blockin(vd, vb)
        while True:
            n = L.vorbis_synthesis_pcmout(vd, C.byref(pcm))
            if n <= 0:
                break
            for c in range(ch):
                out[c].append(np.ctypeslib.as_array(pcm[c], (n,)).copy())
            L.vorbis_synthesis_read(vd, n)
    L.vorbis_block_clear(vb)
    L.vorbis_dsp_clear(vd)
    L.vorbis_comment_clear(vc)
    L.vorbis_info_clear(vi)
    return np.stack([np.concatenate(o) for o in out])


# ---- streams ----
class Stream:
    """a short stream of the reference encoder: headers, audio packets, the encoder's granule per packet, block sizes"""

    def __init__(self, name, frames, seed):
        e = ref_host.encoder(name)
        recs = e.encode_stream(gated_noise(e.channels, e.rate, frames, seed))
        self.name, self.channels = name, e.channels
        self.bs = (e.blocksize(0), e.blocksize(1))
        self.headers = ref_host.encoder_headers(ref_host.encoder(name))
        self.packets = [r["packet"] for r in recs]
        self.end = recs[-1]["granulepos"]
        self.Ws = [r["W"] for r in recs]
        self.granules = packet_granules(self.packets, self.end, self.bs)
        self.blob = e.pack_setup()
        steps = self.steps()
        assert 6 <= len(self.packets) <= 14 and set(self.Ws) == {0, 1}, (len(self.packets), self.Ws)
        assert sum(steps) > self.end > sum(steps[:-1]), "the last block is really cut"

    def steps(self):
        return [self.bs[self.Ws[i - 1]] // 4 + self.bs[self.Ws[i]] // 4 if i else 0 for i in range(len(self.Ws))]


def stream(name=STEREO, v=0):
    """stream v of a setup: lengths chosen so that 6 .. 14 packets of both block sizes come out and the last block is cut"""
    if (name, v) not in _streams:
        _streams[name, v] = Stream(name, LENGTHS[v], 40 + v)
    return _streams[name, v]


# ---- the page writer ----
def lacing(p):
    return [255] * (len(p) // 255) + [len(p) % 255]


def pages_of_packets(packets, granules, serial, seq0, groups, first_flags=0, eos=True):
    """whole packets, groups[i] of them on page i -> [page]; the page's granule is its last packet's; eos: the flag on the last"""
    out, at = [], 0
    for i, n in enumerate(groups):
        chunk = packets[at:at + n]
        flags = (first_flags if i == 0 else 0) | (4 if eos and i == len(groups) - 1 else 0)
        out.append(page(flags, granules[at + n - 1], serial, seq0 + i, [v for p in chunk for v in lacing(p)], b"".join(chunk)))
        at += n
    assert at == len(packets)
    return out


def logical(s, serial, groups=None, eos=True, seq0=0, granules=None, packets=None):
    """a stream as pages: the identification header alone on its begin-of-stream page, the comment and setup headers on
    the next, then the audio packets, groups[i] on audio page i (default: two a page)"""
    packets = s.packets if packets is None else packets
    granules = s.granules[:len(packets)] if granules is None else granules
    if groups is None:
        groups = [2] * (len(packets) // 2) + [1] * (len(packets) % 2)
    return (pages_of_packets(s.headers[:1], [0], serial, seq0, [1], 2, False) + pages_of_packets(s.headers[1:], [0, 0], serial, seq0 + 1, [2], 0, False) +
            (pages_of_packets(packets, granules, serial, seq0 + 2, groups, 0, eos) if packets else []))


def foreign(serial, n, seq0=0, bos=True, size=300):
    """n pages of a stream that is no Vorbis stream: one packet a page"""
    rng = np.random.default_rng(serial)
    out = []
    for i in range(n):
        body = b"fishead\0" + rng.integers(0, 256, size - 8, dtype=np.uint8).tobytes()
        out.append(page((2 if bos and i == 0 else 0) | (4 if i == n - 1 else 0), i, serial, seq0 + i, lacing(body), body))
    return out


def reseq(pg, seq=None, flags=None, granule=None):
    """a page with another sequence number, flags or granule position, sealed anew"""
    n = pg[26]
    return page(pg[5] if flags is None else flags, struct.unpack_from("<q", pg, 6)[0] if granule is None else granule,
                struct.unpack_from("<I", pg, 14)[0], struct.unpack_from("<I", pg, 18)[0] if seq is None else seq, list(pg[27:27 + n]), pg[27 + n:])


# ---- the independent reader ----
def read_links(f):
    """The link rules of include/vorbis_amd.h ("files as a reader takes them") over tests/ogg_framing.py's pages ->
    [(begin, end, serial or None, pages of that serial)]"""
    pages = ogg_framing.pages_of(f)
    links, run = [], False
    for i, p in enumerate(pages):
        bos = bool(p["flags"] & 2) or i == 0
        if bos and not run:
            if links:
                links[-1][1] = p["offset"]
            links.append([p["offset"], len(f), None, []])
            run = True
        if not bos:
            run = False
        if bos and links[-1][2] is None and p["data"][:7] == b"\x01vorbis":
            links[-1][2] = p["serial"]
        if links[-1][2] == p["serial"]:
            links[-1][3].append(p)
    return [tuple(x) for x in links]


def link_marks(pages):
    """a link's stream pages -> (packets, granules, eos) of its audio packets, as libogg hands them out"""
    r = ogg_framing.Reassembler()
    gran, eos = [], []
    for p in pages:
        before = len(r.packets)
        r.take([p])
        done = len(r.packets) - before
        gran += [-1] * done
        eos += [0] * done
        if done:
            gran[-1], eos[-1] = (p["granule"] if p["granule"] >= -1 else -1), (1 if p["flags"] & 4 else 0)
    assert not r.is_open
    return r.packets, gran[3:], eos[3:]


def expected(f):
    """what a well-formed file decodes to under the policy: per link the reference over its packets and marks, end to end
    -> (pcm, [per link pcm]); read-only, once per file"""
    f = _same_as.get(bytes(f), bytes(f))  # (a file whose damage a reader passes over: what the undamaged file decodes to)
    if f not in _want:
        parts = []
        for _, _, serial, pages in read_links(f):
            assert serial is not None
            packets, gran, eos = link_marks(pages)
            parts.append(reference_decode(packets, gran, eos) if len(packets) > 3 else np.zeros((packets[0][11], 0), np.float32))
        whole = None  # (links of differing channel counts have no signal end to end)
        if len({p.shape[0] for p in parts}) == 1:
            whole = np.concatenate(parts, axis=1)
            whole.setflags(write=False)
        _want[f] = (whole, parts)
    return _want[f]


# ---- the granule walk, restated ----
def walk(Ws, bs, granule, eos):
    """include/vorbis_amd.h, "packets with marks", word for word -> (frames, [(first, count, out_at)]): the runs of kept
    frames in the stream's own frames (the first block's centre at 0)"""
    count, pos, keep = 0, -1, []
    for p, W in enumerate(Ws):
        add = bs[Ws[p - 1]] // 4 + bs[W] // 4 if p else 0
        lo, count = count, count + add
        front = back = 0
        g = granule[p] if granule[p] >= -1 else -1
        if pos == -1:
            if g != -1:
                pos = g
                if count > g:
                    cut = min(count - g, add)
                    front, back = (0, cut) if eos[p] else (cut, 0)
        else:
            pos += add
            if g != -1 and pos != g:
                if pos > g and eos[p]:
                    back = min(pos - g, add)
                pos = g
        keep.append((lo + front, count - back))
    runs = []
    for a, b in keep:
        if b > a:
            if runs and runs[-1][1] == a:
                runs[-1][1] = b
            else:
                runs.append([a, b])
    out, at = [], 0
    for a, b in runs:
        out.append((a, b - a, at))
        at += b - a
    return at, out


# ---- the files ----
def _trim(s, k, extra, eos=True, only_page=False):
    """the first audio page holds packets 0 .. k with a granule `extra` short of its samples"""
    steps = s.steps()
    n = len(s.packets)
    gr = list(s.granules)
    gr[k] = sum(steps[:k + 1]) - extra
    groups = [n] if only_page else [k + 1] + [1] * (n - k - 1)
    return b"".join(logical(s, 0x7a00 + k, groups, eos, granules=gr))


def files():
    """name -> (file, the status it must have under the policy); once per process"""
    if _files:
        return _files
    a, b, c, m = stream(STEREO, 0), stream(STEREO, 1), stream(STEREO, 2), stream(MONO, 3)
    F = {}
    F["plain"] = b"".join(logical(a, 0x100)), 0
    F["shift"] = b"".join(logical(a, 0x101, granules=[g + SHIFT for g in a.granules])), 0
    for k in (1, 3):
        step = a.steps()[k]
        for what, extra in (("below", step - 7), ("equal", step), ("above", step + 40), ("none", 0)):
            F["trim_k%d_%s" % (k, what)] = _trim(a, k, extra), 0
    F["trim_packet0"] = _trim(a, 0, 0), 0
    F["trim_only_page_eos"] = _trim(b, len(b.packets) - 1, 300, True, True), 0
    F["no_eos"] = b"".join(logical(a, 0x102, eos=False)), 0
    for what, d in (("low", -90), ("high", 90)):
        # (from the third audio page, which ends with packet 5, to the last but one: the last page's granule then meets a
        # tracked position that is d off)
        gr = [g + d if 5 <= i < len(b.granules) - 2 else g for i, g in enumerate(b.granules)]
        F["mid_" + what] = b"".join(logical(b, 0x103, granules=gr)), 0
    F["two_links"] = b"".join(logical(a, 0x200) + logical(b, 0x201)), 0
    F["three_links"] = b"".join(logical(a, 0x210) + logical(c, 0x211, seq0=7) + logical(b, 0x212)), 0
    F["one_packet_link"] = b"".join(logical(a, 0x220) + logical(b, 0x221, packets=b.packets[:1]) + logical(c, 0x222)), 0
    F["no_eos_then_bos"] = b"".join(logical(a, 0x230, eos=False) + logical(b, 0x231)), 0
    F["other_setup"] = b"".join(logical(a, 0x240) + logical(m, 0x241)), STATUS_BADHEADER
    la, fo = logical(a, 0x250), foreign(0x251, 4)
    F["foreign_bos_first"] = b"".join(fo[:1] + la[:1] + fo[1:2] + la[1:] + fo[2:]), 0
    F["foreign_bos_after"] = b"".join(la[:1] + fo[:1] + la[1:3] + fo[1:] + la[3:]), 0
    mixed = la[:1] + fo[:1]
    for i, pg in enumerate(la[1:]):
        mixed += [pg] + (fo[1 + i:2 + i] if i < 3 else [])
    F["foreign_interleaved"] = b"".join(mixed), 0
    bad = bytearray(fo[2])
    bad[-1] ^= 0x10
    F["foreign_bad_crc"] = b"".join(la[:1] + fo[:1] + la[1:3] + fo[1:2] + [bytes(bad)] + la[3:] + fo[3:]), 0
    _same_as[F["foreign_bad_crc"][0]] = b"".join(la[:1] + fo[:1] + la[1:3] + fo[1:3] + la[3:] + fo[3:])
    F["foreign_past_end"] = b"".join(la[:1] + fo[:1] + la[1:]) + fo[1][:-5], STATUS_BADPAGE
    F["sequence_gap"] = b"".join(logical(a, 0x260) + la[:4] + la[5:]), STATUS_BADPAGE
    last = b.packets[-1]
    assert len(last) > 255
    open_page = page(0, -1, 0x271, 2 + len(b.packets) - 1, [255], last[:255])
    F["link_ends_in_packet"] = b"".join(logical(b, 0x271, groups=[1] * (len(b.packets) - 1), packets=b.packets[:-1], eos=False) + [open_page] + logical(a, 0x272)), STATUS_BADPAGE
    F["foreign_only"] = b"".join(foreign(0x280, 3) + foreign(0x281, 2)), STATUS_BADHEADER
    _files.update(F)
    return _files


def mono_files():
    """the mono stream's files (a context of their own): a plain one, a shifted one, a chain of the two"""
    m = stream(MONO, 3)
    one = logical(m, 0x300)
    two = logical(m, 0x301, granules=[g + SHIFT for g in m.granules])
    return {"mono_plain": (b"".join(one), 0), "mono_shift": (b"".join(two), 0), "mono_chain": (b"".join(one + two), 0)}


# ---- the host program's jobs ----
def build():
    return hostbuild.program("decode_links_host.cpp", ["-O2"])


def _i64s(v):
    v = [] if v is None else [int(x) for x in v]
    return struct.pack("<i", len(v)) + struct.pack("<%dq" % len(v), *v)


def _padded(b):
    return bytes(b) + b"\0" * (-len(b) & 3)


def _run(exe, tmp, mode, blob, job, tag):
    paths = [os.path.join(str(tmp), "%s_%s" % (tag, n)) for n in ("setup", "job", "out")]
    with open(paths[0], "wb") as f:
        f.write(bytes(blob))
    with open(paths[1], "wb") as f:
        f.write(job)
    r = subprocess.run([exe, mode] + paths, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    with open(paths[2], "rb") as f:
        return f.read()


def _results(raw, at, n, ch, floats):
    out = []
    for _ in range(n):
        st, frames, nseg = struct.unpack_from("<iqi", raw, at)
        at += 16
        segs = [struct.unpack_from("<5q", raw, at + 40 * i) for i in range(nseg)]
        at += 40 * nseg
        pcm = None
        if floats and st == 0:
            pcm = np.frombuffer(raw, np.float32, ch * frames, at).reshape(ch, frames)
            at += 4 * ch * frames
        out.append(dict(status=st, frames=frames, segments=segs, pcm=pcm))
    assert at == len(raw), (at, len(raw))
    return out


def run_ogg(exe, tmp, blob, files_, ch, follow=True, setup_header=None, tag="ogg"):
    hdr = bytes(setup_header) if setup_header is not None else b""
    job = struct.pack("<iii", 1 if follow else 0, len(files_), len(hdr)) + _padded(hdr) + b"".join(struct.pack("<q", len(f)) + _padded(f) for f in files_)
    return _results(_run(exe, tmp, "ogg", blob, job, tag), 0, len(files_), ch, follow)


def run_packets(exe, tmp, blob, streams, granules, eos, ch, decode=True, tag="packets"):
    """streams: per stream its audio packets; granules / eos: per stream a list per packet (eos None: NULL) -> None where
    the descriptor was refused, else the results"""
    flat = [p for row in streams for p in row]
    off = np.concatenate([[0], np.cumsum([len(p) for p in flat])]).astype(np.int64)
    start = np.concatenate([[0], np.cumsum([len(row) for row in streams])]).astype(np.int64)
    data = b"".join(flat)
    job = (struct.pack("<iii", len(streams), len(flat), 1 if decode else 0) + _i64s(off) + _i64s(start) + _i64s([g for row in granules for g in row]) +
           _i64s(None if eos is None else [e for row in eos for e in row]) + struct.pack("<i", len(data)) + _padded(data))
    raw = _run(exe, tmp, "packets", blob, job, tag)
    if not struct.unpack_from("<i", raw, 0)[0]:
        return None
    return _results(raw, 4, len(streams), ch, decode)


def run_links(exe, tmp, blob, f, cap, tag="links"):
    """-> (return code, nlinks, [(begin, end, serial)] x min(cap, nlinks))"""
    raw = _run(exe, tmp, "links", blob, struct.pack("<iq", cap, len(f)) + _padded(f), tag)
    rc, n = struct.unpack_from("<iq", raw, 0)
    rows = [struct.unpack_from("<3q", raw, 12 + 24 * i) for i in range(min(cap, n))]
    assert len(raw) == 12 + 24 * len(rows)
    return rc, n, rows
