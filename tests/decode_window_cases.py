"""Windows for the window decoder's tests (tests/test_decode_window_cpu.py on the one-lane host build,
tests/test_decode_window_gpu.py on the GPU): the window list a stream is put through, what the plan must take for each
window -- computed here from the packets' mode bits and tests/ogg_framing.py's pages, never from the code under test --
and the job files of tests/c/decode_window_host.cpp.

The oracle of a window is always the reference decode of the WHOLE stream, sliced."""
import os
import struct
import subprocess

import numpy as np

from tests import hostbuild, ogg_framing, ref_host
from tests import ogg_demux_cases as cases

NULL_STREAM, NULL_START, NULL_COUNT, NULL_BYTES, NULL_FILE_OFFSET = 1, 2, 4, 8, 16


def classes(packets, bs):
    """the size class of each audio packet, from its mode bit"""
    return [(p[0] >> 1) & 1 if bs[0] != bs[1] else 0 for p in packets]


def centres(packets, bs):
    """the block centres C_0 = 0 < C_1 < ... (lib/block.c:840-842: bs[lW] / 4 + bs[W] / 4 apart)"""
    Ws, out = classes(packets, bs), []
    for i in range(len(packets)):
        out.append(out[-1] + bs[Ws[i - 1]] // 4 + bs[Ws[i]] // 4 if i else 0)
    return out


def edge_windows(packets, bs, T):
    """The window list of one stream -> [(start, count)]: start in {0, C_k - 1, C_k, C_k + 1} for one k at each of the
    size-class transitions the stream has, x count in {0, 1, one step, T}; start = T - 1, T, T + 5; start + count beyond T;
    (0, T); two overlapping windows.  A stream without frames: windows that must all come out empty."""
    if T == 0:
        return [(0, 0), (0, 5), (5, 5)]
    C, Ws = centres(packets, bs), classes(packets, bs)
    out = []
    for lW, W in ((0, 0), (0, 1), (1, 0), (1, 1)):
        ks = [k for k in range(1, len(C)) if (Ws[k - 1], Ws[k]) == (lW, W)]
        if not ks:
            continue
        k = ks[len(ks) // 2]
        for start in (0, C[k] - 1, C[k], C[k] + 1):
            for count in (0, 1, C[k] - C[k - 1], T):
                out.append((start, count))
    out += [(T - 1, 1), (T - 1, 9), (T, 1), (T + 5, 3), (max(T - 10, 0), 50), (0, T)]
    out += [(T // 3, T // 3), (T // 3 + T // 6, T // 3)]  # two that overlap
    return list(dict.fromkeys(out))


def transitions(packets, bs):
    Ws = classes(packets, bs)
    return set(zip(Ws[:-1], Ws[1:]))


def cut(start, count, T):
    return min(start, T), min(start + count, T)


def blocks_of(packets, bs, T, start, count):
    """-> (kA - 1, kB) of a non-empty window, None of an empty one: kA / kB the first k with C_k > a / C_k > b - 1"""
    a, b = cut(start, count, T)
    if b <= a:
        return None
    C = centres(packets, bs)
    kA = next(k for k in range(len(C)) if C[k] > a)
    kB = next(k for k in range(len(C)) if C[k] > b - 1)
    return kA - 1, kB


def nblocks_of(streams, bs, Ts, windows):
    """streams: per stream its audio packets; windows: [(stream, start, count)] -> [short, long] blocks, summed: blocks
    kA - 1 .. kB, kB - kA + 2 of them, per non-empty window"""
    n = [0, 0]
    for s, start, count in windows:
        span = blocks_of(streams[s], bs, Ts[s], start, count)
        if span:
            for W in classes(streams[s], bs)[span[0]:span[1] + 1]:
                n[W] += 1
    return n


def packet_pages(pages, nheaders=3):
    """per audio packet (first, last): the pages that hold its first and its last byte (tests/ogg_framing.py's pages)"""
    out, k, first, last = [], 0, None, None
    for i, p in enumerate(pages):
        for v in p["lacing"]:
            if v:
                first, last = (i if first is None else first), i
            if v < 255:
                if k >= nheaders:
                    out.append((first, last))
                k, first, last = k + 1, None, None
    return out


def staged_bytes(files, streams, bs, Ts, windows):
    """the bytes a window call stages: per non-empty window its pages' lengths, from the page in which its first packet
    begins through the one that holds its last packet's last byte -> (bytes, pages)"""
    total = rows = 0
    for s, start, count in windows:
        span = blocks_of(streams[s], bs, Ts[s], start, count)
        if span:
            pages = ogg_framing.demux(files[s])[0]
            where = packet_pages(pages)
            p0, p1 = where[span[0]][0], where[span[1]][1]
            total += sum(p["bytes"] for p in pages[p0:p1 + 1])
            rows += p1 - p0 + 1
    return total, rows


def damage_case(name):
    """ogg_demux_cases.damaged's body_bit file (a segment a page) -> (blob, setup header, [the file, a clean one], packets, T,
    want, the window over the damaged page, a window beside it)"""
    d = cases.damaged(name)
    s = d.kind.index("body_bit")
    f, base = d.files[s], cases.base_files(name, "singles")[2][0]
    assert len(f) == len(base)
    (at,) = [i for i in range(len(f)) if f[i] != base[i]]
    pages = ogg_framing.demux(base)[0]
    j = next(i for i, p in enumerate(pages) if p["offset"] <= at < p["offset"] + p["bytes"])
    packets, _, want = cases.expected(base)
    where = packet_pages(pages)
    enc = ref_host.encoder(name)
    bs = (enc.blocksize(0), enc.blocksize(1))
    C = centres(packets, bs)
    k = next(k for k, (a, b) in enumerate(where) if a <= j <= b)
    assert not (where[k][0] == j and at == pages[j]["offset"] + 27 + pages[j]["nseg"])  # (not a packet's mode byte: the plan stands)
    m = k + 3 if k + 4 < len(C) else k - 4
    assert 1 <= k < len(C) - 1 and m >= 0
    over, beside = (0, C[k] - 2, 4), (0, C[m] + 1, 2)
    assert blocks_of(packets, bs, want.shape[1], *over[1:]) == (k - 1, k + 1) and blocks_of(packets, bs, want.shape[1], *beside[1:]) == (m, m + 1)
    return d.blob, d.setup_header, [f, d.files[s - 1]], want, cases.expected(d.files[s - 1])[2], over, beside


# ---- the host program's jobs ----
def build():
    return hostbuild.program("decode_window_host.cpp", ["-O2"])


def _i64s(v):
    v = [] if v is None else [int(x) for x in v]
    return struct.pack("<i", len(v)) + struct.pack("<%dq" % len(v), *v)


def _padded(b):
    return bytes(b) + b"\0" * (-len(b) & 3)


def _files(files):
    return b"".join(struct.pack("<q", len(f)) + _padded(f) for f in files)


def call(windows, null=0, file_offset=None, files=None, columns=None):
    """windows: [(stream, start, count)]; null: NULL_* bits; file_offset / files: what the call hands again where that is
    not the index's own; columns: the three lists as given (their lengths may differ from nwindows)"""
    cols = columns if columns is not None else ([w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows])
    nw = len(windows) if not isinstance(windows, int) else windows
    return (struct.pack("<ii", null, nw) + b"".join(_i64s(c) for c in cols) + _i64s(file_offset) +
            struct.pack("<i", len(files) if files else 0) + (_files(files) if files else b""))


def _read_calls(raw, at, calls, nwindows, ch):
    out = []
    for nw in nwindows:
        (ok,) = struct.unpack_from("<i", raw, at)
        at += 4
        if not ok:
            out.append(None)
            continue
        n0, n1, staged, rows = struct.unpack_from("<4q", raw, at)
        at += 32
        wins = []
        for _ in range(nw):
            st, frames = struct.unpack_from("<ii", raw, at)
            at += 8
            wins.append((st, np.frombuffer(raw, np.float32, ch * frames, at).reshape(ch, frames)))
            at += 4 * ch * frames
        out.append(dict(nblocks=[n0, n1], staged=staged, rows=rows, windows=wins))
    assert at == len(raw), (at, len(raw))
    return out


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


def run_ogg(exe, tmp, blob, files, setup_header, calls, nwindows, ch, tag="ogg"):
    """calls: call()'s bytes; nwindows: per call how many windows a result holds -> ([(status, T)] of the index, per call None
    (refused) or dict(nblocks, staged, rows, windows=[(status, pcm)]))"""
    hdr = bytes(setup_header) if setup_header is not None else b""
    job = struct.pack("<ii", len(files), len(hdr)) + _padded(hdr) + _files(files) + struct.pack("<i", len(calls)) + b"".join(calls)
    raw = _run(exe, tmp, "ogg", blob, job, tag)
    info = [struct.unpack_from("<iq", raw, 12 * s) for s in range(len(files))]
    return info, _read_calls(raw, 12 * len(files), calls, nwindows, ch)


def run_packets(exe, tmp, blob, streams, ends, calls, nwindows, ch, tag="packets"):
    flat = [p for row in streams for p in row]
    off = np.concatenate([[0], np.cumsum([len(p) for p in flat])]).astype(np.int64)
    start = np.concatenate([[0], np.cumsum([len(row) for row in streams])]).astype(np.int64)
    data = b"".join(flat)
    job = (struct.pack("<ii", len(streams), len(flat)) + _i64s(off) + _i64s(start) + _i64s(ends) + struct.pack("<i", len(data)) + _padded(data) +
           struct.pack("<i", len(calls)) + b"".join(calls))
    return _read_calls(_run(exe, tmp, "packets", blob, job, tag), 0, calls, nwindows, ch)
