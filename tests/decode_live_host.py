"""The live decoder on the host: the shipped planning (vorbis_amd/csrc/vamd_decode_live_plan.h), unpack_packet, synth_block,
the two carry bodies and lap_sample for one lane as a program of its own -- tests/c/decode_live_host.cpp, built with
-fsanitize=address,undefined -- the job files it reads and the results it writes; and the cut lists both the CPU and the
GPU tests use."""
import os
import subprocess

import numpy as np

from tests import hostbuild

NULL_SLOT, NULL_BYTES, NULL_OFFSET, NULL_START, NULL_CLOSE, NULL_GRANULE = 1, 2, 4, 8, 16, 32


def build():
    return hostbuild.program("decode_live_host.cpp")


def call(slots, pieces, close=(), granules=None, **raw):
    """One call of the decoder: pieces[i] the packets of slot slots[i]; close: the slots whose stream ends with this piece;
    granules: {slot: end granule}.  raw: a descriptor field as given instead of as derived -- nstreams, npackets, slot,
    offset, stream_start, close, end_granule (lists), null (NULL_* bits)."""
    flat = [p for row in pieces for p in row]
    off = np.zeros(len(flat) + 1, np.int64)
    np.cumsum([len(p) for p in flat], out=off[1:])
    start = np.zeros(len(pieces) + 1, np.int64)
    np.cumsum([len(row) for row in pieces], out=start[1:])
    granules = granules or {}
    d = dict(nstreams=len(slots), npackets=len(flat), slot=list(slots), offset=off.tolist(), stream_start=start.tolist(),
             close=[int(s in close) for s in slots], end_granule=[granules.get(s, -1) for s in slots], bytes=b"".join(flat), null=0)
    assert set(raw) <= set(d), raw
    d.update(raw)
    return d


def _i64s(v):
    return np.int32(len(v)).tobytes() + np.array(v, np.int64).tobytes()


def run(exe, tmp, blob, max_streams, calls, ch):
    """-> per call None (the descriptor was refused) or [(status, pcm [ch][frames])] per stream of the call"""
    setup, job, out = (os.path.join(str(tmp), n) for n in ("setup.bin", "live.job", "live.out"))
    np.ascontiguousarray(blob, np.uint8).tofile(setup)
    with open(job, "wb") as f:
        f.write(np.array([max_streams, len(calls)], np.int32).tobytes())
        for d in calls:
            f.write(np.array([d["nstreams"], d["npackets"], d["null"]], np.int32).tobytes())
            for k in ("slot", "offset", "stream_start", "close", "end_granule"):
                f.write(_i64s(d[k]))
            b = d["bytes"]
            f.write(np.int32(len(b)).tobytes() + b + b"\0" * (-len(b) & 3))
    r = subprocess.run([exe, setup, job, out], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    raw, at, res = np.fromfile(out, np.int32), 0, []
    for d in calls:
        ok = int(raw[at])
        at += 1
        if not ok:
            res.append(None)
            continue
        rows = []
        for _ in range(d["nstreams"]):
            status, frames = int(raw[at]), int(raw[at + 1])
            rows.append((status, raw[at + 2:at + 2 + ch * frames].view(np.float32).reshape(ch, frames)))
            at += 2 + ch * frames
        res.append(rows)
    assert at == raw.size
    return res


# ---- cuts ----
def pieces_of(packets, cuts):
    """the packet list cut at the positions `cuts` (non-decreasing, 0 .. len(packets); equal neighbours: an empty piece)"""
    edges = [0] + list(cuts) + [len(packets)]
    assert all(a <= b for a, b in zip(edges[:-1], edges[1:]))
    return [packets[a:b] for a, b in zip(edges[:-1], edges[1:])]


def closes_empty(packets, cuts):
    """the last piece of this cut list is empty: it only frees the slot, and the end granule is not applied"""
    return bool(cuts) and cuts[-1] == len(packets)


def random_cuts(n, rng):
    """a seeded cut list of n packets: two to eight cuts anywhere, the ends included, two of them equal (an empty piece)"""
    k = int(rng.integers(2, 9))
    cuts = sorted(int(v) for v in rng.integers(0, n + 1, k))
    cuts[int(rng.integers(1, k))] = cuts[0]
    return sorted(cuts)


def rounds(streams, cut_lists, ends, slots=None):
    """The calls that decode streams[i] on slot slots[i] (default i), cut by cut_lists[i], all streams side by side: round r
    holds piece r of every stream that still has one (later rounds name fewer slots); a stream's last piece closes it with
    its end granule.  -> (calls as (slots, pieces, close, granules), per round the stream behind each row)"""
    slots = list(range(len(streams))) if slots is None else slots
    cut = [pieces_of(p, c) for p, c in zip(streams, cut_lists)]
    calls, who = [], []
    for r in range(max(len(c) for c in cut)):
        live = [i for i in range(len(streams)) if r < len(cut[i])]
        last = [i for i in live if r == len(cut[i]) - 1]
        calls.append(([slots[i] for i in live], [cut[i][r] for i in live], [slots[i] for i in last], {slots[i]: ends[i] for i in last}))
        who.append(live)
    return calls, who


def join(results, who, nstreams, ch):
    """per stream (status or-ed over its pieces, its pieces' samples laid end to end)"""
    status, parts = [0] * nstreams, [[np.zeros((ch, 0), np.float32)] for _ in range(nstreams)]
    for rows, live in zip(results, who):
        assert rows is not None and len(rows) == len(live)
        for i, (st, pcm) in zip(live, rows):
            status[i] |= st
            parts[i].append(pcm)
    return [(status[i], np.concatenate(parts[i], axis=1)) for i in range(nstreams)]
