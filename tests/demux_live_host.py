"""The live Ogg decoder on the host: the shipped walk (vorbis_amd/csrc/vamd_demux_live.h), the live block plan over its
packet table, the bodies of k_ogg_packet_carry_in, k_ogg_depage and k_ogg_packet_carry_out with the lanes in turn, then
unpack, synth, the lap carries and the lap, as a program of its own -- tests/c/demux_live_host.cpp, built with
-fsanitize=address,undefined -- the job file it reads and the result it writes; and the byte cuts both the CPU and the GPU
tests use."""
import os
import subprocess

import numpy as np

from tests import hostbuild

NULL_SLOT, NULL_BYTES, NULL_OFFSET, NULL_CLOSE = 1, 2, 4, 8
V_STATUS, V_PACKETS, V_GRANULE, V_SAMPLES = 1, 2, 4, 8  # a compact run's verdict bits


def build():
    return hostbuild.program("demux_live_host.cpp")


def call(slots, pieces, close=(), **raw):
    """One call of the decoder: pieces[i] the next bytes of slot slots[i]; close: the slots whose stream ends with this
    piece.  raw: a descriptor field as given instead of as derived -- nstreams, slot, piece_offset, close (lists), null
    (NULL_* bits)."""
    off = np.zeros(len(pieces) + 1, np.int64)
    np.cumsum([len(p) for p in pieces], out=off[1:])
    d = dict(nstreams=len(slots), slot=list(slots), piece_offset=off.tolist(), close=[int(s in close) for s in slots],
             bytes=b"".join(bytes(p) for p in pieces), null=0)
    assert set(raw) <= set(d), raw
    d.update(raw)
    return d


def ref(packets, end, pcm):
    """what a stream must come to: tests/ogg_demux_cases.expected()'s triple"""
    return dict(packets=[bytes(p) for p in packets], end=int(end), pcm=np.ascontiguousarray(pcm, np.float32))


def full(calls):
    return dict(compact=0, calls=calls, expect=[])


def compact(calls, expect):
    """expect: [(slot, index into refs)]: the run's pieces on that slot, laid end to end, are held to the ref in the program"""
    return dict(compact=1, calls=calls, expect=list(expect))


def _i64s(v):
    return np.int32(len(v)).tobytes() + np.array(v, np.int64).tobytes()


def _padded(b):
    return bytes(b) + b"\0" * (-len(b) & 3)


def run(exe, tmp, blob, ch, runs, refs=(), max_streams=4, setup_header=None, max_packet_bytes=8192, max_header_bytes=1 << 20):
    """Every run on a fresh decoder.  -> per run: a full run, per call None (the descriptor was refused) or per stream
    dict(status, pcm [ch][frames], end, carry_in, carry_out, packets); a compact run, dict(refused, largest, verdict=[bits
    per expectation])"""
    setup, job, out = (os.path.join(str(tmp), n) for n in ("setup.bin", "oggl.job", "oggl.out"))
    np.ascontiguousarray(blob, np.uint8).tofile(setup)
    hdr = bytes(setup_header) if setup_header is not None else b""
    with open(job, "wb") as f:
        f.write(np.array([max_streams, len(hdr)], np.int32).tobytes() + _padded(hdr))
        f.write(np.array([max_packet_bytes, max_header_bytes], np.int64).tobytes() + np.array([len(refs), len(runs)], np.int32).tobytes())
        for R in refs:
            f.write(np.int32(len(R["packets"])).tobytes() + np.array([len(p) for p in R["packets"]], np.int32).tobytes())
            f.write(_padded(b"".join(R["packets"])) + np.int64(R["end"]).tobytes() + np.int32(R["pcm"].shape[1]).tobytes())
            assert R["pcm"].shape[0] == ch
            f.write(R["pcm"].tobytes())
        for u in runs:
            f.write(np.array([u["compact"], len(u["calls"]), len(u["expect"])], np.int32).tobytes())
            f.write(np.array(u["expect"], np.int32).reshape(-1, 2).tobytes())
            for d in u["calls"]:
                f.write(np.array([d["nstreams"], d["null"]], np.int32).tobytes())
                for k in ("slot", "piece_offset", "close"):
                    f.write(_i64s(d[k]))
                f.write(np.int32(len(d["bytes"])).tobytes() + _padded(d["bytes"]))
    r = subprocess.run([exe, setup, job, out], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    raw = open(out, "rb").read()
    i32 = lambda at: int(np.frombuffer(raw, np.int32, 1, at)[0])  # noqa: E731
    at, res = 0, []
    for u in runs:
        if u["compact"]:
            n = len(u["expect"])
            res.append(dict(refused=i32(at), largest=i32(at + 4), verdict=np.frombuffer(raw, np.int32, n, at + 8).tolist()))
            at += 8 + 4 * n
            continue
        rows_of = []
        for d in u["calls"]:
            ok = i32(at)
            at += 4
            if not ok:
                rows_of.append(None)
                continue
            rows = []
            for _ in range(d["nstreams"]):
                status, frames, end = i32(at), i32(at + 4), int(np.frombuffer(raw, np.int64, 1, at + 8)[0])
                cin, cout, n = i32(at + 16), i32(at + 20), i32(at + 24)
                sizes = np.frombuffer(raw, np.int32, n, at + 28)
                at += 28 + 4 * n
                packets = []
                for v in sizes:
                    packets.append(raw[at:at + int(v)])
                    at += int(v)
                at += -int(sizes.sum()) & 3
                pcm = np.frombuffer(raw, np.float32, ch * frames, at).reshape(ch, frames)
                at += 4 * ch * frames
                rows.append(dict(status=status, pcm=pcm, end=end, carry_in=cin, carry_out=cout, packets=packets))
            rows_of.append(rows)
        res.append(rows_of)
    assert at == len(raw)
    return res


# ---- cuts ----
def pieces_of(f, cuts):
    """the file's bytes cut at the positions `cuts` (non-decreasing, 0 .. len(f); equal neighbours: an empty piece)"""
    edges = [0] + list(cuts) + [len(f)]
    assert all(a <= b for a, b in zip(edges[:-1], edges[1:]))
    return [f[a:b] for a, b in zip(edges[:-1], edges[1:])]


def every(f, step):
    """cuts every `step` bytes"""
    return list(range(step, len(f), step))


def random_cuts(n, rng):
    """a seeded cut list of n bytes: two to eight cuts anywhere, the ends included, two of them equal (an empty piece)"""
    k = int(rng.integers(2, 9))
    cuts = sorted(int(v) for v in rng.integers(0, n + 1, k))
    cuts[int(rng.integers(1, k))] = cuts[0]
    return sorted(cuts)


def one_stream(f, cuts, slot=0, close_with_last=True):
    """the calls that feed one file cut by `cuts` to a slot: the last piece closes it, or an empty piece behind it does"""
    pieces = pieces_of(f, cuts)
    calls = [call([slot], [p], [slot] if close_with_last and i == len(pieces) - 1 else []) for i, p in enumerate(pieces)]
    if not close_with_last:
        calls.append(call([slot], [b""], [slot]))
    return calls


def rounds(files, cut_lists, slots=None):
    """The calls that feed files[i] to slot slots[i] (default i), cut by cut_lists[i], all streams side by side: round r holds
    piece r of every stream that still has one (later rounds name fewer slots); a stream's last piece closes it.
    -> (calls as (slots, pieces, close), per round the stream behind each row)"""
    slots = list(range(len(files))) if slots is None else slots
    cut = [pieces_of(f, c) for f, c in zip(files, cut_lists)]
    calls, who = [], []
    for r in range(max(len(c) for c in cut)):
        live = [i for i in range(len(files)) if r < len(cut[i])]
        last = [i for i in live if r == len(cut[i]) - 1]
        calls.append(([slots[i] for i in live], [cut[i][r] for i in live], [slots[i] for i in last]))
        who.append(live)
    return calls, who


def join(results, who, nstreams, ch):
    """per stream (status or-ed over its pieces, its pieces' samples laid end to end, its packets, the last end granule a
    call applied)"""
    status, parts = [0] * nstreams, [[np.zeros((ch, 0), np.float32)] for _ in range(nstreams)]
    packets, end = [[] for _ in range(nstreams)], [-1] * nstreams
    for rows, live in zip(results, who):
        assert rows is not None and len(rows) == len(live)
        for i, row in zip(live, rows):
            status[i] |= row["status"]
            parts[i].append(row["pcm"])
            packets[i] += row["packets"]
            end[i] = row["end"] if row["end"] >= 0 else end[i]
    return [dict(status=status[i], pcm=np.concatenate(parts[i], axis=1), packets=packets[i], end=end[i]) for i in range(nstreams)]
