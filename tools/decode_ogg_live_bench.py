"""The live Ogg decoder (vamd_decode_ogg_live_wrote: the host's walk with its state per slot, k_ogg_packet_carry_in,
k_ogg_depage, k_ogg_packet_carry_out, then k_unpack, k_synth, the lap carries and k_lap per piece) on
tools/decode_ogg_bench.py's set: 64 files x 20 s stereo, VBR q 0.4 -- the files an Ogg feed makes of them, cut into BYTE
pieces worth --pieces seconds (default 1 and 0.1: a file of 20 s in 20 and in 200 equal runs of bytes, so the cuts fall
inside pages and packets), every stream's piece in one call, a call after the other -- beside, in the same process,
vamd_decode_live_wrote over the same streams' packets cut at the same packets (the packets each byte piece completes,
demuxed beforehand and not timed) and vamd_decode_ogg over the whole set.

The driver starts every step as a process of its own under a time limit and stops at the first that fails; a step's result
is one JSON line, and the steps hand the files on in a file in --work.
    encode   tools/decode_ogg_bench.py's: the Ogg feed's files of the set, saved
    time     after a warm-up pass of each, --reps passes, the three turn and turn about: LiveOggDecoder.run() call by call,
             LiveDecoder.run() call by call, decode_ogg_run() of the whole set -- the median call and its spread, the median
             pass and its spread; per call also vamd_decode_ogg_live_plan alone (the host walk and the block plan, nothing
             enqueued); the live Ogg pieces' samples laid end to end against decode_ogg's for every stream (bits)
    trace    rocprofv3 --kernel-trace --stats over `time` with one pass: k_ogg_depage and the others in us per launch.  An
             Ogg feed ends its pages at packet ends, so on its files no packet is left open by a whole page and the two
             byte-carry kernels have nothing to launch for; a second trace runs `time` over the first --repaged files laid
             out anew with three segments a page (tests/ogg_demux_cases.write), where most packets lie across pages

    python tools/decode_ogg_live_bench.py --streams 64 --seconds 20 --reps 7 [--steps encode,time,trace]
"""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.decode_ogg_bench import SETUP, load_files, step_encode  # noqa: E402

LIMITS = {"encode": 240, "time": 400, "trace": 400}  # seconds a step may take
KERNELS = ("k_ogg_packet_carry_in", "k_ogg_packet_carry_out", "k_ogg_depage", "k_decode_carry_in", "k_decode_carry_out", "k_unpack", "k_synth", "k_lap")


def walk(f):
    """a clean file's audio packets with, for each, the offset behind the page that completes it, and the end granule (the
    page headers and lacing tables alone: no checksum)"""
    pos, cur, done, packets, ends, granule = 0, [], 0, [], [], -1
    while pos < len(f):
        n = f[pos + 26]
        lacing = f[pos + 27:pos + 27 + n]
        at = pos + 27 + n
        end = at + sum(lacing)
        for v in lacing:
            cur.append(f[at:at + v])
            at += v
            if v < 255:
                if done >= 3:
                    packets.append(b"".join(cur)), ends.append(end)
                    granule = int.from_bytes(f[pos + 6:pos + 14], "little", signed=True)
                cur, done = [], done + 1
        pos = end
    return packets, ends, granule


def repaged(f, segments=3):
    """the file's packets in pages of `segments` segments: a packet of 255 bytes and more lies across pages"""
    from tests import ogg_demux_cases, ogg_framing
    pages, packets = ogg_framing.demux(f)
    gr = ogg_framing.page_granules(pages, len(packets) - 3)
    return ogg_demux_cases.write(packets, [0, 0, 0] + list(gr), lambda *a: segments, pages[0]["serial"])


def cuts_of(f, npieces):
    return [len(f) * k // npieces for k in range(1, npieces)]


def stat(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def step_time(a):
    import torch
    import vorbis_amd
    files = load_files(a.files)
    if a.repaged:
        files = [repaged(f) for f in files[:a.repaged]]
    ns = len(files)
    walked = [walk(f) for f in files]
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(SETUP), 0)
    prep_whole = an.decode_ogg_prepare(files)
    pcm, frames, off, status = an.decode_ogg_run(prep_whole)  # warm-up: the tables, the workspace
    torch.cuda.synchronize()
    assert not status.any()
    want = pcm.cpu().numpy()
    scratch = torch.zeros(pcm.numel() + 4, dtype=torch.float32, device=pcm.device)
    ogg, live = an.live_ogg_decoder(ns), an.live_decoder(ns)
    res = {"step": "time", "streams": ns, "repaged": bool(a.repaged), "file_bytes": sum(len(f) for f in files), "packets": sum(len(w[0]) for w in walked), "pieces": {}}
    whole_ms = []
    for seconds in a.piece_seconds:
        npieces = max(1, int(round(a.seconds / seconds)))
        cuts = [cuts_of(f, npieces) + [len(f)] for f in files]
        slots, last = list(range(ns)), npieces - 1
        preps_ogg, preps_live = [], []
        for i in range(npieces):
            lo = [c[i - 1] if i else 0 for c in cuts]
            preps_ogg.append(ogg.prepare(slots, [f[b:c[i]] for f, b, c in zip(files, lo, cuts)], close=slots if i == last else ()))
            rows = [[p for p, e in zip(w[0], w[1]) if b < e <= c[i]] for w, b, c in zip(walked, lo, cuts)]  # the packets the byte piece completes
            preps_live.append(live.prepare(slots, rows, close=slots if i == last else (), end_granules={s: walked[s][2] for s in slots} if i == last else None))
        t = {"ogg_call": [], "live_call": [], "ogg_plan": [], "ogg_pass": [], "live_pass": []}
        equal = 0
        fr, nb = np.zeros(ns, np.int64), np.zeros(2, np.int64)
        for rep in range(a.reps + 1):  # (pass 0 warms up, and is the one compared)
            parts, t_ogg, t_live = [[] for _ in range(ns)], 0.0, 0.0
            for p in preps_ogg:
                t0 = time.perf_counter()
                an.L.vamd_decode_ogg_live_plan(ogg.h, C.byref(p["desc"]), C.c_void_p(fr.ctypes.data), C.c_void_p(nb.ctypes.data))
                t1 = time.perf_counter()
                out, f_, o, st = ogg.run(p, scratch)  # (returns when the statuses are back: the stream is idle)
                t2 = time.perf_counter()
                t_ogg += (t2 - t1) * 1e3
                if rep:
                    t["ogg_plan"].append((t1 - t0) * 1e3), t["ogg_call"].append((t2 - t1) * 1e3)
                else:
                    assert not st.any()
                    h = out.cpu().numpy()
                    for s in range(ns):
                        parts[s].append(h[int(o[s]):int(o[s]) + 2 * int(f_[s])].reshape(2, int(f_[s])))
            for p in preps_live:
                t0 = time.perf_counter()
                live.run(p, scratch)
                dt = (time.perf_counter() - t0) * 1e3
                t_live += dt
                if rep:
                    t["live_call"].append(dt)
            t0 = time.perf_counter()
            an.decode_ogg_run(prep_whole, pcm)
            if rep:
                whole_ms.append((time.perf_counter() - t0) * 1e3), t["ogg_pass"].append(t_ogg), t["live_pass"].append(t_live)
            else:
                for s in range(ns):
                    got = np.concatenate(parts[s], axis=1)
                    w = want[int(off[s]):int(off[s]) + 2 * int(frames[s])].reshape(2, int(frames[s]))
                    equal += int(got.shape == w.shape and np.array_equal(got.view(np.uint32), w.view(np.uint32)))
        res["pieces"]["%g s" % seconds] = {"calls_a_pass": npieces, "ogg_live_call_ms": stat(t["ogg_call"]), "packet_live_call_ms": stat(t["live_call"]),
                                          "ogg_live_plan_alone_ms": stat(t["ogg_plan"]), "ogg_live_pass_ms": stat(t["ogg_pass"]),
                                          "packet_live_pass_ms": stat(t["live_pass"]),
                                          "call_over_packet_live_call_ms": round(statistics.median(t["ogg_call"]) - statistics.median(t["live_call"]), 3),
                                          "streams_equal_to_decode_ogg": "%d of %d" % (equal, ns)}
    res["decode_ogg_whole_ms"] = stat(whole_ms)
    res["note"] = "a run() plans, then decodes: the live Ogg call's time holds the host walk twice, the packet call's its plan twice"
    an.close()
    return res


def trace_of(a, out, more, limit):
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "decode_ogg_live", "--", sys.executable, os.path.abspath(__file__),
           "--only", "time", "--work", a.work, "--reps", "1", "--seconds", str(a.seconds), "--pieces", ",".join("%g" % s for s in a.piece_seconds)] + more
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=limit)
    if r.returncode:
        raise RuntimeError("rocprofv3 failed: " + r.stderr[-2000:])
    us = {k: [] for k in KERNELS}
    files = glob.glob(os.path.join(out, "**", "*.csv"), recursive=True)
    for path in files:
        if not path.endswith("kernel_trace.csv"):
            continue
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "").split("(")[0].split("::")[-1].strip()
                if name in us:
                    us[name].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    res = {k: {"launches": len(v), "median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)} for k, v in us.items() if v}
    if not res:
        res["files"] = {os.path.relpath(p, out): open(p).readline().strip() for p in files}  # (another rocprofv3's names: say which)
    return res


def step_trace(a):
    half = (LIMITS["trace"] - 20) // 2
    return {"step": "trace", "us_per_launch": trace_of(a, os.path.join(a.work, "trace_ogg_live"), [], half),
            "us_per_launch_repaged_%d_files" % a.repaged_files: trace_of(a, os.path.join(a.work, "trace_ogg_live_repaged"),
                                                                        ["--repaged", str(a.repaged_files)], half)}


STEPS = {"encode": step_encode, "time": step_time, "trace": step_trace}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--pieces", default="1,0.1", help="the piece lengths in seconds")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", default="encode,time,trace")
    ap.add_argument("--work", default=None, help="where the steps keep the files (default: a temporary directory)")
    ap.add_argument("--repaged", type=int, default=0, help="`time` over this many of the files, laid out anew with three segments a page")
    ap.add_argument("--repaged-files", type=int, default=8, help="how many files the second trace lays out anew")
    ap.add_argument("--only", choices=sorted(STEPS), default=None, help="run this one step in this process (the driver's children)")
    a = ap.parse_args()
    a.piece_seconds = [float(v) for v in a.pieces.split(",")]
    if a.only:
        a.files = os.path.join(a.work, "files.npz")
        print(json.dumps(STEPS[a.only](a)), flush=True)
        return 0
    work = a.work or tempfile.mkdtemp(prefix="decode_ogg_live_bench_")
    os.makedirs(work, exist_ok=True)
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--only", step, "--work", work, "--streams", str(a.streams),
               "--seconds", str(a.seconds), "--reps", str(a.reps), "--pieces", a.pieces, "--repaged-files", str(a.repaged_files)]
        r = subprocess.run(cmd)
        if r.returncode:  # a step that failed, faulted or ran out of time ends the run: nothing more is started
            print(json.dumps({"step": step, "failed": r.returncode}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
