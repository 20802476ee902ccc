"""The live decoder (vamd_decode_live_wrote: k_unpack, k_synth, k_decode_carry_in / _out, k_lap per piece) on
tools/decode_bench.py's workload: 64 streams x 20 s stereo, VBR q 0.4 -- the packets a feed makes of them, cut by their
granule positions into pieces of --pieces seconds (default 1 and 0.1), every stream's piece in one call, a call after
the other -- beside vamd_decode_streams over the whole set in the same process.

The driver starts every step as a process of its own under a time limit and stops at the first that fails; a step's result
is one JSON line, and the steps hand the packets on in a file in --work.
    encode   tools/decode_bench.py's: the feed's packets of the set, saved
    time     per piece length: LiveDecoder.run() call by call over the whole set, --reps passes after a warm-up pass -- the
             median call, and the median over the passes of a pass's total; decode_run() of the whole set, --reps repeats;
             the pieces' samples laid end to end against the whole-stream call's for every stream (bits)
    trace    rocprofv3 --kernel-trace --stats over `time` with one pass: the two carry kernels (and the others) in us per launch

    python tools/decode_live_bench.py --streams 64 --seconds 20 --reps 7 [--steps encode,time,trace]
"""
import argparse
import csv
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
from tools.decode_bench import SETUP, load_rows, step_encode  # noqa: E402

LIMITS = {"encode": 240, "time": 300, "trace": 300}  # seconds a step may take
KERNELS = ("k_decode_carry_in", "k_decode_carry_out", "k_unpack", "k_synth", "k_lap")


def cut(rows, frames_a_piece, npieces):
    """per piece, per stream the packets whose granule position lies in the piece (the last piece takes the rest)"""
    out = [[[] for _ in rows] for _ in range(npieces)]
    for s, (packets, granules) in enumerate(rows):
        for p, g in zip(packets, granules):
            out[min(max(int(g) - 1, 0) // frames_a_piece, npieces - 1)][s].append(p)
    return out


def step_time(a):
    import torch
    import vorbis_amd
    rows = load_rows(a.packets)
    ns = len(rows)
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(SETUP), 0)
    prep = an.decode_prepare([p for p, _ in rows], [g[-1] for _, g in rows])
    pcm, frames, off, status = an.decode_run(prep)  # warm-up: the tables, the workspace
    torch.cuda.synchronize()
    whole = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        an.decode_run(prep, pcm)
        whole.append((time.perf_counter() - t0) * 1e3)
    want = pcm.cpu().numpy()
    res = {"step": "time", "streams": ns, "blocks": sum(len(p) for p, _ in rows), "whole_ms_reps": [round(x, 3) for x in whole],
           "whole_ms_median": round(statistics.median(whole), 3), "pieces": {}}
    dec = an.live_decoder(ns)
    scratch = torch.zeros(pcm.numel() + 4, dtype=torch.float32, device=pcm.device)
    for seconds in a.piece_seconds:
        npieces = max(1, int(round(a.seconds / seconds)))
        pieces = cut(rows, int(44100 * seconds), npieces)
        preps = [dec.prepare(list(range(ns)), pieces[i], close=list(range(ns)) if i == npieces - 1 else (),
                             end_granules={s: rows[s][1][-1] for s in range(ns)} if i == npieces - 1 else None) for i in range(npieces)]
        calls, totals, equal = [], [], 0
        for rep in range(a.reps + 1):  # (pass 0 warms up, and is the one compared)
            parts, t_pass = [[] for _ in range(ns)], 0.0
            for p in preps:
                t0 = time.perf_counter()
                out, f, o, st = dec.run(p, scratch)  # (returns when the statuses are back: the stream is idle)
                dt = (time.perf_counter() - t0) * 1e3
                t_pass += dt
                if rep:
                    calls.append(dt)
                else:
                    assert not st.any()
                    h = out.cpu().numpy()
                    for s in range(ns):
                        parts[s].append(h[int(o[s]):int(o[s]) + 2 * int(f[s])].reshape(2, int(f[s])))
            if rep:
                totals.append(t_pass)
            else:
                for s in range(ns):
                    got = np.concatenate(parts[s], axis=1)
                    w = want[int(off[s]):int(off[s]) + 2 * int(frames[s])].reshape(2, int(frames[s]))
                    equal += int(got.shape == w.shape and np.array_equal(got.view(np.uint32), w.view(np.uint32)))
        res["pieces"]["%g s" % seconds] = {"calls_a_pass": npieces, "call_ms_median": round(statistics.median(calls), 3),
                                          "call_ms_min_max": [round(min(calls), 3), round(max(calls), 3)],
                                          "pass_ms_reps": [round(x, 2) for x in totals], "pass_ms_median": round(statistics.median(totals), 2),
                                          "streams_equal_to_the_whole_stream_call": "%d of %d" % (equal, ns)}
    an.close()
    return res


def step_trace(a):
    out = os.path.join(a.work, "trace_live")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "decode_live", "--", sys.executable, os.path.abspath(__file__),
           "--only", "time", "--work", a.work, "--reps", "1", "--seconds", str(a.seconds), "--pieces", ",".join("%g" % s for s in a.piece_seconds)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS["trace"] - 10)
    if r.returncode:
        raise RuntimeError("rocprofv3 failed: " + r.stderr[-2000:])
    us = {k: [] for k in KERNELS}
    files = glob.glob(os.path.join(out, "**", "*.csv"), recursive=True)
    for path in files:
        if not path.endswith("kernel_trace.csv"):
            continue
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                for k in KERNELS:
                    if name.startswith(k + "(") or name == k or name.startswith(k + " "):
                        us[k].append((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3)
    res = {"step": "trace", "us_per_launch": {k: {"launches": len(v), "median": round(statistics.median(v), 2), "min": round(min(v), 2), "max": round(max(v), 2)}
                                              for k, v in us.items() if v}}
    if not res["us_per_launch"]:
        res["files"] = {os.path.relpath(p, out): open(p).readline().strip() for p in files}  # (another rocprofv3's names: say which)
    return res


STEPS = {"encode": step_encode, "time": step_time, "trace": step_trace}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--pieces", default="1,0.1", help="the piece lengths in seconds")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", default="encode,time,trace")
    ap.add_argument("--work", default=None, help="where the steps keep the packets (default: a temporary directory)")
    ap.add_argument("--only", choices=sorted(STEPS), default=None, help="run this one step in this process (the driver's children)")
    a = ap.parse_args()
    a.piece_seconds = [float(v) for v in a.pieces.split(",")]
    if a.only:
        a.packets = os.path.join(a.work, "packets.npz")
        print(json.dumps(STEPS[a.only](a)), flush=True)
        return 0
    work = a.work or tempfile.mkdtemp(prefix="decode_live_bench_")
    os.makedirs(work, exist_ok=True)
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--only", step, "--work", work, "--streams", str(a.streams),
               "--seconds", str(a.seconds), "--reps", str(a.reps), "--pieces", a.pieces]
        r = subprocess.run(cmd)
        if r.returncode:  # a step that failed, faulted or ran out of time ends the run: nothing more is started
            print(json.dumps({"step": step, "failed": r.returncode}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
