"""What the keep policy (vamd_decode_partial: k_unpack_partial, the bounded k_synth) costs, on tools/decode_bench.py's
workload: 64 streams x 20 s stereo, VBR q 0.4 -- the packets a feed makes of them, in host memory, to PCM on the device.

The driver starts every step as a process of its own under a time limit and stops at the first that fails; a step's result
is one JSON line, and the steps hand the packets on in a file in --work.
    encode   tools/decode_bench.py's: the feed's packets of the set, saved
    time     one process, one context: decode_run() on the clean packets with the policy off and on in turn, --reps of
             each after a warm-up of each; then the policy on with one packet in a hundred cut to half its length (the
             same descriptor otherwise).  ms per call; the statuses seen; on clean packets the two policies' PCM compared
    trace    rocprofv3 --kernel-trace --stats over `time`: k_unpack / k_unpack_partial, k_synth / k_synth_bounded and k_lap
             in us per launch, by kernel name and grid

    python tools/decode_partial_bench.py --streams 64 --seconds 20 --reps 5 [--steps encode,time,trace]
"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tools.decode_bench import SETUP, load_rows, step_encode  # noqa: E402

LIMITS = {"encode": 240, "time": 300, "trace": 360}  # seconds a step may take
CUT_EVERY = 100


def cut_rows(rows):
    """one packet in CUT_EVERY cut to half its length, counted over the whole set (never to less than two bytes)"""
    out, k = [], 0
    for packets, granules in rows:
        new = []
        for p in packets:
            k += 1
            new.append(p[:max(len(p) // 2, 2)] if k % CUT_EVERY == 0 and len(p) > 4 else p)
        out.append((new, granules))
    return out


def step_time(a):
    import torch
    import vorbis_amd
    rows = load_rows(a.packets)
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(SETUP), 0)
    clean = an.decode_prepare([p for p, _ in rows], [g[-1] for _, g in rows])
    cut = an.decode_prepare([p for p, _ in cut_rows(rows)], [g[-1] for _, g in rows])
    pcm = {}
    for keep in (False, True):  # warm-up: the tables, the workspace, both sets of kernels
        an.keep_partial = keep
        pcm[keep] = an.decode_run(clean)[0].clone()
    torch.cuda.synchronize()
    same = bool(torch.equal(pcm[False].view(torch.int32), pcm[True].view(torch.int32)))
    ms = {False: [], True: []}
    out = pcm[True]
    for _ in range(a.reps):
        for keep in (False, True):
            an.keep_partial = keep
            t0 = time.perf_counter()
            an.decode_run(clean, out)  # (returns when the statuses are back: the stream is idle)
            ms[keep].append((time.perf_counter() - t0) * 1e3)
    an.keep_partial = True
    status = an.decode_run(cut, out)[3]
    ms_cut = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        an.decode_run(cut, out)
        ms_cut.append((time.perf_counter() - t0) * 1e3)
    an.keep_partial = False
    status_default = an.decode_run(cut, out)[3]
    an.close()
    blocks = sum(len(p) for p, _ in rows)
    r3 = lambda v: [round(x, 3) for x in v]
    return {"step": "time", "blocks": blocks, "cut_packets": blocks // CUT_EVERY, "clean_pcm_same_under_both_policies": same,
            "ms_default": r3(ms[False]), "ms_keep": r3(ms[True]), "ms_keep_one_packet_in_%d_cut" % CUT_EVERY: r3(ms_cut),
            "keep_over_default_min": round(min(ms[True]) / min(ms[False]), 4),
            "statuses_keep_cut": sorted({int(v) for v in status}), "statuses_default_cut": sorted({int(v) for v in status_default})}


def step_trace(a):
    out = os.path.join(a.work, "trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "decode_partial", "--", sys.executable,
           os.path.abspath(__file__), "--only", "time", "--work", a.work, "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS["trace"] - 10)
    if r.returncode:
        raise RuntimeError("rocprofv3 failed: " + r.stderr[-2000:])
    launches = []
    files = glob.glob(os.path.join(out, "**", "*.csv"), recursive=True)
    for path in files:
        if not path.endswith("kernel_trace.csv"):
            continue
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "").split("(")[0]
                if name.startswith(("k_unpack", "k_synth", "k_lap")):
                    launches.append((int(row["Start_Timestamp"]), name, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3,
                                     row.get("Grid_Size_X", row.get("Grid_Size", "?"))))
    launches.sort()
    kernels = {}
    for _, k, us, grid in launches:
        kernels.setdefault("%s grid %s" % (k, grid), []).append(round(us, 1))
    # (in launch order: the two warm-ups, then default and keep in turn, then the calls with cut packets -- all of them the keep kernels')
    res = {"step": "trace", "us_per_launch_in_launch_order": kernels,
           "us_median": {k: float(np.median(v)) for k, v in kernels.items()}}
    if not kernels:
        res["files"] = {os.path.relpath(p, out): open(p).readline().strip() for p in files}
    return res


STEPS = {"encode": step_encode, "time": step_time, "trace": step_trace}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", default="encode,time,trace")
    ap.add_argument("--work", default=None, help="where the steps keep the packets (default: a temporary directory)")
    ap.add_argument("--only", choices=sorted(STEPS), default=None, help="run this one step in this process (the driver's children)")
    a = ap.parse_args()
    if a.only:
        a.packets = os.path.join(a.work, "packets.npz")
        print(json.dumps(STEPS[a.only](a)), flush=True)
        return 0
    work = a.work or tempfile.mkdtemp(prefix="decode_partial_bench_")
    os.makedirs(work, exist_ok=True)
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--only", step, "--work", work, "--streams", str(a.streams),
               "--seconds", str(a.seconds), "--reps", str(a.reps)]
        r = subprocess.run(cmd)
        if r.returncode:  # a step that failed, faulted or ran out of time ends the run: nothing more is started
            print(json.dumps({"step": step, "failed": r.returncode}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
