"""What the decoded signal's output formats (vamd_decode_output: int16 as ov_read converts, fp16, bf16; planar or
interleaved) cost or save on tools/decode_bench.py's set: 64 streams x 20 s stereo, VBR q 0.4 -- the packets a feed makes of
them, in host memory, to PCM on the device.  The format is applied in the store of the last kernel (k_lap_as in k_lap's
place), so a format's call is compared with

    (a) the fp32 planar call in the same process, and
    (b) the fp32 planar call followed by the torch passes a caller writes without the policy:
        (x * 32768).round().clamp(-32768, 32767).to(int16) for int16, .to(dtype) for the float types, and per stream
        .T.contiguous() for interleaved.

The comparison with the parent commit's vamd_decode_streams (c) is tools/decode_bench.py --only time run on both trees over
the same packets file, in processes of their own.

The driver starts every step as a process of its own under a time limit and stops at the first that fails; a step's
result is one JSON line, and the steps hand the packets on in a file in --work.
    encode   tools/decode_bench.py's: the feed's packets of the set, saved
    time     in ONE process, --reps repeats each after a warm-up, interleaved rep by rep: decode_run() end to end in each
             of the eight formats, and (b) for each; every format's PCM against the torch conversion of the fp32 result
    trace    rocprofv3 --kernel-trace over `time`, a run of its own: the lap kernel's us per launch, by instantiation

    python tools/decode_formats_bench.py --streams 64 --seconds 20 --reps 7 [--steps encode,time,trace]
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
DTYPES = ("float32", "int16", "float16", "bfloat16")


def torch_convert(t, x, frames, off, dtype, interleaved, ch):
    """(b): the passes a caller writes over the fp32 planar result -> the converted tensor (flat, the same offsets)"""
    y = x if dtype == t.float32 else (x * 32768).round().clamp(-32768, 32767).to(t.int16) if dtype == t.int16 else x.to(dtype)
    if interleaved:
        if y is x:
            y = x.clone()
        for s in range(len(frames)):
            a, f = int(off[s]), int(frames[s])
            y[a:a + ch * f] = y[a:a + ch * f].view(ch, f).T.contiguous().view(-1)
    return y


def step_time(a):
    import torch as t
    import vorbis_amd
    rows = load_rows(a.packets)
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(SETUP), 0)
    ch = an.channels
    prep = an.decode_prepare([p for p, _ in rows], [g[-1] for _, g in rows])
    formats = [(d, il) for d in DTYPES for il in (False, True)]
    key = lambda d, il: "%s_%s" % (d, "interleaved" if il else "planar")
    pcm, equal = {}, {}
    base, frames, off, status = an.decode_run(prep)  # warm-up: the tables, the workspace
    for d, il in formats:
        an.pcm_dtype, an.pcm_interleaved = getattr(t, d), il
        pcm[d, il] = an.decode_run(prep)[0]
        want = torch_convert(t, base, frames, off, getattr(t, d), il, ch)
        n = int((frames * ch).sum())
        bits = t.int32 if d == "float32" else t.int16
        equal[key(d, il)] = bool(t.equal(pcm[d, il][:n].view(bits), want[:n].view(bits)))
    t.cuda.synchronize()
    ms = {key(d, il): [] for d, il in formats}
    ms.update({"torch_" + key(d, il): [] for d, il in formats[1:]})

    def timed(k, fn):
        t.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        t.cuda.synchronize()
        ms[k].append(round((time.perf_counter() - t0) * 1e3, 3))

    def with_torch(d, il):
        an.decode_run(prep, base)
        torch_convert(t, base, frames, off, getattr(t, d), il, ch)
    for _ in range(a.reps):
        for d, il in formats:
            an.pcm_dtype, an.pcm_interleaved = getattr(t, d), il
            timed(key(d, il), lambda: an.decode_run(prep, pcm[d, il]))
        an.pcm_dtype, an.pcm_interleaved = t.float32, False
        for d, il in formats[1:]:
            timed("torch_" + key(d, il), lambda: with_torch(d, il))
    an.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"step": "time", "blocks": sum(len(p) for p, _ in rows), "frames": int(frames.sum()), "flagged_streams": int((status != 0).sum()),
            "equal_to_the_torch_conversion_of_fp32": equal, "ms_reps": ms, "ms_median": med, "ms_min_max": {k: [min(v), max(v)] for k, v in ms.items()},
            "minus_fp32_planar_ms": {k: round(v - med["float32_planar"], 3) for k, v in med.items() if not k.startswith("torch_")},
            "minus_torch_passes_ms": {k: round(med[k] - med["torch_" + k], 3) for k in med if "torch_" + k in med},
            "note": "each figure includes vamd_decode_plan once more than the decode call itself (decode_run plans, then decodes); "
                    "int16 against torch differs where torch's round() and the clamp see a NaN, which no decoded stream of the set holds"}


def step_trace(a):
    out = os.path.join(a.work, "trace")
    cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", out, "-o", "formats", "--", sys.executable, os.path.abspath(__file__),
           "--only", "time", "--work", a.work, "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS["trace"] - 10)
    if r.returncode:
        raise RuntimeError("rocprofv3 failed: " + r.stderr[-2000:])
    launches, files = {}, glob.glob(os.path.join(out, "**", "*.csv"), recursive=True)
    for path in files:
        if not path.endswith("kernel_trace.csv"):
            continue
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                if "k_lap" in name:
                    launches.setdefault(name.split("(")[0].replace("void ", ""), []).append((int(row["Start_Timestamp"]), (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3))
    us = {k: [round(u, 1) for _, u in sorted(v)] for k, v in launches.items()}
    res = {"step": "trace", "lap_us_median": {k: float(np.median(v)) for k, v in us.items()}, "lap_us_min_max": {k: [min(v), max(v)] for k, v in us.items()},
           "launches": {k: len(v) for k, v in us.items()},
           "note": "PcmOut<D, IL>: D 0 float32, 1 int16, 2 float16, 3 bfloat16; k_lap without arguments is float32 planar, in every format's torch run too"}
    if not us:
        res["files"] = {os.path.relpath(p, out): open(p).readline().strip() for p in files}  # (another rocprofv3's names: say which)
    return res


STEPS = {"encode": step_encode, "time": step_time, "trace": step_trace}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", default="encode,time,trace")
    ap.add_argument("--work", default=None, help="where the steps keep the packets (default: a temporary directory)")
    ap.add_argument("--only", choices=sorted(STEPS), default=None, help="run this one step in this process (the driver's children)")
    a = ap.parse_args()
    if a.only:
        a.packets = os.path.join(a.work, "packets.npz")
        print(json.dumps(STEPS[a.only](a)), flush=True)
        return 0
    work = a.work or tempfile.mkdtemp(prefix="decode_formats_bench_")
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
