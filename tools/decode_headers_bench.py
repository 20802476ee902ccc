"""The header-made decoder (vamd_create_decoder) on tools/decode_ogg_bench.py's set: 64 streams x 20 s stereo, VBR q 0.4, the
files an Ogg feed makes of them.

The driver starts every step as a process of its own under a time limit and stops at the first that fails; a step's result
is one JSON line, and the steps hand the files on in a file in --work.
    encode   tools/decode_ogg_bench.py's: the Ogg feed's files of the set, saved
    time     in ONE process, --reps repeats each after a warm-up, interleaved rep by rep:
               (a) decode_ogg on the blob context, (b) decode_ogg on a context made from the files' own headers -- the same
               kernels: (b)'s PCM against (a)'s, bit for bit;
               (c) decode_streams over the files' packets on the blob context, (d) the same packets on a context made from
               the headers with every lookup-1 residue book written out as lookup type 2 (tests/setup_header_cases.py,
               "explicit"): the same values, from the table -- k_synth_values; (d)'s PCM against (c)'s, bit for bit;
             and the host's share of a context: vamd_create_decoder (parse, image, device) and Analyzer(blob) whole, and
             vamd_create_decoder on a device ordinal that does not exist, which returns behind the parse and the image build
    trace    rocprofv3 --kernel-trace --stats over `time`: k_synth against k_synth_values, k_unpack and k_lap beside them

    python tools/decode_headers_bench.py --streams 64 --seconds 20 --reps 7 [--steps encode,time,trace]
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
from tools.decode_ogg_bench import SETUP, load_files, step_encode  # noqa: E402

LIMITS = {"encode": 240, "time": 240, "trace": 300}  # seconds a step may take


def step_time(a):
    import ctypes as C
    import torch
    import vorbis_amd
    from tests import ogg_demux_cases as cases, setup_header_cases as shc
    files = load_files(a.files)
    headers = vorbis_amd.read_ogg_headers(files[0])
    streams, ends = [], []
    for f in files:
        packets, end, _ = cases.expected(f, decode=False)
        streams.append([bytes(p) for p in packets]), ends.append(int(end))
    blob = vorbis_amd.default_setup_blob(SETUP)
    ms = {"create_blob_context": [], "create_decoder": [], "parse_and_image_alone": []}

    def timed(key, fn):
        t0 = time.perf_counter()
        r = fn()
        ms.setdefault(key, []).append(round((time.perf_counter() - t0) * 1e3, 3))
        return r
    L, h = vorbis_amd.load_library(), C.c_void_p()
    made = []
    for _ in range(a.reps):
        made.append(timed("create_blob_context", lambda: vorbis_amd.Analyzer(blob, 0)))
        made.append(timed("create_decoder", lambda: vorbis_amd.Analyzer.from_headers(headers[0], headers[2], 0)))
        r = timed("parse_and_image_alone", lambda: L.vamd_create_decoder(C.byref(h), headers[0], len(headers[0]), headers[2], len(headers[2]), 9999))
        assert r == vorbis_amd.VAMD_EFAULT, r
    for m in made[2:]:
        m.close()
    an, hd = made[0], made[1]
    ex = vorbis_amd.Analyzer.from_headers(*shc.variant(headers, "explicit")[::2], 0)
    cfg = {"header_context": hd.config_string(), "explicit_context": ex.config_string()}
    prep = {"a_blob_decode_ogg": (an, an.decode_ogg_prepare(files), an.decode_ogg_run), "b_headers_decode_ogg": (hd, hd.decode_ogg_prepare(files), hd.decode_ogg_run),
            "c_blob_decode_streams": (an, an.decode_prepare(streams, ends), an.decode_run), "d_explicit_decode_streams": (ex, ex.decode_prepare(streams, ends), ex.decode_run)}
    out = {k: run(p) for k, (_, p, run) in prep.items()}  # warm-ups: the tables, the workspaces
    torch.cuda.synchronize()

    def same(x, y):  # per stream: its status, its frames, its samples
        (pa, fa, oa, sa), (pb, fb, ob, sb) = out[x], out[y]
        if sa.any() or sb.any() or not np.array_equal(fa, fb):
            return False
        return all(torch.equal(pa[int(oa[s]):int(oa[s]) + 2 * int(fa[s])].view(torch.int32), pb[int(ob[s]):int(ob[s]) + 2 * int(fb[s])].view(torch.int32))
                   for s in range(len(fa)))
    equal = {"b_equals_a_bit_for_bit": same("a_blob_decode_ogg", "b_headers_decode_ogg"), "d_equals_c_bit_for_bit": same("c_blob_decode_streams", "d_explicit_decode_streams")}
    for _ in range(a.reps):
        for k, (_, p, run) in prep.items():
            timed(k, lambda: run(p, out[k][0]))
    for m in (an, hd, ex):
        m.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"step": "time", "files": len(files), "frames": int(out["a_blob_decode_ogg"][1].sum()), **equal, "config": cfg, "ms_reps": ms, "ms_median": med}


def step_trace(a):
    out = os.path.join(a.work, "trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "decode_headers", "--", sys.executable, os.path.abspath(__file__),
           "--only", "time", "--work", a.work, "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS["trace"] - 10)
    if r.returncode:
        raise RuntimeError("rocprofv3 failed: " + r.stderr[-2000:])
    kernels = {}
    for path in glob.glob(os.path.join(out, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "").split("(")[0]
                for k in ("k_synth_values", "k_synth", "k_unpack", "k_lap", "k_ogg_depage"):
                    if k in name:
                        kernels.setdefault("%s grid %s" % (k, row.get("Grid_Size_X", row.get("Grid_Size", "?"))), []).append(
                            round((int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3, 1))
                        break
    return {"step": "trace", "us_median_and_launches": {k: [float(np.median(v)), len(v)] for k, v in sorted(kernels.items())},
            "us_min_max": {k: [min(v), max(v)] for k, v in sorted(kernels.items())}}


STEPS = {"encode": step_encode, "time": step_time, "trace": step_trace}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", default="encode,time,trace")
    ap.add_argument("--work", default=None, help="where the steps keep the files (default: a temporary directory)")
    ap.add_argument("--only", choices=sorted(STEPS), default=None, help="run this one step in this process (the driver's children)")
    a = ap.parse_args()
    if a.only:
        a.files = os.path.join(a.work, "files.npz")
        print(json.dumps(STEPS[a.only](a)), flush=True)
        return 0
    work = a.work or tempfile.mkdtemp(prefix="decode_headers_bench_")
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
