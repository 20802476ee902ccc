"""The Ogg decode entry (vamd_decode_ogg: the host's page walk, k_ogg_depage, then k_unpack, k_synth, k_lap) on
tools/decode_bench.py's set: 64 streams x 20 s stereo, VBR q 0.4 (the committed 44k_stereo_q4 blob), the FILES an Ogg feed
makes of them, in host memory, to PCM on the device -- beside the path a caller had before: a host demux of the files
(tools/ogg_demux_ref.c, compiled -O2: page walk, table CRC, packet gather) in front of vamd_decode_streams.

The driver starts every step as a process of its own under a time limit and stops at the first that fails; a step's result
is one JSON line, and the steps hand the files on in a file in --work.
    encode   the Ogg feed's files of the set, saved
    time     in ONE process, --reps repeats each after a warm-up, the three interleaved rep by rep: (a) decode_run over the
             files' packets, (b) decode_ogg_run over the files, (c) the C host demux of the files; and the host scan alone
             (vamd_decode_ogg_plan: the walk and the block plan, nothing enqueued).  (b)'s PCM against (a)'s, bit for bit.
    trace    rocprofv3 --kernel-trace --stats over `time`: k_ogg_depage, k_unpack, k_synth, k_lap in us per launch

    python tools/decode_ogg_bench.py --streams 64 --seconds 20 --reps 7 [--steps encode,time,trace]
"""
import argparse
import csv
import ctypes as C
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
SETUP = "44k_stereo_q4"
LIMITS = {"encode": 240, "time": 240, "trace": 300}  # seconds a step may take


def step_encode(a):
    import torch
    import vorbis_amd
    from tests import ref_host
    from tools.feed_device_bench import stream_set
    frames = int(44100 * a.seconds)
    pcm = stream_set(a.streams, frames)
    src = (torch.from_numpy(np.ascontiguousarray(pcm.transpose(0, 2, 1))).cuda().float() / 32768.0).contiguous()
    headers = ref_host.reference_headers(2, 44100, 0.4)
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob(SETUP), lanes_per_device=1, max_streams=a.streams, max_frames=frames,
                           fmt=vorbis_amd.FEED_S16 | vorbis_amd.FEED_NO_ARENA, ogg_headers=headers)
    try:
        files = feed.encode_ogg_tensors(src)
    finally:
        feed.close()
    np.savez(a.files, bytes=np.frombuffer(b"".join(files), np.uint8), lengths=np.array([len(f) for f in files], np.int64))
    return {"step": "encode", "streams": a.streams, "seconds": a.seconds, "file_bytes": sum(len(f) for f in files)}


def load_files(path):
    z = np.load(path)
    data, ends = z["bytes"].tobytes(), np.concatenate([[0], np.cumsum(z["lengths"])])
    return [data[int(ends[k]):int(ends[k + 1])] for k in range(len(z["lengths"]))]


class HostDemux:
    """tools/ogg_demux_ref.c as a shared library, built -O2 into --work"""

    def __init__(self, work):
        lib = os.path.join(work, "libogg_demux_ref.so")
        subprocess.check_call(["gcc", "-O2", "-shared", "-fPIC", os.path.join(ROOT, "tools", "ogg_demux_ref.c"), "-o", lib])
        self.L = C.CDLL(lib)
        self.L.ogg_demux_ref.restype = C.c_long
        self.L.ogg_demux_ref.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p]

    def run(self, files, out, sizes):
        """every file in turn -> per stream (number of packets, end granule); the packets back to back in `out`"""
        res, at, k = [], 0, 0
        for f in files:
            end = C.c_longlong()
            n = self.L.ogg_demux_ref(f, len(f), out.ctypes.data + at, out.size - at, sizes.ctypes.data + 8 * k, sizes.size - k, C.byref(end))
            assert n >= 0
            at, k = at + int(sizes[k:k + n].sum()), k + n
            res.append((n, end.value))
        return res


def step_time(a):
    import torch
    import vorbis_amd
    files = load_files(a.files)
    total = sum(len(f) for f in files)
    demux = HostDemux(a.work)
    out, sizes = np.zeros(total, np.uint8), np.zeros(total // 16 + 64, np.int64)
    table = demux.run(files, out, sizes)
    streams, ends, at, byte = [], [], 0, 0
    for n, end in table:
        row = []
        for v in sizes[at:at + n]:
            row.append(out[byte:byte + int(v)].tobytes())
            byte += int(v)
        streams.append(row), ends.append(end)
        at += n
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(SETUP), 0)
    prep_a, prep_b = an.decode_prepare(streams, ends), an.decode_ogg_prepare(files)
    pcm_a, frames, off, status_a = an.decode_run(prep_a)  # warm-ups: the tables, the workspaces
    pcm_b, frames_b, off_b, status_b = an.decode_ogg_run(prep_b)
    torch.cuda.synchronize()
    same = bool(np.array_equal(frames, frames_b) and torch.equal(pcm_a.view(torch.int32), pcm_b.view(torch.int32)))
    d, fr, nb = prep_b["desc"], np.zeros(len(files), np.int64), np.zeros(2, np.int64)
    ms = {"a_decode_streams": [], "b_decode_ogg": [], "c_host_demux": [], "host_scan_and_plan": []}

    def timed(key, fn):
        t0 = time.perf_counter()
        fn()
        ms[key].append(round((time.perf_counter() - t0) * 1e3, 3))
    for _ in range(a.reps):  # (each returns when its statuses are back: the stream is idle between them)
        timed("a_decode_streams", lambda: an.decode_run(prep_a, pcm_a))
        timed("b_decode_ogg", lambda: an.decode_ogg_run(prep_b, pcm_b))
        timed("c_host_demux", lambda: demux.run(files, out, sizes))
        timed("host_scan_and_plan", lambda: an.L.vamd_decode_ogg_plan(an.h, C.byref(d), C.c_void_p(fr.ctypes.data), C.c_void_p(nb.ctypes.data)))
    an.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"step": "time", "file_bytes": total, "packets": int(sum(n for n, _ in table)), "frames": int(frames.sum()),
            "flagged_streams": int((status_a != 0).sum() + (status_b != 0).sum()), "b_equals_a_bit_for_bit": same, "ms_reps": ms, "ms_median": med,
            "b_minus_a_plus_c_ms": round(med["b_decode_ogg"] - med["a_decode_streams"] - med["c_host_demux"], 3),
            "note": "a and b each include vamd_decode_plan / vamd_decode_ogg_plan once more than the decode call itself (decode_run plans, then decodes)"}


def step_trace(a):
    out = os.path.join(a.work, "trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "decode_ogg", "--", sys.executable, os.path.abspath(__file__),
           "--only", "time", "--work", a.work, "--reps", str(a.reps)]
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
                name = row.get("Kernel_Name", "")
                for k in ("k_ogg_depage", "k_unpack", "k_synth", "k_lap"):
                    if k in name.split("(")[0]:
                        launches.append((int(row["Start_Timestamp"]), k, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3,
                                         row.get("Grid_Size_X", row.get("Grid_Size", "?"))))
    launches.sort()
    kernels = {}
    for _, k, us, grid in launches:
        kernels.setdefault("%s grid %s" % (k, grid), []).append(round(us, 1))
    res = {"step": "trace", "us_per_launch_in_start_order": kernels}
    if not kernels:
        res["files"] = {os.path.relpath(p, out): open(p).readline().strip() for p in files}
    return res


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
    work = a.work or tempfile.mkdtemp(prefix="decode_ogg_bench_")
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
