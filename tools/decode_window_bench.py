"""Windows of Ogg files (vamd_ogg_index_create, vamd_decode_ogg_window: per window its own pages up, k_ogg_depage over them,
k_unpack, k_synth, k_lap_window) on tools/decode_ogg_bench.py's set: the FILES an Ogg feed makes of 64 streams x 20 s
stereo, VBR q 0.4 (the committed 44k_stereo_q4 blob), in host memory -- beside the whole-file entries on the same set,
vamd_decode_ogg and vamd_decode_streams, which a window must leave as fast as they were.

The driver starts every step as a process of its own under a time limit and stops at the first that fails; a step's result
is one JSON line, and the steps hand the files on in a file in --work.
    encode   tools/decode_ogg_bench.py's: the Ogg feed's files of the set, saved
    time     in ONE process, medians of --reps repeats each after a warm-up, interleaved rep by rep: index create; window
             calls of 64 x 1 s and 64 x 0.1 s at seeded starts and of 640 x 1 s, ten a file -- the decode call, and of it the
             host's share (vamd_decode_ogg_window_plan: the checks, the plan, the page rows; nothing enqueued) and the bytes
             and pages staged; decode_run over the files' packets and decode_ogg_run over the files.  Every window's PCM
             against the whole decode's frames, bit for bit.
    whole    tools/decode_ogg_bench.py's `time` step on the same files: the two whole-file entries in a process that runs
             nothing else between them
    parent   with --parent TREE (a built checkout of the parent commit): that tree's `time` step likewise, to hold `whole`
             against

    python tools/decode_window_bench.py --streams 64 --seconds 20 --reps 7 [--parent TREE] [--steps encode,time,whole,parent]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
LIMITS = {"encode": 240, "time": 300, "whole": 240, "parent": 240}  # seconds a step may take
RATE = 44100


def step_time(a):
    import torch
    import vorbis_amd
    from vorbis_amd.abi import _OggWindowDesc
    from tools.decode_ogg_bench import SETUP, HostDemux, load_files
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
    whole = pcm_b.clone()
    x = an.ogg_index(files)
    ns, ch, vp = len(files), an.channels, C.c_void_p
    rng = np.random.default_rng(30)
    sets = {}
    for key, per_file, length in (("64x1s", 1, RATE), ("64x0.1s", 1, RATE // 10), ("640x1s", 10, RATE)):
        stream = np.repeat(np.arange(ns, dtype=np.int64), per_file)
        start = np.array([int(rng.integers(0, max(1, int(x.frames[s]) - length))) for s in stream], np.int64)
        sets[key] = (stream, start, np.full(len(stream), length, np.int64))
    ms = {"a_decode_streams": [], "b_decode_ogg": [], "index_create": []}
    calls, report = {}, {}
    for key, (stream, start, count) in sets.items():
        pcm, fr, o, st = x._run(stream, start, count)  # (a warm-up, and the check)
        ok = not st.any()
        for w in range(len(stream)):
            s, a0, n = int(stream[w]), int(start[w]), int(fr[w])
            for c in range(ch):
                lo = int(off_b[s]) + c * int(frames_b[s]) + a0
                ok = ok and torch.equal(pcm[int(o[w]) + c * n:int(o[w]) + (c + 1) * n].view(torch.int32), whole[lo:lo + n].view(torch.int32))
        d = _OggWindowDesc(len(stream), vp(stream.ctypes.data), vp(start.ctypes.data), vp(count.ctypes.data), vp(x._data.ctypes.data), vp(x._off.ctypes.data), None)
        nb, staged, status = np.zeros(2, np.int64), np.zeros(2, np.int64), np.zeros(len(stream), np.uint8)
        an.L.vamd_decode_ogg_window_plan(an.h, x.h, C.byref(d), vp(fr.ctypes.data), vp(nb.ctypes.data), vp(staged.ctypes.data))
        calls[key] = (d, fr, nb, o, pcm, status)
        ms["window_" + key], ms["window_" + key + "_host_plan"] = [], []
        report[key] = {"windows": len(stream), "frames": int(fr.sum()), "blocks": [int(v) for v in nb], "bytes_staged": int(staged[0]),
                       "pages_staged": int(staged[1]), "equals_whole_decode_bit_for_bit": bool(ok)}

    def timed(key, fn):
        t0 = time.perf_counter()
        fn()
        ms[key].append(round((time.perf_counter() - t0) * 1e3, 3))

    def create():
        y = an.ogg_index(files)
        y.close()
    for _ in range(a.reps):  # (each returns when its statuses are back: the stream is idle between them)
        timed("a_decode_streams", lambda: an.decode_run(prep_a, pcm_a))
        timed("b_decode_ogg", lambda: an.decode_ogg_run(prep_b, pcm_b))
        timed("index_create", create)
        for key, (d, fr, nb, o, pcm, status) in calls.items():
            timed("window_" + key, lambda: an.L.vamd_decode_ogg_window(an.h, x.h, C.byref(d), vp(o.ctypes.data), vp(pcm.data_ptr()), vp(status.ctypes.data)))
            timed("window_" + key + "_host_plan", lambda: an.L.vamd_decode_ogg_window_plan(an.h, x.h, C.byref(d), vp(fr.ctypes.data), vp(nb.ctypes.data), None))
    an.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"step": "time", "file_bytes": total, "streams": ns, "frames_per_stream": int(frames[0]), "flagged_streams": int((status_a != 0).sum() + (status_b != 0).sum()),
            "b_equals_a_bit_for_bit": same, "windows": report, "ms_reps": ms, "ms_median": med,
            "note": "a and b include their plan call once more than the decode call itself (decode_run plans, then decodes), as in tools/decode_ogg_bench.py; "
                    "index_create includes joining the files' bytes in Python; a window call is the decode call alone, its host_plan the plan call alone "
                    "(the decode call plans the same way, then gathers the pages, uploads and runs)"}


def step_encode(a):
    from tools.decode_ogg_bench import step_encode as encode
    return encode(a)


def whole_file_entries(tree, a, step):
    """tools/decode_ogg_bench.py's `time` step of a tree on the files in --work -> the two whole-file entries' times"""
    cmd = [sys.executable, os.path.join(tree, "tools", "decode_ogg_bench.py"), "--only", "time", "--work", a.work, "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=tree, timeout=LIMITS[step] - 10)
    if r.returncode:
        raise RuntimeError("the step failed in %s: %s" % (tree, r.stderr[-2000:]))
    res = json.loads(r.stdout.strip().splitlines()[-1])
    return {"step": step, "ms_reps": {k: res["ms_reps"][k] for k in ("a_decode_streams", "b_decode_ogg")},
            "ms_median": {k: res["ms_median"][k] for k in ("a_decode_streams", "b_decode_ogg")}}


def step_whole(a):
    return whole_file_entries(ROOT, a, "whole")


def step_parent(a):
    if not a.parent:
        return {"step": "parent", "skipped": "no --parent tree"}
    return whole_file_entries(a.parent, a, "parent")


STEPS = {"encode": step_encode, "time": step_time, "whole": step_whole, "parent": step_parent}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", default="encode,time,whole,parent")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit, for the whole-file entries' times there")
    ap.add_argument("--work", default=None, help="where the steps keep the files (default: a temporary directory)")
    ap.add_argument("--only", choices=sorted(STEPS), default=None, help="run this one step in this process (the driver's children)")
    a = ap.parse_args()
    if a.only:
        a.files = os.path.join(a.work, "files.npz")
        print(json.dumps(STEPS[a.only](a)), flush=True)
        return 0
    work = a.work or tempfile.mkdtemp(prefix="decode_window_bench_")
    os.makedirs(work, exist_ok=True)
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--only", step, "--work", work, "--streams", str(a.streams),
               "--seconds", str(a.seconds), "--reps", str(a.reps)] + (["--parent", os.path.abspath(a.parent)] if a.parent else [])
        r = subprocess.run(cmd)
        if r.returncode:  # a step that failed, faulted or ran out of time ends the run: nothing more is started
            print(json.dumps({"step": step, "failed": r.returncode}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
