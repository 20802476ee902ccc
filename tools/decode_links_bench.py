"""What the follow policy (vamd_decode_follow: links, foreign pages, the page granules' cuts) costs on
tools/decode_ogg_bench.py's set: the FILES an Ogg feed makes of 64 streams x 20 s stereo, VBR q 0.4, in host memory, to
PCM on the device.  The policy is host work -- the page walk keeps a mark per packet and the plan walks them -- plus
k_lap_segments in k_lap's place.

The driver starts every step as a process of its own under a time limit and stops at the first that fails; a step's
result is one JSON line, and the steps hand the files on in files in --work.
    encode   tools/decode_ogg_bench.py's: the Ogg feed's files of the set, saved
    recut    the same packets as four links a file (each link its own headers and serial number, eight packets a page,
             granule positions counted from 0 per link), saved
    time     in ONE process, --reps repeats each after a warm-up, interleaved rep by rep: decode_ogg_run over the clean
             files with the policy off, the same with it on, and the re-cut files with it on; and the host scan and plan
             alone (vamd_decode_ogg_plan) for each of the three.  On against off, bit for bit, on the clean files.

    python tools/decode_links_bench.py --streams 64 --seconds 20 --reps 7 [--steps encode,recut,time]
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
from tools.decode_ogg_bench import SETUP, load_files, step_encode  # noqa: E402

LINKS = 4
LIMITS = {"encode": 240, "recut": 400, "time": 240}  # seconds a step may take


def step_recut(a):
    from tests import ogg_demux_cases as w
    from tests import ogg_framing
    files, out = load_files(a.files), []
    bs = (256, 2048)  # the setup's block sizes
    for s, f in enumerate(files):
        packets = ogg_framing.packets_of(ogg_framing.pages_of(f))
        headers, audio = packets[:3], packets[3:]
        cuts = [len(audio) * k // LINKS for k in range(LINKS + 1)]
        links = []
        for k in range(LINKS):
            part = audio[cuts[k]:cuts[k + 1]]
            Ws = [(p[0] >> 1) & 1 for p in part]
            gr, at = [], 0
            for i in range(len(part)):
                at += bs[Ws[i - 1]] // 4 + bs[Ws[i]] // 4 if i else 0
                gr.append(at)
            links.append(w.write(headers + part, [0, 0, 0] + gr, lambda seq, at_, segs: w._to_packet_end(seq, at_, segs, 1 if seq == 0 else 2 if seq == 1 else 8),
                                 0x10000 * (s + 1) + k))
        out.append(b"".join(links))
    np.savez(a.recut, bytes=np.frombuffer(b"".join(out), np.uint8), lengths=np.array([len(f) for f in out], np.int64))
    return {"step": "recut", "links_a_file": LINKS, "file_bytes": sum(len(f) for f in out)}


def step_time(a):
    import torch
    import vorbis_amd
    clean, chained = load_files(a.files), load_files(a.recut)
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(SETUP), 0)
    prep = {"clean": an.decode_ogg_prepare(clean), "links": an.decode_ogg_prepare(chained)}
    runs = (("off_clean", "clean", False), ("on_clean", "clean", True), ("on_links", "links", True))
    pcm, frames, status = {}, {}, {}
    for key, which, on in runs:  # warm-ups: the tables, the workspaces
        an.follow_links = on
        pcm[key], frames[key], _, status[key] = an.decode_ogg_run(prep[which])
    torch.cuda.synchronize()
    same = bool(np.array_equal(frames["off_clean"], frames["on_clean"]) and
                torch.equal(pcm["off_clean"].view(torch.int32), pcm["on_clean"].view(torch.int32)))
    fr, nb = np.zeros(len(clean), np.int64), np.zeros(2, np.int64)
    ms = {k: [] for k, _, _ in runs}
    ms.update({"plan_" + k: [] for k, _, _ in runs})

    def timed(key, fn):
        t0 = time.perf_counter()
        fn()
        ms[key].append(round((time.perf_counter() - t0) * 1e3, 3))
    for _ in range(a.reps):  # (each returns when its statuses are back: the stream is idle between them)
        for key, which, on in runs:
            an.follow_links = on
            timed(key, lambda: an.decode_ogg_run(prep[which], pcm[key]))
            d = prep[which]["desc"]
            timed("plan_" + key, lambda: an.L.vamd_decode_ogg_plan(an.h, C.byref(d), C.c_void_p(fr.ctypes.data), C.c_void_p(nb.ctypes.data)))
    an.close()
    med = {k: float(np.median(v)) for k, v in ms.items()}
    return {"step": "time", "files": len(clean), "file_bytes": {"clean": sum(map(len, clean)), "links": sum(map(len, chained))},
            "frames": {k: int(v.sum()) for k, v in frames.items()}, "flagged": {k: int((v != 0).sum()) for k, v in status.items()},
            "on_equals_off_bit_for_bit": same, "ms_reps": ms, "ms_median": med, "ms_min_max": {k: [min(v), max(v)] for k, v in ms.items()},
            "on_minus_off_ms": round(med["on_clean"] - med["off_clean"], 3), "links_minus_on_ms": round(med["on_links"] - med["on_clean"], 3),
            "note": "each decode figure includes vamd_decode_ogg_plan once more than the decode call itself (decode_ogg_run plans, then decodes)"}


STEPS = {"encode": step_encode, "recut": step_recut, "time": step_time}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", default="encode,recut,time")
    ap.add_argument("--work", default=None, help="where the steps keep the files (default: a temporary directory)")
    ap.add_argument("--only", choices=sorted(STEPS), default=None, help="run this one step in this process (the driver's children)")
    a = ap.parse_args()
    if a.only:
        a.files, a.recut = os.path.join(a.work, "files.npz"), os.path.join(a.work, "links.npz")
        print(json.dumps(STEPS[a.only](a)), flush=True)
        return 0
    work = a.work or tempfile.mkdtemp(prefix="decode_links_bench_")
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
