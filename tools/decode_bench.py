"""The packet decoder (vamd_decode_streams: k_unpack, k_synth, k_lap) on tools/feed_decoded_bench.py's workload: 64 streams x
20 s stereo, VBR q 0.4 (the committed 44k_stereo_q4 blob) -- the packets a feed makes of them, in host memory, to PCM on the
device -- beside libvorbis' decoder on the CPU over the same packets.

The driver starts every step as a process of its own under a time limit and stops at the first that fails; a step's result
is one JSON line, and the steps hand the packets on in a file in --work.
    encode   the feed's packets of the set (a plain device-fed feed), saved
    time     decode_run() end to end, --reps repeats after a warm-up: ms per group, blocks/s; the PCM against the CPU
             decoder's for the first streams
    phases   k_unpack's in-kernel stopwatch (vamd_debug_cycles): head / floors / residues
    trace    rocprofv3 --kernel-trace --stats over `time`: k_unpack, k_synth, k_lap in us per launch
    cpu      ref_host.reference_decode over the same packets, a process per stream on --cpus CPUs

    python tools/decode_bench.py --streams 64 --seconds 20 --reps 5 [--steps encode,time,phases,trace,cpu]
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
SETUP = "44k_stereo_q4"
LIMITS = {"encode": 240, "time": 240, "phases": 120, "trace": 300, "cpu": 540}  # seconds a step may take


def save_rows(path, rows):
    flat = [p for row in rows for p, _, _, _ in row]
    np.savez(path, bytes=np.frombuffer(b"".join(flat), np.uint8), lengths=np.array([len(p) for p in flat], np.int64),
             counts=np.array([len(row) for row in rows], np.int64), granules=np.array([g for row in rows for _, g, _, _ in row], np.int64))


def load_rows(path):
    """-> per stream (packets, granules)"""
    z = np.load(path)
    data, ends = z["bytes"].tobytes(), np.concatenate([[0], np.cumsum(z["lengths"])])
    packets = [data[int(ends[k]):int(ends[k + 1])] for k in range(len(z["lengths"]))]
    out, at = [], 0
    for n in z["counts"]:
        out.append((packets[at:at + int(n)], [int(g) for g in z["granules"][at:at + int(n)]]))
        at += int(n)
    return out


def step_encode(a):
    import torch
    import vorbis_amd
    from tools.feed_device_bench import stream_set
    frames = int(44100 * a.seconds)
    pcm = stream_set(a.streams, frames)
    src = (torch.from_numpy(np.ascontiguousarray(pcm.transpose(0, 2, 1))).cuda().float() / 32768.0).contiguous()
    feed = vorbis_amd.Feed(vorbis_amd.default_setup_blob(SETUP), lanes_per_device=1, max_streams=a.streams, max_frames=frames,
                           fmt=vorbis_amd.FEED_S16 | vorbis_amd.FEED_NO_ARENA)
    try:
        rows = feed.encode_tensors(src)
    finally:
        feed.close()
    save_rows(a.packets, rows)
    return {"step": "encode", "streams": a.streams, "seconds": a.seconds, "blocks": sum(len(r) for r in rows),
            "short_blocks": sum(1 for r in rows for _, _, W, _ in r if not W), "packet_bytes": sum(len(p) for r in rows for p, _, _, _ in r)}


def _reference(args):
    from tests import ref_host
    headers, packets, granules = args
    return ref_host.reference_decode(headers + packets, granules)


def step_time(a):
    import torch
    import vorbis_amd
    from tests import ref_host
    rows = load_rows(a.packets)
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(SETUP), 0)
    prep = an.decode_prepare([p for p, _ in rows], [g[-1] for _, g in rows])
    pcm, frames, off, status = an.decode_run(prep)  # warm-up: the tables, the workspace
    torch.cuda.synchronize()
    ms = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        an.decode_run(prep, pcm)  # (returns when the statuses are back: the stream is idle)
        ms.append((time.perf_counter() - t0) * 1e3)
    headers = ref_host.reference_headers(2, 44100, 0.4)
    same = 0
    for s in range(min(2, len(rows))):
        want = _reference((headers, rows[s][0], rows[s][1]))
        got = pcm[int(off[s]):int(off[s]) + 2 * int(frames[s])].view(2, int(frames[s])).cpu().numpy()
        same += int(got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32)))
    an.close()
    blocks = sum(len(p) for p, _ in rows)
    return {"step": "time", "blocks": blocks, "frames": int(frames.sum()), "flagged_streams": int((status != 0).sum()), "ms_reps": [round(x, 3) for x in ms],
            "blocks_per_s": blocks / (min(ms) * 1e-3), "streams_equal_to_the_cpu_decoder": "%d of %d compared" % (same, min(2, len(rows)))}


def step_phases(a):
    import torch
    import vorbis_amd
    rows = load_rows(a.packets)
    an = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob(SETUP), 0)
    prep = an.decode_prepare([p for p, _ in rows], [g[-1] for _, g in rows])
    pcm = an.decode_run(prep)[0]
    an.debug_cycles(True)
    an.decode_run(prep, pcm)
    torch.cuda.synchronize()
    c = an.debug_cycles(False, read=True).reshape(-1)  # the 80 slots
    an.close()
    waves = (sum(len(p) for p, _ in rows) + 63) // 64
    k = [float(x) / waves / 1e3 for x in c[56:59]]  # k_unpack's slots: head, floors, residues
    return {"step": "phases", "waves": waves, "kcycles_per_wave": {"head": round(k[0], 2), "floors": round(k[1], 2), "residues": round(k[2], 2)},
            "share_percent": {n: round(100 * x / max(sum(k), 1e-9), 1) for n, x in zip(("head", "floors", "residues"), k)}}


def step_trace(a):
    out = os.path.join(a.work, "trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "decode", "--", sys.executable, os.path.abspath(__file__),
           "--only", "time", "--work", a.work, "--reps", str(a.reps)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS["trace"] - 10)
    if r.returncode:
        raise RuntimeError("rocprofv3 failed: " + r.stderr[-2000:])
    # every launch of the three kernels, in start order: us, with the grid that tells k_synth's size classes apart
    launches = []
    files = glob.glob(os.path.join(out, "**", "*.csv"), recursive=True)
    for path in files:
        if not path.endswith("kernel_trace.csv"):
            continue
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                for k in ("k_unpack", "k_synth", "k_lap"):
                    if name.startswith(k):
                        launches.append((int(row["Start_Timestamp"]), k, (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e3,
                                         row.get("Grid_Size_X", row.get("Grid_Size", "?"))))
    launches.sort()
    kernels = {}
    for _, k, us, grid in launches:
        kernels.setdefault("%s grid %s" % (k, grid), []).append(round(us, 1))
    res = {"step": "trace", "us_per_launch_the_first_is_the_warm_up": kernels}
    if not kernels:
        res["files"] = {os.path.relpath(p, out): open(p).readline().strip() for p in files}  # (another rocprofv3's names: say which)
    return res


def step_cpu(a):
    from multiprocessing import Pool
    from tests import ref_host
    rows = load_rows(a.packets)
    headers = ref_host.reference_headers(2, 44100, 0.4)
    t0 = time.perf_counter()
    with Pool(a.cpus) as pool:
        frames = sum(x.shape[1] for x in pool.imap_unordered(_reference, [(headers, p, g) for p, g in rows]))
    dt = time.perf_counter() - t0
    blocks = sum(len(p) for p, _ in rows)
    return {"step": "cpu", "cpus": a.cpus, "frames": int(frames), "ms": round(dt * 1e3, 1), "blocks_per_s": blocks / dt}


STEPS = {"encode": step_encode, "time": step_time, "phases": step_phases, "trace": step_trace, "cpu": step_cpu}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cpus", type=int, default=16)
    ap.add_argument("--steps", default="encode,time,phases,trace,cpu")
    ap.add_argument("--work", default=None, help="where the steps keep the packets (default: a temporary directory)")
    ap.add_argument("--only", choices=sorted(STEPS), default=None, help="run this one step in this process (the driver's children)")
    a = ap.parse_args()
    if a.only:
        a.packets = os.path.join(a.work, "packets.npz")
        print(json.dumps(STEPS[a.only](a)), flush=True)
        return 0
    work = a.work or tempfile.mkdtemp(prefix="decode_bench_")
    os.makedirs(work, exist_ok=True)
    for step in a.steps.split(","):
        cmd = ["timeout", "-k", "10", str(LIMITS[step]), sys.executable, os.path.abspath(__file__), "--only", step, "--work", work, "--streams", str(a.streams),
               "--seconds", str(a.seconds), "--reps", str(a.reps), "--cpus", str(a.cpus)]
        r = subprocess.run(cmd)
        if r.returncode:  # a step that failed, faulted or ran out of time ends the run: nothing more is started
            print(json.dumps({"step": step, "failed": r.returncode}), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
