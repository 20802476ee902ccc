"""The decoded feed (VAMD_FEED_DECODED, vamd_feed_decoded) on tools/feed_device_bench.py's device-fed workload: 64 streams x
20 s stereo, VBR q 0.4 (the committed 44k_stereo_q4 blob), a resident fp32 (streams, 2, frames) tensor.

Cases, alternating in one process, --reps timed repeats each after a warm-up group; one JSON line per case:
    plain      a feed without the flag: wrote_device() -> packets()                       (the unchanged path)
    decoded    a feed with it: wrote_device() -> packets() -> decoded(copy=False)          packets_wall_s: until packets()
               returned; wall_s: until the decoded signal was complete; extra HBM per lane from the group's shapes

    python tools/feed_decoded_bench.py --streams 64 --seconds 20 --reps 5
    python tools/feed_decoded_bench.py --only plain     # runs on a library without the flag too (the parent commit's)
    rocprofv3 --kernel-trace --stats -- python tools/feed_decoded_bench.py --only decoded --reps 2    # k_synth / k_lap / k_transform
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.feed_device_bench import stream_set  # noqa: E402


def one_group(f, src, decoded):
    slot, _ = f.buffer()
    t0 = time.perf_counter()
    f.wrote_device(slot, src, layout="scf")
    r = f.packets(slot, copy=False)
    t_packets = time.perf_counter() - t0
    frames = None
    if decoded:
        dec = f.decoded(slot, copy=False)
        frames = sum(int(d.shape[1]) for d in dec)
    dt = time.perf_counter() - t0
    res = {"blocks": int(r["nblocks"]), "short_blocks": int((np.asarray(r["info"]) & 1 == 0).sum()), "total_ms": r["total_ms"],
           "device_ms": r["device_ms"], "frames": frames}
    f.release(slot)
    return dt, t_packets, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--only", choices=("plain", "decoded"), default=None)
    a = ap.parse_args()
    import torch
    import vorbis_amd
    frames = int(44100 * a.seconds)
    pcm = stream_set(a.streams, frames)
    src = (torch.from_numpy(np.ascontiguousarray(pcm.transpose(0, 2, 1))).cuda().float() / 32768.0).contiguous()
    torch.cuda.synchronize()
    blob = vorbis_amd.default_setup_blob("44k_stereo_q4")
    cases = [c for c in ("plain", "decoded") if a.only in (None, c)]
    fmt = vorbis_amd.FEED_S16 | vorbis_amd.FEED_NO_ARENA
    feeds = {c: vorbis_amd.Feed(blob, lanes_per_device=a.lanes, max_streams=a.streams, max_frames=frames, fmt=fmt,
                                **({"decoded": True} if c == "decoded" else {})) for c in cases}
    runs = {c: [] for c in cases}
    for rep in range(a.reps + 1):
        for c, f in feeds.items():
            got = one_group(f, src, c == "decoded")
            if rep:
                runs[c].append(got)
    for c in cases:
        dt, t_packets, res = min(runs[c], key=lambda x: x[0])
        line = {"case": c, "streams": a.streams, "seconds": a.seconds, "blocks": res["blocks"], "blocks_per_s": res["blocks"] / dt,
                "wall_ms_reps": [round(x[0] * 1e3, 3) for x in runs[c]], "packets_wall_ms_reps": [round(x[1] * 1e3, 3) for x in runs[c]],
                "total_ms_reps": [round(x[2]["total_ms"], 3) for x in runs[c]], "device_ms_reps": [round(x[2]["device_ms"], 3) for x in runs[c]]}
        if c == "decoded":
            ch, bs = 2, (256, 2048)
            group = a.streams * frames * ch
            line["decoded_frames"] = res["frames"]
            # what a lane of a decoded feed holds beyond a plain one's (vamd_feed.hip, feed_create / enqueue_decoded)
            line["extra_hbm_bytes_per_lane"] = {"decoded_arena": (group + 4) * 4, "scratch_long": (2 * group + a.streams * 4 * bs[1] * ch) * 4,
                                                "scratch_short": (res["short_blocks"] * ch * bs[0] + 4) * 4}
        print(json.dumps(line), flush=True)
    for f in feeds.values():
        f.close()


if __name__ == "__main__":
    main()
