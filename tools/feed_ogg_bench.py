"""The host-fed farm as a packet feed and as an Ogg feed (vamd_feed_ogg_headers: complete Ogg Vorbis files back, framed on
the device): the same 16-bit stream set through both, alternating in one process, VBR q 0.4 (the committed
44k_stereo_q4 blob); blocks/s, packet bytes/s and, for the Ogg feed, file bytes/s (best of --reps, after a warm-up
group).  One JSON line per feed.  The packet half uses only calls older libraries have too (--only packets), so the
tool can be run beside an earlier checkout for a before/after of the packet feed.

    python tools/feed_ogg_bench.py --streams 64 --seconds 20 --reps 3
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--only", choices=("packets", "ogg"), default=None, help="one feed only (for a trace of it, or an older library)")
    a = ap.parse_args()
    import vorbis_amd
    frames = int(44100 * a.seconds)
    rng = np.random.default_rng(1)
    t = np.arange(frames) / 44100.0
    pcm = np.empty((a.streams, frames, 2), np.int16)
    for s in range(a.streams):  # music-like: tones over noise, loudness swinging (tools/feed_managed_bench.py's set)
        env = 0.05 + 0.4 * (np.sin(2 * np.pi * (0.7 + 0.01 * s) * t) > 0)
        x = env[:, None] * (0.5 * np.sin(2 * np.pi * (220 + 7 * s) * t)[:, None] + (rng.random((frames, 2)) - 0.5) * 0.4)
        pcm[s] = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    blob = vorbis_amd.default_setup_blob("44k_stereo_q4")
    names = [a.only] if a.only else ["packets", "ogg"]
    feeds = {}
    for k in names:
        kw = {}
        if k == "ogg":
            from tests import ogg_host
            kw["ogg_headers"] = ogg_host.reference_headers(2, 44100, 0.4)  # (needs the reference build, oracle/_ref)
        feeds[k] = vorbis_amd.Feed(blob, lanes_per_device=a.lanes, max_streams=a.streams, max_frames=frames, **kw)
    best = {k: None for k in names}
    flat = pcm.reshape(-1)
    for rep in range(a.reps + 1):
        for k in names:
            f = feeds[k]
            slot, buf = f.buffer(2)
            buf[:flat.size] = flat
            t0 = time.perf_counter()
            f.wrote(slot, a.streams, frames)
            file_bytes = 0
            if k == "ogg":
                file_bytes = f.ogg(slot, copy=False)["total_bytes"]
            r = f.packets(slot, copy=False)
            dt = time.perf_counter() - t0
            nb, nbytes, dev = r["nblocks"], r["total_bytes"], r["device_ms"]
            f.release(slot)
            if rep and (best[k] is None or dt < best[k][0]):
                best[k] = (dt, nb, nbytes, dev, file_bytes)
    for k in names:
        dt, nb, nbytes, dev, file_bytes = best[k]
        line = {"feed": k, "streams": a.streams, "seconds": a.seconds, "blocks": nb, "wall_s": dt, "device_ms": dev,
                "blocks_per_s": nb / dt, "packet_bytes_per_s": nbytes / dt}
        if k == "ogg":
            line["file_bytes_per_s"] = file_bytes / dt
            line["file_bytes"] = file_bytes
        print(json.dumps(line))
    for f in feeds.values():
        f.close()


if __name__ == "__main__":
    main()
