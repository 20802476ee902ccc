"""The host-fed farm on a bitrate-managed setup beside the VBR one: the same 16-bit stream set through a VBR q 0.4 blob
and an ABR 128 kb/s blob (tests/bitrate_host.managed_blob: the reference's vamd_pack_setup, oracle/_ref), the two
alternating in one process, blocks/s and packet bytes/s each (best of --reps, after a warm-up group).  One JSON line per setup.

    python tools/feed_managed_bench.py --streams 64 --seconds 20 --reps 3
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
    ap.add_argument("--only", choices=("vbr", "abr"), default=None, help="one setup only (for a trace of it)")
    a = ap.parse_args()
    import vorbis_amd
    from oracle import ref
    frames = int(44100 * a.seconds)
    rng = np.random.default_rng(1)
    t = np.arange(frames) / 44100.0
    pcm = np.empty((a.streams, frames, 2), np.int16)
    for s in range(a.streams):  # music-like: tones over noise, loudness swinging
        env = 0.05 + 0.4 * (np.sin(2 * np.pi * (0.7 + 0.01 * s) * t) > 0)
        x = env[:, None] * (0.5 * np.sin(2 * np.pi * (220 + 7 * s) * t)[:, None] + (rng.random((frames, 2)) - 0.5) * 0.4)
        pcm[s] = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    from tests import bitrate_host
    setups = {"vbr": ref.RefEncoder(2, 44100, 0.4).pack_setup(), "abr": bitrate_host.managed_blob(2, (-1, 128000, -1))}
    names = [a.only] if a.only else ["vbr", "abr"]
    feeds = {k: vorbis_amd.Feed(setups[k], lanes_per_device=a.lanes, max_streams=a.streams, max_frames=frames) for k in names}
    best = {k: None for k in names}
    flat = pcm.reshape(-1)
    for rep in range(a.reps + 1):
        for k in names:
            f = feeds[k]
            slot, buf = f.buffer(2)
            buf[:flat.size] = flat
            t0 = time.perf_counter()
            f.wrote(slot, a.streams, frames)
            r = f.packets(slot, copy=False)
            dt = time.perf_counter() - t0
            nb, nbytes, dev = r["nblocks"], r["total_bytes"], r["device_ms"]
            f.release(slot)
            if rep and (best[k] is None or dt < best[k][0]):
                best[k] = (dt, nb, nbytes, dev)
    for k in names:
        dt, nb, nbytes, dev = best[k]
        print(json.dumps({"setup": k, "streams": a.streams, "seconds": a.seconds, "blocks": nb, "wall_s": dt, "device_ms": dev,
                          "blocks_per_s": nb / dt, "packet_bytes_per_s": nbytes / dt, "kbps": nbytes * 8 / a.seconds / a.streams / 1e3}))
    for f in feeds.values():
        f.close()


if __name__ == "__main__":
    main()
