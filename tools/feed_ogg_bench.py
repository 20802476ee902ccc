"""The host-fed farm as a packet feed and as an Ogg feed (vamd_feed_ogg_headers: complete Ogg Vorbis files back, framed on
the device): the same 16-bit stream set through both, alternating in one process, VBR q 0.4 (the committed
44k_stereo_q4 blob); blocks/s, packet bytes/s and, for the Ogg feed, file bytes/s (best of --reps, after a warm-up
group).  One JSON line per feed.  The packet half uses only calls older libraries have too (--only packets), so the
tool can be run beside an earlier checkout for a before/after of the packet feed.

    python tools/feed_ogg_bench.py --streams 64 --seconds 20 --reps 3

--live: the same pair as LIVE feeds (vamd_feed_create_live, one lane: a lane's streams are its own) -- the set fed in
--piece second pieces, every stream closed with its last; the Ogg feed (vamd_feed_ogg_headers_live) returns the files in
pieces.  Per feed the whole set's blocks/s and bytes/s and the mean time per group (best of --reps passes over the set).

    python tools/feed_ogg_bench.py --live --streams 64 --seconds 20 --piece 1 --reps 3

--tags BYTES: every stream of the Ogg feed gets a comment header of its own of about BYTES bytes (vamd_feed_ogg_comments;
a title and a padding tag), handed over inside the timed part of every group -- of a live feed, of the group that begins
the streams.  wall_s_reps: every timed repetition's wall time, in order (wall_s is their best).

    python tools/feed_ogg_bench.py --streams 64 --seconds 20 --reps 3 --tags 65536

--flush (with --live): the Ogg feed flushes every stream in every group (vamd_feed_ogg_flush, inside the timed part), so
each group returns every stream's open page too; `pages` counts all pages the set handed out (with and without --flush, so
the difference is the flushed ones), file_bytes shows the growth.

    python tools/feed_ogg_bench.py --live --streams 64 --seconds 20 --piece 0.1 --reps 3 --flush
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
    ap.add_argument("--live", action="store_true", help="live feeds: the streams in pieces, the Ogg files in pieces")
    ap.add_argument("--piece", type=float, default=1.0, help="--live: seconds per piece")
    ap.add_argument("--tags", type=int, default=0, help="the Ogg feed: a comment header of its own per stream, of about this many bytes")
    ap.add_argument("--flush", action="store_true", help="--live: the Ogg feed flushes every stream in every group")
    a = ap.parse_args()
    if a.flush and not a.live:
        ap.error("--flush goes with --live: a whole stream's file has no open page to flush")
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
    a.comments = None
    if a.tags:
        a.comments = [vorbis_amd.comment_packet([("TITLE", "stream %d" % s), ("PAD", "x" * max(0, a.tags - 64))], "vorbis_amd feed_ogg_bench")
                      for s in range(a.streams)]
    if a.live:
        return live(a, vorbis_amd, blob, pcm, names)
    feeds = {}
    for k in names:
        kw = {}
        if k == "ogg":
            from tests import ref_host
            kw["ogg_headers"] = ref_host.reference_headers(2, 44100, 0.4)  # (needs the reference build, oracle/_ref)
        feeds[k] = vorbis_amd.Feed(blob, lanes_per_device=a.lanes, max_streams=a.streams, max_frames=frames, **kw)
    best = {k: None for k in names}
    walls = {k: [] for k in names}
    flat = pcm.reshape(-1)
    for rep in range(a.reps + 1):
        for k in names:
            f = feeds[k]
            slot, buf = f.buffer(2)
            buf[:flat.size] = flat
            t0 = time.perf_counter()
            if k == "ogg" and a.comments:
                f.ogg_comments(slot, a.comments)
            f.wrote(slot, a.streams, frames)
            file_bytes = 0
            if k == "ogg":
                file_bytes = f.ogg(slot, copy=False)["total_bytes"]
            r = f.packets(slot, copy=False)
            dt = time.perf_counter() - t0
            nb, nbytes, dev = r["nblocks"], r["total_bytes"], r["device_ms"]
            f.release(slot)
            if rep:
                walls[k].append(dt)
            if rep and (best[k] is None or dt < best[k][0]):
                best[k] = (dt, nb, nbytes, dev, file_bytes)
    for k in names:
        dt, nb, nbytes, dev, file_bytes = best[k]
        line = {"feed": k, "streams": a.streams, "seconds": a.seconds, "blocks": nb, "wall_s": dt, "device_ms": dev,
                "blocks_per_s": nb / dt, "packet_bytes_per_s": nbytes / dt, "wall_s_reps": walls[k]}
        if k == "ogg":
            line["file_bytes_per_s"] = file_bytes / dt
            line["file_bytes"] = file_bytes
            line["tags"] = a.tags
        print(json.dumps(line))
    for f in feeds.values():
        f.close()


def live(a, vorbis_amd, blob, pcm, names):
    frames, piece = pcm.shape[1], int(44100 * a.piece)
    feeds = {}
    for k in names:
        kw = {}
        if k == "ogg":
            from tests import ref_host
            kw["ogg_headers"] = ref_host.reference_headers(2, 44100, 0.4)  # (needs the reference build, oracle/_ref)
        feeds[k] = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=a.streams, max_frames=piece, write_frames=1024, **kw)
    best = {k: None for k in names}
    walls = {k: [] for k in names}
    for rep in range(a.reps + 1):
        for k in names:
            f = feeds[k]
            dt = dev = 0.0
            nb = nbytes = file_bytes = groups = pages = 0
            for at in range(0, frames, piece):
                flat = np.ascontiguousarray(pcm[:, at:at + piece]).reshape(-1)
                n = min(piece, frames - at)
                slot, buf = f.buffer(2)
                buf[:flat.size] = flat
                t0 = time.perf_counter()
                if k == "ogg" and a.comments and at == 0:
                    f.ogg_comments(slot, a.comments)
                if k == "ogg" and a.flush:
                    f.ogg_flush(slot, True)
                f.wrote_live(slot, [n] * a.streams, [at + piece >= frames] * a.streams)
                if k == "ogg":
                    o = f.ogg(slot, copy=False)
                    file_bytes += o["total_bytes"]
                    pages += int(np.sum(o["npages"]))
                r = f.packets(slot, copy=False)
                dt += time.perf_counter() - t0
                nb, nbytes, dev, groups = nb + r["nblocks"], nbytes + r["total_bytes"], dev + r["device_ms"], groups + 1
                f.release(slot)
            if rep:
                walls[k].append(dt)
            if rep and (best[k] is None or dt < best[k][0]):
                best[k] = (dt, nb, nbytes, dev, file_bytes, groups, pages)
    for k in names:
        dt, nb, nbytes, dev, file_bytes, groups, pages = best[k]
        line = {"feed": "live " + k, "streams": a.streams, "seconds": a.seconds, "piece_s": a.piece, "groups": groups, "blocks": nb,
                "wall_s": dt, "group_ms": 1e3 * dt / groups, "group_device_ms": dev / groups, "blocks_per_s": nb / dt,
                "packet_bytes_per_s": nbytes / dt, "wall_s_reps": walls[k]}
        if k == "ogg":
            line["file_bytes_per_s"] = file_bytes / dt
            line["file_bytes"] = file_bytes
            line["tags"] = a.tags
            line["flush"] = bool(a.flush)
            line["pages"] = pages
        print(json.dumps(line))
    for f in feeds.values():
        f.close()


if __name__ == "__main__":
    main()
