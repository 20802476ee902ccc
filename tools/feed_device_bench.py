"""The feed from samples that are already in device memory (vamd_feed_wrote_device) beside the host-fed feed, on README's
Ogg row: 64 streams x 20 s stereo, VBR q 0.4 (the committed 44k_stereo_q4 blob), the same 16-bit stream set throughout.

Cases, alternating in one process, --reps timed repeats each after a warm-up group:
    host s16            the pinned arena, as tools/feed_ogg_bench.py runs it (the samples are in the arena before the clock starts)
    dev s16 interleaved a resident (streams, frames, 2) int16 tensor
    dev f32 / f16 / bf16 planar   resident (streams, 2, frames) tensors
each as a packet feed and as an Ogg feed; then ABR 128 once (host s16 and dev f32, packets), and a live feed in --piece second
pieces (host s16 and dev f32, packets and Ogg).  One JSON line per case: blocks/s (best repeat), every repeat's wall time,
per-group total_ms and device_ms (of the best repeat), and for device-fed cases check_ms: the host's time inside
wrote_device (the per-stream pointer and range check, the producer's event) of that repeat.

    python tools/feed_device_bench.py --streams 64 --seconds 20 --reps 5
    python tools/feed_device_bench.py --only host      # the host-fed cases alone: runs on a library without the device-fed calls
    rocprofv3 --kernel-trace --stats -- python tools/feed_device_bench.py --only ingest --reps 2    # the ingest kernels' own times
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stream_set(streams, frames):
    rng = np.random.default_rng(1)
    t = np.arange(frames) / 44100.0
    pcm = np.empty((streams, frames, 2), np.int16)
    for s in range(streams):  # music-like: tones over noise, loudness swinging (tools/feed_ogg_bench.py's set)
        env = 0.05 + 0.4 * (np.sin(2 * np.pi * (0.7 + 0.01 * s) * t) > 0)
        x = env[:, None] * (0.5 * np.sin(2 * np.pi * (220 + 7 * s) * t)[:, None] + (rng.random((frames, 2)) - 0.5) * 0.4)
        pcm[s] = np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    return pcm


def sources(pcm, names):
    """the resident tensors of the device-fed cases: name -> (tensor, layout)"""
    import torch
    out = {}
    planar = None
    for k in names:
        if k == "host":
            continue
        if k == "dev_s16":
            out[k] = (torch.from_numpy(pcm).cuda(), "sfc")
            continue
        if planar is None:
            planar = (torch.from_numpy(np.ascontiguousarray(pcm.transpose(0, 2, 1))).cuda().float() / 32768.0).contiguous()
        out[k] = ({"dev_f32": planar, "dev_f16": planar.half(), "dev_bf16": planar.bfloat16()}[k], "scf")
    torch.cuda.synchronize()
    return out


def one_group(f, k, pcm_flat, src, ns, frames, ogg):
    """-> (wall s, check ms, result dict, file bytes)"""
    slot, buf = f.buffer(2) if k == "host" else f.buffer()
    if k == "host":
        buf[:pcm_flat.size] = pcm_flat
    t0 = time.perf_counter()
    check_ms = 0.0
    if k == "host":
        f.wrote(slot, ns, frames)
    else:
        f.wrote_device(slot, src[0], layout=src[1])
        check_ms = (time.perf_counter() - t0) * 1e3
    file_bytes = f.ogg(slot, copy=False)["total_bytes"] if ogg else 0
    r = f.packets(slot, copy=False)
    dt = time.perf_counter() - t0
    res = {"blocks": int(r["nblocks"]), "packet_bytes": int(r["total_bytes"]), "total_ms": r["total_ms"], "device_ms": r["device_ms"],
           "upload_ms": r["upload_ms"]}
    f.release(slot)
    return dt, check_ms, res, file_bytes


def report(name, streams, seconds, runs):
    """runs: the timed repeats [(wall, check_ms, res, file_bytes)] -> one JSON line"""
    best = min(runs, key=lambda x: x[0])
    dt, check_ms, res, file_bytes = best
    line = {"case": name, "streams": streams, "seconds": seconds, "blocks": res["blocks"], "blocks_per_s": res["blocks"] / dt, "wall_s": dt,
            "wall_s_reps": [round(x[0], 6) for x in runs], "total_ms": res["total_ms"], "device_ms": res["device_ms"],
            "upload_ms": res["upload_ms"], "total_ms_reps": [round(x[2]["total_ms"], 3) for x in runs],
            "device_ms_reps": [round(x[2]["device_ms"], 3) for x in runs]}
    if not name.startswith("host"):
        line["check_ms"] = check_ms
        line["check_ms_reps"] = [round(x[1], 4) for x in runs]
    if file_bytes:
        line["file_bytes"] = file_bytes
    print(json.dumps(line), flush=True)


def whole(a, vorbis_amd, blob, pcm, names, tag, headers):
    ns, frames = pcm.shape[0], pcm.shape[1]
    src = sources(pcm, names)
    flat = pcm.reshape(-1)
    kinds = [False] + ([True] if headers is not None else [])
    feeds = {}
    for k in names:
        for ogg in kinds:
            kw = {"ogg_headers": headers} if ogg else {}
            fmt = vorbis_amd.FEED_S16 if k == "host" else vorbis_amd.FEED_S16 | vorbis_amd.FEED_NO_ARENA
            feeds[k, ogg] = vorbis_amd.Feed(blob, lanes_per_device=a.lanes, max_streams=ns, max_frames=frames, fmt=fmt, **kw)
    runs = {key: [] for key in feeds}
    for rep in range(a.reps + 1):
        for key, f in feeds.items():
            got = one_group(f, key[0], flat, src.get(key[0]), ns, frames, key[1])
            if rep:
                runs[key].append(got)
    for key in feeds:
        report("%s%s %s" % (key[0], tag, "ogg" if key[1] else "packets"), ns, a.seconds, runs[key])
    for f in feeds.values():
        f.close()


def live(a, vorbis_amd, blob, pcm, names, headers):
    import torch
    ns, frames, piece = pcm.shape[0], pcm.shape[1], int(44100 * a.piece)
    src = sources(pcm, names)
    kinds = [False] + ([True] if headers is not None else [])
    for k in names:
        for ogg in kinds:
            kw = {"ogg_headers": headers} if ogg else {}
            f = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=ns, max_frames=piece, write_frames=1024, **kw)
            walls = []
            best = None
            for rep in range(a.reps + 1):
                dt = dev = tot = chk = 0.0
                nb = groups = 0
                for at in range(0, frames, piece):
                    n = min(piece, frames - at)
                    close = [at + piece >= frames] * ns
                    if k == "host":
                        slot, buf = f.buffer(2)
                        part = np.ascontiguousarray(pcm[:, at:at + piece]).reshape(-1)
                        buf[:part.size] = part
                        t0 = time.perf_counter()
                        f.wrote_live(slot, [n] * ns, close)
                    else:
                        slot, _ = f.buffer()
                        t, layout = src[k]
                        view = t[:, at:at + n] if layout == "sfc" else t[:, :, at:at + n]   # (a slice of the resident tensor: no copy)
                        t0 = time.perf_counter()
                        f.wrote_live_device(slot, view, close=close, layout=layout)
                        chk += (time.perf_counter() - t0) * 1e3
                    if ogg:
                        f.ogg(slot, copy=False)
                    r = f.packets(slot, copy=False)
                    dt += time.perf_counter() - t0
                    nb, dev, tot, groups = nb + r["nblocks"], dev + r["device_ms"], tot + r["total_ms"], groups + 1
                    f.release(slot)
                if rep:
                    walls.append(round(dt, 6))
                    if best is None or dt < best[0]:
                        best = (dt, nb, dev, tot, chk, groups)
            dt, nb, dev, tot, chk, groups = best
            line = {"case": "live %s %s" % (k, "ogg" if ogg else "packets"), "streams": ns, "seconds": a.seconds, "piece_s": a.piece, "groups": groups,
                    "blocks": nb, "blocks_per_s": nb / dt, "wall_s": dt, "wall_s_reps": walls, "total_ms": tot / groups, "device_ms": dev / groups}
            if k != "host":
                line["check_ms"] = chk / groups
            print(json.dumps(line), flush=True)
            f.close()
    torch.cuda.synchronize()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=64)
    ap.add_argument("--seconds", type=float, default=20.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--lanes", type=int, default=2)
    ap.add_argument("--piece", type=float, default=1.0, help="the live feed: seconds per piece")
    ap.add_argument("--only", choices=("host", "ingest"), default=None,
                    help="host: the host-fed whole-stream cases alone (calls an earlier library has too); ingest: packets only, one group per dtype (for a kernel trace)")
    a = ap.parse_args()
    import vorbis_amd
    pcm = stream_set(a.streams, int(44100 * a.seconds))
    blob = vorbis_amd.default_setup_blob("44k_stereo_q4")
    headers = None
    if a.only != "ingest":
        from tests import ref_host
        headers = ref_host.reference_headers(2, 44100, 0.4)  # (needs the reference build, oracle/_ref)
    if a.only == "host":
        return whole(a, vorbis_amd, blob, pcm, ["host"], "_s16", headers)
    everything = ["host", "dev_s16", "dev_f32", "dev_f16", "dev_bf16"]
    whole(a, vorbis_amd, blob, pcm, everything, "", headers)
    if a.only == "ingest":
        return
    from tests import bitrate_host
    whole(a, vorbis_amd, bitrate_host.managed_blob(2, (-1, 128000, -1)), pcm, ["host", "dev_f32"], " abr128", None)
    live(a, vorbis_amd, blob, pcm, ["host", "dev_f32"], headers)


if __name__ == "__main__":
    main()
