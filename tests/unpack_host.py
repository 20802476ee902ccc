"""The packet decoder's front half on the host: vorbis_amd/csrc/k_unpack.h compiled for one lane with the shipped planning
(vamd_decode_plan.h) and back half (k_synth.h) as a program of its own -- tests/c/unpack_host.cpp, built with
-fsanitize=address,undefined -- the job files it reads and the results it writes."""
import os
import subprocess

import numpy as np

from tests import hostbuild
from tests.synth_host import RES_CLASS_STRIDE

STATUS_NOTAUDIO, STATUS_BADCODE, STATUS_TRUNCATED = 4, 8, 16  # include/vorbis_amd.h


def build():
    return hostbuild.program("unpack_host.cpp")


def _run(exe, args):
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    return r.stdout


def _setup_file(tmp, blob):
    path = os.path.join(str(tmp), "setup.bin")
    np.ascontiguousarray(blob, np.uint8).tofile(path)
    return path


def _packet(p):
    return np.int32(len(p)).tobytes() + bytes(p) + b"\0" * (-len(p) & 3)


def info(exe, tmp, blob):
    """per size class: dict(submaps, cap, sub [ch], look_n [submaps], ent_base [submaps])"""
    out = {}
    for line in _run(exe, ["info", _setup_file(tmp, blob)]).splitlines():
        a, b, c = (list(map(int, part.split())) for part in line.split("|"))
        out[a[0]] = dict(submaps=a[1], cap=a[2], sub=b, look_n=c[0::2], ent_base=c[1::2])
    return out


def host_unpack_blocks(exe, tmp, blob, blocks, bs, ch):
    """blocks [(W, packet)] -> per block dict(status, post_valid, ilogmask [ch][n2], res_class, res_count, res_entries,
    pcm [ch][n]): unpack_packet's rows, and synth_block over them"""
    geo = info(exe, tmp, blob)
    job, out = os.path.join(str(tmp), "unpack.job"), os.path.join(str(tmp), "unpack.out")
    with open(job, "wb") as f:
        f.write(np.int32(len(blocks)).tobytes())
        for W, p in blocks:
            f.write(np.int32(W).tobytes() + _packet(p))
    _run(exe, ["blocks", _setup_file(tmp, blob), job, out])
    raw, at, res = np.fromfile(out, np.int32), 0, []

    def take(count):
        nonlocal at
        at += count
        assert at <= raw.size
        return raw[at - count:at]
    for W, _ in blocks:
        n, S, cap = bs[W], geo[W]["submaps"], geo[W]["cap"]
        res.append(dict(status=int(take(1)[0]), post_valid=take(ch), ilogmask=take(ch * (n // 2)).reshape(ch, n // 2),
                        res_class=take(S * RES_CLASS_STRIDE), res_count=take(2 * S), res_entries=take(cap),
                        pcm=take(ch * n).view(np.float32).reshape(ch, n)))
    assert at == raw.size
    return res, geo


def _streams_job(tmp, streams, granules):
    job = os.path.join(str(tmp), "streams.job")
    with open(job, "wb") as f:
        f.write(np.int32(len(streams)).tobytes())
        for packets, g in zip(streams, granules):
            f.write(np.int32(len(packets)).tobytes() + np.int64(g).tobytes())
            for p in packets:
                f.write(_packet(p))
    return job


def host_decode_streams(exe, tmp, blob, streams, granules, ch):
    """streams: lists of packets; granules: per stream the last packet's granule position (-1: none)
    -> [(status, pcm [ch][frames])]: plan, unpack, synth, lap"""
    out = os.path.join(str(tmp), "streams.out")
    _run(exe, ["streams", _setup_file(tmp, blob), _streams_job(tmp, streams, granules), out])
    raw, at, res = np.fromfile(out, np.int32), 0, []
    for _ in streams:
        status, frames = int(raw[at]), int(raw[at + 1])
        res.append((status, raw[at + 2:at + 2 + ch * frames].view(np.float32).reshape(ch, frames)))
        at += 2 + ch * frames
    assert at == raw.size
    return res


def host_fuzz(exe, tmp, blob, packets):
    """-> the program's summary line; it fails the test itself where a case does"""
    return _run(exe, ["fuzz", _setup_file(tmp, blob), _streams_job(tmp, [packets], [-1])])
