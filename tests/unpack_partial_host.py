"""The packet decoder under the keep policy (vamd_decode_partial) on the host: k_unpack.h's second instantiation of the
walk and k_synth.h's bounded residue add compiled for one lane with the shipped planning as a program of its own --
tests/c/unpack_partial_host.cpp, built with -fsanitize=address,undefined -- the job files it reads and the results it
writes.  With keep = 0 the same program runs the default pair."""
import os
import subprocess

import numpy as np

from tests import hostbuild

STATUS_NOTAUDIO, STATUS_BADCODE, STATUS_TRUNCATED, STATUS_PARTIAL = 4, 8, 16, 128  # include/vorbis_amd.h
# where the reader first failed (k_unpack.h, UNPACK_AT_*)
AT_FLAG, AT_POST, AT_FLOORBOOK, AT_PHRASE, AT_CLASSES, AT_ENTRY = 1, 2, 3, 4, 5, 6


def build():
    return hostbuild.program("unpack_partial_host.cpp")


def _run(exe, args):
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    return r.stdout


def _file(tmp, name, data):
    path = os.path.join(str(tmp), name)
    np.frombuffer(bytes(data), np.uint8).tofile(path)
    return path


def setup_args(tmp, blob=None, headers=None):
    """the program's SETUP words: a setup blob, or a stream's [identification, comment, setup] headers"""
    if headers is not None:
        return ["headers", _file(tmp, "id.bin", headers[0]), _file(tmp, "setup_header.bin", headers[2])]
    return ["blob", _file(tmp, "setup.bin", np.ascontiguousarray(blob, np.uint8).tobytes())]


def _packet(p):
    return np.int32(len(p)).tobytes() + bytes(p) + b"\0" * (-len(p) & 3)


def host_blocks(exe, tmp, setup, packets, bs, ch, keep=1):
    """packets -> per packet dict(status, W, place, index, stage, res_count [4], pcm [ch][n] or None): the walk's status,
    where its reader first failed, and vb->pcm where the packet is kept"""
    job, out = os.path.join(str(tmp), "partial.job"), os.path.join(str(tmp), "partial.out")
    with open(job, "wb") as f:
        f.write(np.int32(keep).tobytes() + np.int32(len(packets)).tobytes())
        for p in packets:
            f.write(_packet(p))
    _run(exe, ["blocks"] + setup + [job, out])
    raw, at, res = np.fromfile(out, np.int32), 0, []
    for _ in packets:
        rec = raw[at:at + 12]
        at += 12
        W, pcm = int(rec[1]), None
        if rec[9]:
            pcm = raw[at:at + ch * bs[W]].view(np.float32).reshape(ch, bs[W])
            at += ch * bs[W]
        res.append(dict(status=int(rec[0]), W=W, place=int(rec[2]), index=int(rec[3]), stage=int(rec[4]), res_count=[int(v) for v in rec[5:9]], pcm=pcm))
    assert at == raw.size
    return res


def host_entry_ends(exe, tmp, setup, packets):
    """packets -> per packet [per submap (two) the bits of the packet behind which the reader stood when it had read each
    entry]: the count of entries a cut of n bytes can have read is the number of those at or below 8 n"""
    job, out = os.path.join(str(tmp), "ends.job"), os.path.join(str(tmp), "ends.out")
    with open(job, "wb") as f:
        f.write(np.int32(1).tobytes() + np.int32(len(packets)).tobytes())
        for p in packets:
            f.write(_packet(p))
    _run(exe, ["ends"] + setup + [job, out])
    raw, at, res = np.fromfile(out, np.int32), 0, []
    for _ in packets:
        row = []
        for _ in range(2):
            n = int(raw[at])
            row.append(raw[at + 1:at + 1 + n])
            at += 1 + n
        res.append(row)
    assert at == raw.size
    return res


def host_streams(exe, tmp, setup, streams, granules, ch, keep=1):
    """streams: lists of packets; granules: per stream the last packet's granule position (-1: none)
    -> [(status, pcm [ch][frames])]: plan, unpack, synth, lap under the policy"""
    job, out = os.path.join(str(tmp), "partial_streams.job"), os.path.join(str(tmp), "partial_streams.out")
    with open(job, "wb") as f:
        f.write(np.int32(keep).tobytes() + np.int32(len(streams)).tobytes())
        for packets, g in zip(streams, granules):
            f.write(np.int32(len(packets)).tobytes() + np.int64(g).tobytes())
            for p in packets:
                f.write(_packet(p))
    _run(exe, ["streams"] + setup + [job, out])
    raw, at, res = np.fromfile(out, np.int32), 0, []
    for _ in streams:
        status, frames = int(raw[at]), int(raw[at + 1])
        res.append((status, raw[at + 2:at + 2 + ch * frames].view(np.float32).reshape(ch, frames)))
        at += 2 + ch * frames
    assert at == raw.size
    return res
