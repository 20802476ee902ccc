"""The Ogg decode entry's host half on the host: the shipped scan (vorbis_amd/csrc/vamd_demux.h), the block plan over its
packet table and k_ogg_depage's body (k_demux.h) with the lanes in turn, as a program of its own -- tests/c/demux_host.cpp,
built with -fsanitize=address,undefined -- the job file it reads and the result it writes."""
import os
import subprocess

import numpy as np

from tests import hostbuild


def build():
    return hostbuild.program("demux_host.cpp")


def _padded(b):
    return bytes(b) + b"\0" * (-len(b) & 3)


def host_scan(exe, tmp, blob, files, setup_header=None):
    """files: one `bytes` per stream -> per stream dict(status, end, frames, packets): the scan's status or-ed with its
    pages' and the plan's, the end granule, the frames the plan gives the stream, and its audio packets as the depage
    left them in the packed arena, cut by the scan's packet table"""
    setup, job, out = (os.path.join(str(tmp), n) for n in ("setup.bin", "demux.job", "demux.out"))
    np.ascontiguousarray(blob, np.uint8).tofile(setup)
    hdr = bytes(setup_header) if setup_header is not None else b""
    with open(job, "wb") as f:
        f.write(np.array([len(files), len(hdr)], np.int32).tobytes() + _padded(hdr))
        for x in files:
            f.write(np.int64(len(x)).tobytes() + _padded(x))
    r = subprocess.run([exe, "scan", setup, job, out], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    raw, at, res = open(out, "rb").read(), 0, []
    for _ in files:
        status, end, frames, n = np.frombuffer(raw, np.int32, 1, at)[0], np.frombuffer(raw, np.int64, 1, at + 4)[0], \
            np.frombuffer(raw, np.int32, 1, at + 12)[0], int(np.frombuffer(raw, np.int32, 1, at + 16)[0])
        sizes = np.frombuffer(raw, np.int32, n, at + 20)
        at += 20 + 4 * n
        packets = []
        for v in sizes:
            packets.append(raw[at:at + int(v)])
            at += int(v)
        at += -int(sizes.sum()) & 3
        res.append(dict(status=int(status), end=int(end), frames=int(frames), packets=packets))
    assert at == len(raw)
    return res
