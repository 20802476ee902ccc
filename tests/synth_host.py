"""What the synthesis tests stand on, beside the reference side (tests/ref_host.py).

* The shipped k_synth.h compiled for one lane on the host as a program of its own (tests/c/synth_host.cpp, built with
  -fsanitize=address,undefined), and the job files it reads.
* The block set both the CPU and the GPU tests use, and the one-lane emulation's rows of a block."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests import checker, hostbuild

RES_CLASS_STRIDE = 512
_f32p = C.POINTER(C.c_float)

SETUPS = checker.ENCODERS  # (channels, rate, quality, coupled): the setups of the block-level tests
# the feed's: 44.1 kHz stereo q 0.4, mono q 0.5, 5.1 q 0.3, stereo q -0.1, 8 kHz mono
FEED_SETUPS = ("44k_stereo_q4", "44k_mono_q5", "44k_51_q3", "44k_stereo_qm1", "8k_mono_q3")
SHORT_LENGTHS = (1, 20, 33, 1023, 2048, 2049, 3073, 7777)  # tests/test_feed.py::test_short_streams


# ---- the shipped bodies on the host ----
def build():
    return hostbuild.program("synth_host.cpp")


def _run(exe, args, out, count):
    r = subprocess.run([exe] + args + [out], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-2000:] + r.stderr[-4000:])
    got = np.fromfile(out, np.float32)
    assert got.size == count, (got.size, count)
    return got


def host_mdct_backward(exe, tmp, n, trig, spectrum):
    job = os.path.join(str(tmp), "mdct.job")
    with open(job, "wb") as f:
        f.write(np.int32(n).tobytes() + np.ascontiguousarray(trig, np.float32).tobytes() + np.ascontiguousarray(spectrum, np.float32).tobytes())
    return _run(exe, ["mdct", job], os.path.join(str(tmp), "mdct.out"), n)


def emul_block(em, pcm, W, lW=None, nW=None, blocktype=None):
    """The one-lane emulation's outputs of a block in the layout the batch holds them in (rows per submap, not trimmed)"""
    from tests.emul.emul import _Taps, _i32p
    lW, nW = W if lW is None else lW, W if nW is None else nW
    blocktype = (1 if W else 0) if blocktype is None else blocktype
    ch, n2 = em.channels, em.bs[W] // 2
    pcm = np.ascontiguousarray(pcm, np.float32)
    S, cap = em.L.emul_submaps(em.h, W), em.L.emul_residue_capacity(em.h, W)
    assert cap > 0
    o = dict(W=W, post_valid=np.zeros(ch, np.int32), ilogmask=np.zeros((ch, n2), np.int32), res_class=np.zeros(S * RES_CLASS_STRIDE, np.int32),
             res_count=np.zeros(2 * S, np.int32), res_entries=np.zeros((cap + 1) & ~1, np.uint16))
    pk, pbits = np.zeros(em.L.emul_packet_capacity(em.h, W), np.uint8), np.zeros(1, np.int32)
    t = _Taps()
    for k in ("post_valid", "ilogmask", "res_class", "res_count"):
        setattr(t, k, o[k].ctypes.data_as(_i32p))
    t.res_entries = o["res_entries"].ctypes.data_as(C.POINTER(C.c_ushort))
    t.packet, t.packet_bits = pk.ctypes.data, pbits.ctypes.data_as(_i32p)
    assert em.L.emul_analyze_block(em.h, pcm.ctypes.data_as(_f32p), lW, W, nW, blocktype, C.c_float(-9999.0), C.byref(t)) == 0
    assert pbits[0] >= 0
    o["packet"] = pk[:(int(pbits[0]) + 7) // 8].tobytes()
    return o


def host_synth_blocks(exe, tmp, blob, blocks, bs, ch):
    """synth_block over emul_block()'s outputs -> a list of [ch][n]"""
    setup, job = os.path.join(str(tmp), "setup.bin"), os.path.join(str(tmp), "block.job")
    np.ascontiguousarray(blob, np.uint8).tofile(setup)
    with open(job, "wb") as f:
        f.write(np.int32(len(blocks)).tobytes())
        for b in blocks:
            f.write(np.int32(b["W"]).tobytes())
            for k in ("post_valid", "ilogmask", "res_class", "res_count", "res_entries"):
                f.write(b[k].tobytes())
    got = _run(exe, ["block", setup, job], os.path.join(str(tmp), "block.out"), sum(ch * bs[b["W"]] for b in blocks))
    out, at = [], 0
    for b in blocks:
        n = bs[b["W"]]
        out.append(got[at:at + ch * n].reshape(ch, n))
        at += ch * n
    return out


def host_lap(exe, tmp, bs, win, blocks, frames):
    """lap_find / lap_sample over one stream's blocks [(W, pcm [ch][n])] -> [ch][frames]"""
    ch = blocks[0][1].shape[0]
    job = os.path.join(str(tmp), "lap.job")
    with open(job, "wb") as f:
        f.write(np.array([ch, bs[0], bs[1], len(blocks), frames], np.int32).tobytes())
        f.write(np.ascontiguousarray(win[0], np.float32).tobytes() + np.ascontiguousarray(win[1], np.float32).tobytes())
        for W, pcm in blocks:
            assert pcm.shape == (ch, bs[W])
            f.write(np.int32(W).tobytes() + np.ascontiguousarray(pcm, np.float32).tobytes())
    return _run(exe, ["lap", job], os.path.join(str(tmp), "lap.out"), ch * frames).reshape(ch, frames)


def windows(blob, bs):
    """the rising half windows the setup blob stages (vamd_xform_tab::off_window), short and long"""
    blob = np.ascontiguousarray(blob, np.uint8)
    out = []
    for W in (0, 1):  # vamd_setup_header: 48 bytes, then xform[2] of 108 bytes each with off_window 92 bytes in (include/vamd_setup.h)
        n, off = np.frombuffer(blob[48 + 108 * W:52 + 108 * W].tobytes(), np.int32)[0], np.frombuffer(blob[140 + 108 * W:144 + 108 * W].tobytes(), np.uint32)[0]
        assert n == bs[W]
        out.append(np.frombuffer(blob[int(off):int(off) + 2 * n].tobytes(), np.float32))
    return out


# ---- signals ----
BLOCK_KINDS = ("noise_half", "noise_quiet", "noise_full", "silence", "one_silent", "tone")


def block_set(ch, n, seed):
    """noise at 0.5 and 0.01, full-scale noise (the top residue class's books clip), digital silence, silence in one
    channel only (coupling dirties nonzero), a tone"""
    rng = np.random.default_rng(seed)
    def noise(a):
        return ((rng.random((ch, n), dtype=np.float32) - 0.5) * 2 * a).astype(np.float32)
    one = noise(0.5)
    one[ch - 1] = 0
    tone = np.tile((0.6 * np.sin(2 * np.pi * 0.0371 * np.arange(n))).astype(np.float32), (ch, 1))
    tone[0] *= 0.5
    return dict(zip(BLOCK_KINDS, (noise(0.5), noise(0.01), noise(1.0), np.zeros((ch, n), np.float32), one, tone)))


def lap_cases(blocks):
    """the (lW, W) pairs a stream's consecutive blocks form"""
    return {(a, b) for a, b in zip([W for W in blocks][:-1], [W for W in blocks][1:])}
