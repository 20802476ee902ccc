"""What the synthesis tests stand on.

* The reference side, through ctypes on the reference build (oracle/_ref/libvorbis_ref.so): the header packets of ANY
  RefEncoder (coupling switched off included), vb->pcm as vorbis_synthesis() leaves it for one packet, and mdct_backward.
* The shipped k_synth.h compiled for one lane on the host as a program of its own (tests/c/synth_host.cpp, built with
  -fsanitize=address,undefined), and the job files it reads.
* The signals: the block set and the gated-noise streams both the CPU and the GPU tests use."""
import ctypes as C
import os
import subprocess

import numpy as np

from tests.ogg_host import OggPacket, _reflib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RES_CLASS_STRIDE = 512
_f32p = C.POINTER(C.c_float)

# (channels, rate, quality, coupled): the setups of the block-level tests
SETUPS = {"44k_stereo_q4": (2, 44100, 0.4, True), "44k_stereo_q9": (2, 44100, 0.9, True), "44k_stereo_q1": (2, 44100, 0.1, True),
          "44k_stereo_qm1": (2, 44100, -0.1, True), "44k_mono_q5": (1, 44100, 0.5, True), "44k_51_q3": (6, 44100, 0.3, True),
          "8k_mono_q3": (1, 8000, 0.3, True), "44k_stereo_q4_uncoupled": (2, 44100, 0.4, False)}
# the feed's: 44.1 kHz stereo q 0.4, mono q 0.5, 5.1 q 0.3, stereo q -0.1, 8 kHz mono
FEED_SETUPS = ("44k_stereo_q4", "44k_mono_q5", "44k_51_q3", "44k_stereo_qm1", "8k_mono_q3")
SHORT_LENGTHS = (1, 20, 33, 1023, 2048, 2049, 3073, 7777)  # tests/test_feed.py::test_short_streams


def encoder(name):
    from oracle import ref
    ch, rate, q, coupled = SETUPS[name]
    return ref.RefEncoder(ch, rate, q, coupled=coupled)


# ---- the reference build ----
_VD_OFFSET = 56  # sizeof(vorbis_info), include/vorbis/codec.h:28-52: ref_enc (oracle/ref_harness.c) keeps its vorbis_dsp_state behind it


def encoder_headers(enc):
    """[identification, comment, setup] of vorbis_analysis_headerout() on a RefEncoder's own state"""
    L = _reflib()
    vc = C.create_string_buffer(4096)
    L.vorbis_comment_init(vc)
    ops = (OggPacket * 3)()
    L.vorbis_analysis_headerout.argtypes = [C.c_void_p] * 5
    assert L.vorbis_analysis_headerout(C.c_void_p(enc.h + _VD_OFFSET), vc, C.byref(ops[0]), C.byref(ops[1]), C.byref(ops[2])) == 0
    out = [C.string_at(o.packet, o.bytes) for o in ops]
    L.vorbis_comment_clear(vc)
    # (the identification header, Vorbis I 4.2.2, names the encoder it came from: a drift of ref_enc's layout would not)
    assert out[0][:7] == b"\x01vorbis" and out[0][11] == enc.channels and int.from_bytes(out[0][12:16], "little") == enc.rate
    return out


class BlockDecoder:
    """vorbis_synthesis_headerin x 3, vorbis_synthesis_init, vorbis_block_init; then vb->pcm per packet"""

    def __init__(self, headers):
        self.L = L = _reflib()
        self.vi, self.vc, self.vd, self.vb = (C.create_string_buffer(4096) for _ in range(4))
        L.vorbis_info_init(self.vi)
        L.vorbis_comment_init(self.vc)
        L.vorbis_synthesis_headerin.argtypes = [C.c_void_p] * 3
        self.keep = []
        for i in range(3):
            o = self._op(i, headers[i])
            r = L.vorbis_synthesis_headerin(self.vi, self.vc, C.byref(o))
            assert r == 0, "vorbis_synthesis_headerin(%d) = %d" % (i, r)
        L.vorbis_synthesis_init.argtypes = [C.c_void_p] * 2
        L.vorbis_block_init.argtypes = [C.c_void_p] * 2
        L.vorbis_synthesis.argtypes = [C.c_void_p] * 2
        L.vorbis_block_clear.argtypes = [C.c_void_p]
        L.vorbis_info_blocksize.argtypes = [C.c_void_p, C.c_int]
        assert L.vorbis_synthesis_init(self.vd, self.vi) == 0
        L.vorbis_block_init(self.vd, self.vb)
        self.channels = C.cast(self.vi, C.POINTER(C.c_int))[1]
        self.bs = (L.vorbis_info_blocksize(self.vi, 0), L.vorbis_info_blocksize(self.vi, 1))
        self.n = 3

    def _op(self, i, p):
        b = C.create_string_buffer(bytes(p), len(p))
        self.keep = self.keep[-8:] + [b]
        return OggPacket(C.cast(b, C.c_void_p), len(p), 1 if i == 0 else 0, 0, -1 if i >= 3 else 0, i)

    def block(self, packet, W):
        """vb->pcm, the first field of vorbis_block (include/vorbis/codec.h:87-89), as [ch][blocksizes[W]]"""
        o = self._op(self.n, packet)
        self.n += 1
        assert self.L.vorbis_synthesis(self.vb, C.byref(o)) == 0
        pcm = C.cast(self.vb, C.POINTER(C.POINTER(_f32p)))[0]
        return np.stack([np.ctypeslib.as_array(pcm[c], (self.bs[W],)).copy() for c in range(self.channels)])

    def synthesis(self, packet):
        """(vorbis_synthesis()'s return value, vb->pcm) for ANY packet: the block's size is the one the packet's own head
        names (two block sizes are two modes: bit 1 of the first byte); None for vb->pcm where the return value is nonzero"""
        o = self._op(self.n, packet)
        self.n += 1
        r = self.L.vorbis_synthesis(self.vb, C.byref(o))
        if r:
            return r, None
        W = (packet[0] >> 1) & 1 if self.bs[0] != self.bs[1] else 0
        pcm = C.cast(self.vb, C.POINTER(C.POINTER(_f32p)))[0]
        return 0, np.stack([np.ctypeslib.as_array(pcm[c], (self.bs[W],)).copy() for c in range(self.channels)])

    def close(self):
        self.L.vorbis_block_clear(self.vb)
        self.L.vorbis_dsp_clear(self.vd)
        self.L.vorbis_comment_clear(self.vc)
        self.L.vorbis_info_clear(self.vi)


class _MdctLookup(C.Structure):  # mdct_lookup, lib/mdct.h:55-63
    _fields_ = [("n", C.c_int), ("log2n", C.c_int), ("trig", _f32p), ("bitrev", C.POINTER(C.c_int)), ("scale", C.c_float)]


def reference_mdct_backward(n, spectrum):
    """-> (the reference's mdct_backward of spectrum [n/2] as float32 [n], its trig table [n + n/4])"""
    L = _reflib()
    look = _MdctLookup()
    L.mdct_init.argtypes = [C.POINTER(_MdctLookup), C.c_int]
    L.mdct_backward.argtypes = [C.POINTER(_MdctLookup), _f32p, _f32p]
    L.mdct_clear.argtypes = [C.POINTER(_MdctLookup)]
    L.mdct_init(C.byref(look), n)
    trig = np.ctypeslib.as_array(look.trig, (n + n // 4,)).copy()
    buf = np.zeros(n, np.float32)  # in place, as mapping0_inverse calls it
    buf[:n // 2] = spectrum
    L.mdct_backward(C.byref(look), buf.ctypes.data_as(_f32p), buf.ctypes.data_as(_f32p))
    L.mdct_clear(C.byref(look))
    return buf, trig


# ---- the shipped bodies on the host ----
def build(outdir):
    exe = os.path.join(str(outdir), "synth_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-ffp-contract=off", "-fno-fast-math", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"),
                           "-I" + os.path.join(ROOT, "vorbis_amd", "csrc"), "-I" + os.path.join(ROOT, "tests", "emul"),
                           os.path.join(ROOT, "tests", "c", "synth_host.cpp"), "-o", exe])
    return exe


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


def gated_noise(ch, rate, frames, seed):
    """bursts, so that the detector switches (tests/test_rates.py::test_hybrid_encode)"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames)
    x = (rng.random((ch, frames), dtype=np.float32) - 0.5) * 2 * np.where((t % (rate // 4)) < rate // 40, 0.5, 0.0005)
    return np.ascontiguousarray(x, dtype=np.float32)


def lap_cases(blocks):
    """the (lW, W) pairs a stream's consecutive blocks form"""
    return {(a, b) for a, b in zip([W for W in blocks][:-1], [W for W in blocks][1:])}
