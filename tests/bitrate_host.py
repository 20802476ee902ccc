"""The bitrate manager's walk (vorbis_amd/csrc/k_bitrate.h) compiled with the host compiler, for the tests: the shipped
header itself, not a sibling of it, built -ffp-contract=off as the library is.  Also the blob's manager section as a
ctypes struct, and the packet the manager hands out rebuilt from a candidate."""
import ctypes as C
import os

import numpy as np

from tests import hostbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PACKETBLOBS = 15
OFF_BITRATE = 44  # vamd_setup_header.off_bitrate (include/vamd_setup.h)
MANAGED = 32      # vamd_setup_header.managed

# BR_* of k_bitrate.h
SLEW_CLAMPED, MIN_FORCED, MAX_FORCED, BELOW_ZERO, TRUNCATED, PADDED = 1, 2, 4, 8, 16, 32

_SHIM = r"""
#include "k_bitrate.h"
extern "C" void walk_init(const vamd_bitrate_tab *t, vamd_bitrate_state *st) { vamd::bitrate_state_init(*t, *st); }
// blocks of ONE stream in stream order: bytes [nb][15], W [nb]
extern "C" void walk(const vamd_bitrate_tab *t, vamd_bitrate_state *st, int samples0, int samples1, long nb,
                     const int32_t *bytes, const int32_t *W, int32_t *choice, int64_t *final_bytes, int32_t *flags) {
  for (long k = 0; k < nb; k++) {
    int fl = 0;
    choice[k] = vamd::bitrate_addblock(*t, *st, bytes + k * VAMD_PACKETBLOBS, W[k], W[k] ? samples1 : samples0,
                                       final_bytes + k, &fl);
    flags[k] = fl;
  }
}
extern "C" long long final_bits(int32_t bits, long long final_bytes) { return vamd::bitrate_final_bits(bits, final_bytes); }
"""


class BitrateTab(C.Structure):  # vamd_bitrate_tab
    _fields_ = [(k, C.c_int64) for k in ("short_per_long", "avg_bitsper", "min_bitsper", "max_bitsper", "minmax_reservoir",
                                         "avg_reservoir", "reservoir_bits", "rate")] + \
               [(k, C.c_double) for k in ("avgfloat", "reservoir_bias", "slew_damp")] + [("pad", C.c_int64)]


class BitrateState(C.Structure):  # vamd_bitrate_state
    _fields_ = [("avgfloat", C.c_double), ("minmax_reservoir", C.c_int64), ("avg_reservoir", C.c_int64), ("pad", C.c_int64)]


def section_offset(blob):
    return int(np.frombuffer(bytes(blob[OFF_BITRATE:OFF_BITRATE + 4]), np.uint32)[0])


def tab_from_blob(blob):
    blob = bytes(np.ascontiguousarray(blob, dtype=np.uint8))
    off = section_offset(blob)
    assert off, "the blob carries no bitrate manager section"
    return BitrateTab.from_buffer_copy(blob[off:off + C.sizeof(BitrateTab)])


SECTIONS = os.path.join(ROOT, "tests", "golden", "bitrate_sections.json")


def recorded_section(ch, rate, rates):
    """The manager's section vamd_pack_setup writes for vorbis_encode_init(ch, rate, *rates), as recorded in
    tests/golden/bitrate_sections.json."""
    import json
    key = "%d/%d/%d/%d/%d" % ((ch, rate) + tuple(int(v) for v in rates))
    with open(SECTIONS) as f:
        rec = json.load(f)["sections"][key]
    t = BitrateTab()
    for k, v in rec.items():
        setattr(t, k, v)
    return t


def graft_section(blob, t):
    """`blob` (a managed setup without the section) with the section `t` appended where vamd_pack_setup puts it: behind
    the codebooks at the next 16-byte boundary, which is the section-less blob's own total_bytes."""
    blob = np.ascontiguousarray(blob, dtype=np.uint8)
    total = int(np.frombuffer(bytes(blob[12:16]), np.uint32)[0])
    assert total == blob.size and total % 16 == 0 and not section_offset(blob)
    t = bytes(t)
    out = np.zeros(total + (len(t) + 15) // 16 * 16, np.uint8)
    out[:total] = blob
    out[total:total + len(t)] = np.frombuffer(t, np.uint8)
    out[OFF_BITRATE:OFF_BITRATE + 4] = np.frombuffer(np.uint32(total).tobytes(), np.uint8)
    out[12:16] = np.frombuffer(np.uint32(out.size).tobytes(), np.uint8)
    return out


def managed_blob(ch, rates, rate=44100):
    """A managed encoder's setup blob with the bitrate manager's section.  The reference encoder packs it
    (oracle.ref.RefEncoder.pack_setup, integration/vamd_pack_setup.c).  Where the oracle library was built from an
    earlier packer, which leaves the section out, the recorded section is grafted on: byte for byte what the current
    packer writes (test_bitrate_walk.py holds the two together wherever the oracle is current)."""
    from oracle import ref
    blob = ref.RefEncoder(ch, rate, managed=rates).pack_setup()
    if section_offset(blob):
        return blob
    return graft_section(blob, recorded_section(ch, rate, rates))


def blocksizes(blob):
    return [int(x) for x in np.frombuffer(bytes(blob[24:32]), np.int32)]


def build():
    return hostbuild.shim("walk", _SHIM)


class HostWalk:
    """The shipped walk on the host: one stream's blocks at a time, its state kept here."""

    def __init__(self, lib, blob):
        self.L = C.CDLL(lib)
        self.L.final_bits.restype = C.c_longlong
        self.L.final_bits.argtypes = [C.c_int32, C.c_longlong]
        self.tab = tab_from_blob(blob)
        bs = blocksizes(blob)
        self.samples = (bs[0] >> 1, bs[1] >> 1)

    def new_state(self):
        st = BitrateState()
        self.L.walk_init(C.byref(self.tab), C.byref(st))
        return st

    def walk(self, st, sizes, W):
        """sizes [nb][15] candidate bytes, W [nb] -> (choice, final_bytes, flags); st is advanced."""
        sizes = np.ascontiguousarray(sizes, dtype=np.int32).reshape(-1, PACKETBLOBS)
        W = np.ascontiguousarray(W, dtype=np.int32)
        nb = sizes.shape[0]
        choice, fin, flags = np.zeros(nb, np.int32), np.zeros(nb, np.int64), np.zeros(nb, np.int32)
        self.L.walk(C.byref(self.tab), C.byref(st), self.samples[0], self.samples[1], C.c_long(nb),
                    sizes.ctypes.data_as(C.c_void_p), W.ctypes.data_as(C.c_void_p), choice.ctypes.data_as(C.c_void_p),
                    fin.ctypes.data_as(C.c_void_p), flags.ctypes.data_as(C.c_void_p))
        return choice, fin, flags

    def final_bits(self, bits, final_bytes):
        return int(self.L.final_bits(int(bits), int(final_bytes)))


def handed_out(candidate, final_bytes):
    """The packet vorbis_bitrate_flushpacket hands out: the candidate cut to final_bytes, or zero-padded up to it."""
    if final_bytes <= len(candidate):
        return candidate[:final_bytes]
    return candidate + bytes(final_bytes - len(candidate))


# (max, nominal, min) and a signal kind per config: what the manager meets in practice and the corners that make every
# branch of vorbis_bitrate_addblock fire
CONFIGS = [
    ("abr128_stereo", 2, (-1, 128000, -1), "music"),
    ("abr64_mono", 1, (-1, 64000, -1), "music"),
    ("cbr128_stereo", 2, (128000, 128000, 128000), "music"),
    ("minmax_stereo", 2, (160000, 96000, 64000), "music"),
    ("tight_max_noise", 2, (128000, 128000, 128000), "noise"),
    ("high_min_quiet", 2, (-1, -1, 160000), "quiet"),
]


def signal(kind, ch, frames, seed):
    """planar float32 [ch][frames]"""
    rng = np.random.default_rng(seed)
    t = np.arange(frames) / 44100.0
    if kind == "noise":
        # spiky spectra: every 256 samples a fresh random magnitude per bin (15 dB spread), random phases -- far more
        # bits than the setup's nominal rate
        n, nf = 256, frames // 256 + 1
        x = np.stack([np.fft.irfft(10 ** rng.uniform(-1.5, 0, (nf, n // 2 + 1)) * np.exp(2j * np.pi * rng.random((nf, n // 2 + 1))),
                                   n=n, axis=1).reshape(-1)[:frames] for _ in range(ch)])
        x *= 0.9 / np.abs(x).max()
    elif kind == "quiet":
        x = (rng.random((ch, frames)) - 0.5) * 2e-5
    else:
        # tones over noise whose loudness swings every ~0.4 s: the floater has to move, and is slew-limited when it does
        env = 0.05 + 0.45 * (np.sin(2 * np.pi * 1.3 * t) > 0)
        x = np.stack([env * (0.5 * np.sin(2 * np.pi * (220 + 110 * c) * t) + 0.3 * np.sin(2 * np.pi * 3520 * t * (1 + 0.1 * c)))
                      + (rng.random(frames) - 0.5) * 0.4 * env for c in range(ch)])
        x[:, int(frames * 0.6):int(frames * 0.62)] *= 0.001
    return np.ascontiguousarray(x, dtype=np.float32)
