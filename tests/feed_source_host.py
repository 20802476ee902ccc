"""What the device-fed feed's tests stand on.

* The shipped vorbis_amd/csrc/k_feed_src.h compiled with the host compiler -- the header itself, not a sibling of it: the
  conversion of a source element to float, the ingest body of a whole-stream group (a thread's share, run here item by item
  over a host buffer, through the vector-load path or through element loads alone), and the host's range check.
* The grid of source layouts both suites walk: where the streams of a group lie in one flat buffer, with which strides."""
import ctypes as C

import numpy as np

from tests import hostbuild


SRC_S16, SRC_F32, SRC_F16, SRC_BF16 = 0, 1, 2, 3
ELEM_BYTES = {SRC_S16: 2, SRC_F32: 4, SRC_F16: 2, SRC_BF16: 2}
AMP_FLOOR = -9999.0

_SHIM = r"""
#include "k_feed_src.h"
using namespace vamd;
extern "C" void convert16(int dtype, const uint16_t *in, long long n, float *out) {
  for (long long i = 0; i < n; i++)
    out[i] = dtype == SRC_S16 ? src_float((int16_t)in[i]) : dtype == SRC_F16 ? src_float(src_f16{in[i]}) : src_float(src_bf16{in[i]});
}
extern "C" int non_finite(float x) { return src_non_finite(x); }
template <typename T>
static void ingest_as(long nstreams, int ch, long frames, int head, int pad, float *pcm, long ss, long cs, float *amp, const long long *frames_of,
                      const long long *base_of, int64_t cstride, int64_t fstride, int vec_ok) {
  const long per = (head >> 2) + ((frames + 3) >> 2) + (pad >> 2);
  for (long t = 0; t < nstreams * per; t++)
    feed_ingest_dev_item<T>(t, ch, frames, head, pad, pcm, ss, cs, amp, -9999.0f, frames_of, base_of, cstride, fstride, vec_ok != 0);
}
// the whole-stream ingest of a device-fed group, every item in turn
extern "C" void ingest(int dtype, long nstreams, int ch, long frames, int head, int pad, float *pcm, long ss, long cs, float *amp,
                       const long long *frames_of, const long long *base_of, long long cstride, long long fstride, int vec_ok) {
  if (dtype == SRC_S16) ingest_as<int16_t>(nstreams, ch, frames, head, pad, pcm, ss, cs, amp, frames_of, base_of, cstride, fstride, vec_ok);
  else if (dtype == SRC_F32) ingest_as<float>(nstreams, ch, frames, head, pad, pcm, ss, cs, amp, frames_of, base_of, cstride, fstride, vec_ok);
  else if (dtype == SRC_F16) ingest_as<src_f16>(nstreams, ch, frames, head, pad, pcm, ss, cs, amp, frames_of, base_of, cstride, fstride, vec_ok);
  else ingest_as<src_bf16>(nstreams, ch, frames, head, pad, pcm, ss, cs, amp, frames_of, base_of, cstride, fstride, vec_ok);
}
extern "C" int extent(int ch, long long frames, long long cstride, long long fstride, int elem_bytes, long long offset, long long alloc_bytes,
                      long long *lo, long long *hi) {
  int64_t l = 0, h = 0;
  const int r = source_extent(ch, frames, cstride, fstride, elem_bytes, offset, alloc_bytes, &l, &h);
  *lo = l, *hi = h;
  return r;
}
"""


def build():
    return hostbuild.shim("feed_source", _SHIM)


def aligned(n, dtype, align=64, offset=0):
    """an array of n elements whose first element lies `offset` bytes behind a multiple of `align`"""
    raw = np.zeros(n * np.dtype(dtype).itemsize + align + offset, np.uint8)
    at = (-raw.ctypes.data) % align + offset
    return raw[at:at + n * np.dtype(dtype).itemsize].view(dtype)


class HostSource:
    def __init__(self, lib):
        self.L = C.CDLL(lib)
        self.L.convert16.argtypes = [C.c_int, C.c_void_p, C.c_longlong, C.c_void_p]
        self.L.convert16.restype = None
        self.L.non_finite.argtypes = [C.c_float]
        self.L.ingest.argtypes = [C.c_int, C.c_long, C.c_int, C.c_long, C.c_int, C.c_int, C.c_void_p, C.c_long, C.c_long, C.c_void_p, C.c_void_p,
                                  C.c_void_p, C.c_longlong, C.c_longlong, C.c_int]
        self.L.ingest.restype = None
        self.L.extent.argtypes = [C.c_int] + [C.c_longlong] * 3 + [C.c_int] + [C.c_longlong] * 2 + [C.c_void_p] * 2

    def convert16(self, dtype, bits):
        bits = np.ascontiguousarray(bits, dtype=np.uint16)
        out = np.zeros(bits.size, np.float32)
        self.L.convert16(dtype, bits.ctypes.data, bits.size, out.ctypes.data)
        return out

    def non_finite(self, x):
        return bool(self.L.non_finite(C.c_float(x)))

    def extent(self, ch, frames, cstride, fstride, elem_bytes, offset, alloc_bytes):
        """-> (code, lo, hi) of source_extent"""
        lo, hi = C.c_longlong(), C.c_longlong()
        r = self.L.extent(ch, frames, cstride, fstride, elem_bytes, offset, alloc_bytes, C.addressof(lo), C.addressof(hi))
        return r, lo.value, hi.value

    def ingest(self, dtype, buf, base_elems, frames_of, ch, cstride, fstride, head, pad, vec_ok, frames=None):
        """The ingest body over the host buffer `buf` (its element type: dtype's): stream s at element base_elems[s].
        -> (pcm [ns, ch, cs] float32 -- filled with a NaN pattern beforehand, so what is not written shows -- and amp [ns])"""
        ns = len(base_elems)
        frames = int(max(frames_of)) if frames is None else frames
        cs = (head + ((frames + 3) & ~3) + pad + 63) // 64 * 64
        pcm = aligned(ns * ch * cs, np.float32)
        pcm.view(np.uint32)[:] = 0x7fc0dead
        amp = np.zeros(ns, np.float32)
        fo = np.ascontiguousarray(frames_of, dtype=np.int64)
        bo = np.array([buf.ctypes.data + int(b) * buf.itemsize for b in base_elems], np.int64)
        self.L.ingest(dtype, ns, ch, frames, head, pad, pcm.ctypes.data, ch * cs, cs, amp.ctypes.data, fo.ctypes.data, bo.ctypes.data,
                      cstride, fstride, int(vec_ok))
        return pcm.reshape(ns, ch, cs), amp


# ---- the grid of layouts (tests/test_feed_source_cpu.py on a host buffer, tests/test_feed_device.py on a device one) ----
FRAMES = [1, 3, 4, 5, 1023, 2049, 5000]
OFFSETS = [0, 1, 2, 3]
LAYOUTS = ["planar", "pitch", "interleaved", "frame_stride_2", "mono_as_stereo", "reversed"]


def layout(name, n, offset, ns=3, ch=2):
    """Where ns streams of n frames in ch channels lie in one flat buffer whose element 0 is aligned: -> dict(elems = the
    buffer's length, base = per stream the element of (channel 0, frame 0), stream = the stride between streams, cstride,
    fstride, rows = the channel rows that exist: ch, or 1 where one row is shown as every channel)"""
    rows = ch
    if name == "planar":
        cst, fst, sst, first = n, 1, ch * n, 0
    elif name == "pitch":           # an odd row pitch
        cst, fst, sst, first = n + 1, 1, ch * (n + 1), 0
    elif name == "interleaved":     # (s, f, c)
        cst, fst, sst, first = 1, ch, ch * n, 0
    elif name == "frame_stride_2":  # every other element of rows twice as long
        cst, fst, sst, first = 2 * n, 2, 2 * ch * n, 0
    elif name == "mono_as_stereo":  # one row shown as every channel
        cst, fst, sst, first, rows = 0, 1, n, 0, 1
    elif name == "reversed":        # a negative frame stride: frame 0 is the row's last element
        cst, fst, sst, first = n, -1, ch * n, n - 1
    else:
        raise ValueError(name)
    return dict(elems=offset + ns * sst + 8, base=[offset + s * sst + first for s in range(ns)], stream=sst, cstride=cst, fstride=fst, rows=rows)


def scatter(buf, lay, values):
    """values [ns, rows, n] (the buffer's element type) -> into buf as the layout has them"""
    ns, rows, n = values.shape
    for s in range(ns):
        for c in range(rows):
            at = lay["base"][s] + c * lay["cstride"] + np.arange(n) * lay["fstride"]
            buf[at] = values[s, c]


def gather(buf, lay, ns, ch, n):
    """-> [ns, ch, n] of the buffer's element type: what a reader of the layout sees"""
    out = np.zeros((ns, ch, n), buf.dtype)
    for s in range(ns):
        for c in range(ch):
            out[s, c] = buf[lay["base"][s] + c * lay["cstride"] + np.arange(n) * lay["fstride"]]
    return out


def to_float(dtype, a):
    """numpy's own conversion of an array of source elements (s16: int16; f32: float32; f16: float16; bf16: the uint16 bits)"""
    if dtype == SRC_S16:
        return a.astype(np.float32) / np.float32(32768.0)
    if dtype == SRC_F32:
        return a.astype(np.float32)
    if dtype == SRC_F16:
        return a.astype(np.float32)
    return (a.astype(np.uint32) << 16).view(np.float32)


NP_DTYPE = {SRC_S16: np.int16, SRC_F32: np.float32, SRC_F16: np.float16, SRC_BF16: np.uint16}


def from_float(dtype, x):
    """float32 samples rounded to the source type: -> the array of source elements (bf16: its uint16 bits, round to nearest even)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    if dtype == SRC_S16:
        return np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16)
    if dtype == SRC_F32:
        return x.copy()
    if dtype == SRC_F16:
        return x.astype(np.float16)
    u = x.view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)
