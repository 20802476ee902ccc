"""What the output-format tests share (tests/test_decode_formats_cpu.py on the one-lane host build,
tests/test_decode_formats_gpu.py on the GPU): the table of edge values, and the expected elements of a format for given
floats -- S16 by ov_read's rule written out in numpy, F16 / BF16 by torch's CPU conversion -- compared as bits."""
import numpy as np
import torch

DTYPES = ("f32", "s16", "f16", "bf16")  # VAMD_PCM_* 0 .. 3
ELEM = {"f32": np.uint32, "s16": np.int16, "f16": np.uint16, "bf16": np.uint16}
TORCH = {"f32": torch.float32, "s16": torch.int16, "f16": torch.float16, "bf16": torch.bfloat16}


def edge_table():
    t = []
    for v in (0.5, 1.5, 2.5):                                     # ties on both sides of zero
        t += [v / 32768.0, -v / 32768.0]
    t += [32766.5 / 32768.0, 32767.5 / 32768.0, -32768.5 / 32768.0]
    t += [1.0, -1.0, 2.0, -2.0, 65535.99, -65535.99]              # (+-65535.99: just inside 2^31 after scaling)
    t += [65536.0, -65536.0, np.inf, -np.inf, np.nan, -0.0, 0.0]
    t += [1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38]           # fp32 denormals
    t += [2.0 ** -24, -2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -24, 2.5 * 2.0 ** -24, 3e-6, 2.0 ** -15, 2.0 ** -14,
          2.0 ** -14 * (1 - 2.0 ** -11), 2.0 ** -14 * (1 - 2.0 ** -12)]      # fp16 denormals, their ties, the edge to normals
    t += [1 + 2.0 ** -11, 1 + 3 * 2.0 ** -11, -(1 + 2.0 ** -11), 1 + 2.0 ** -11 + 2.0 ** -20]  # fp16 ties, and just above one
    t += [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 3 * 2.0 ** -8), 1 + 2.0 ** -8 + 2.0 ** -20]   # bf16 ties, and just above one
    t += [65504.0, 65519.996, 65520.0, -65520.0, 3.3895314e38, 3.4e38, -3.4e38]               # fp16's and bf16's overflow thresholds
    t += [0.25, -0.7, 0.999969, 1e-3]
    return np.array(t, np.float32)


def want_s16(x):
    """ov_read's value for |x * 32768| < 2^31; beyond, saturated by sign, NaN -> 0 (include/vorbis_amd.h)"""
    x = np.asarray(x, np.float32)
    y = x.astype(np.float64) * 32768.0
    inside = np.abs(y) < 2.0 ** 31
    with np.errstate(invalid="ignore"):
        r = np.clip(np.rint(np.where(inside, y, 0.0)), -32768, 32767)
        r = np.where(inside, r, np.where(np.isnan(y), 0.0, np.where(y > 0, 32767.0, -32768.0)))
    return r.astype(np.int16)


def want_bits(x, dtype):
    """the expected elements of `dtype` for the floats x (any shape, kept)"""
    x = np.ascontiguousarray(x, np.float32)
    if dtype == "f32":
        return x.view(np.uint32)
    if dtype == "s16":
        return want_s16(x)
    return torch.from_numpy(x.copy()).to(TORCH[dtype]).view(torch.int16).numpy().view(np.uint16)


def differ(got, want, dtype):
    """where the elements differ: as bits, but that a NaN equals any NaN -- torch's CPU conversion writes a bfloat16 NaN as
    0x7fc0 on its scalar path and 0xffff on its vector path, and the header promises that a NaN stays one, no payload"""
    got, want = np.asarray(got), np.asarray(want)
    ne = got != want
    if dtype in ("f16", "bf16"):
        e, m = (0x7c00, 0x03ff) if dtype == "f16" else (0x7f80, 0x007f)
        ne &= ~((((got & e) == e) & ((got & m) != 0)) & (((want & e) == e) & ((want & m) != 0)))
    return ne


def tensor_bits(t, dtype):
    """a tensor of the format's torch dtype -> its elements as want_bits gives them"""
    assert t.dtype == TORCH[dtype], (t.dtype, dtype)
    t = t.detach().cpu().contiguous()
    if dtype == "f32":
        return t.numpy().view(np.uint32)
    if dtype == "s16":
        return t.numpy()
    return t.view(torch.int16).numpy().view(np.uint16)
