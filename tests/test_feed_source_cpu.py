"""CPU suite: the source side of the device-fed feed -- vorbis_amd/csrc/k_feed_src.h compiled with the host compiler
(tests/feed_source_host.py): the conversion of every 16-bit pattern against numpy, the ingest body over a host buffer for
every layout and misalignment the GPU suite walks (the vector-load path and the element path against each other and
against a numpy gather), and the host's range check."""

import numpy as np
import pytest

from tests import feed_source_host as fs

HEAD, PAD = 1024, 3 * 2048  # the stereo q4 setup's room in front of and behind a stream (blocks 256 / 2048)


@pytest.fixture(scope="module")
def host():
    return fs.HostSource(fs.build())


def test_conversion_of_every_16_bit_pattern(host):
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    # s16: x / 32768.f (examples/encoder_example.c:197-202)
    got = host.convert16(fs.SRC_S16, bits)
    assert np.array_equal(got.view(np.uint32), (bits.view(np.int16).astype(np.float32) / np.float32(32768.0)).view(np.uint32))
    # f16: numpy's astype -- exact, subnormals normalised, signed zeros and infinities kept; NaNs compared as "is NaN"
    got = host.convert16(fs.SRC_F16, bits)
    want = bits.view(np.float16).astype(np.float32)
    nan = np.isnan(want)
    assert nan.sum() == 2 * 1023 and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    sub = ((bits & 0x7c00) == 0) & ((bits & 0x3ff) != 0)
    assert sub.sum() == 2 * 1023 and np.all(got[sub] != 0) and np.all(np.abs(got[sub]) < 2.0 ** -14)
    # bf16: the bits placed in the float's upper half
    got = host.convert16(fs.SRC_BF16, bits)
    want = (bits.astype(np.uint32) << 16).view(np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan])
    # what the live ingest marks: infinities and NaNs, nothing else
    for dtype in (fs.SRC_F16, fs.SRC_BF16):
        f = host.convert16(dtype, bits)
        marked = np.array([host.non_finite(float(x)) for x in f[::7]])
        assert np.array_equal(marked, ~np.isfinite(f[::7]))


def values_of(rng, dtype, shape):
    """source elements of every kind: full-range values, and for the float types a few subnormals and signed zeros"""
    x = ((rng.random(shape) - 0.5) * 1.9).astype(np.float32)
    v = fs.from_float(dtype, x)
    if dtype in (fs.SRC_F16, fs.SRC_BF16):
        flat = v.reshape(-1).view(np.uint16)
        flat[::97] = 0x8000
        flat[5::89] = 0x0001 + (np.arange(flat[5::89].size) % 1000).astype(np.uint16)
    return v


@pytest.mark.parametrize("dtype", [fs.SRC_S16, fs.SRC_F32, fs.SRC_F16, fs.SRC_BF16], ids=["s16", "f32", "f16", "bf16"])
@pytest.mark.parametrize("frames", fs.FRAMES)
def test_ingest_body_over_every_layout(host, dtype, frames):
    """Three streams of `frames` frames, stereo, in every layout at every element offset: the vector-load path and the element
    path give the same stream buffers, those are a numpy gather of the source between a zeroed head and a zeroed pad (the
    tail of the last quad included), and nothing outside them is written."""
    rng = np.random.default_rng(frames * 8 + dtype)
    ns, ch, nd = 3, 2, fs.NP_DTYPE[dtype]
    for name in fs.LAYOUTS:
        for offset in fs.OFFSETS:
            lay = fs.layout(name, frames, offset, ns, ch)
            buf = fs.aligned(lay["elems"], nd)
            buf[:] = values_of(rng, dtype, (lay["elems"],))  # (what lies between the rows is not zero either)
            scatter_vals = values_of(rng, dtype, (ns, lay["rows"], frames))
            fs.scatter(buf, lay, scatter_vals)
            seen = fs.gather(buf, lay, ns, ch, frames)
            want = fs.to_float(dtype, seen)
            outs = []
            for vec_ok in (True, False):
                pcm, amp = host.ingest(dtype, buf, lay["base"], [frames] * ns, ch, lay["cstride"], lay["fstride"], HEAD, PAD, vec_ok)
                assert np.all(amp == np.float32(fs.AMP_FLOOR))
                outs.append(pcm)
            assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), (name, offset)
            pcm = outs[0]
            quads = (frames + 3) & ~3
            assert np.array_equal(pcm[:, :, HEAD:HEAD + frames].view(np.uint32), want.view(np.uint32)), (name, offset)
            assert not pcm[:, :, :HEAD].view(np.uint32).any() and not pcm[:, :, HEAD + frames:HEAD + quads + PAD].view(np.uint32).any(), (name, offset)
            assert np.all(pcm[:, :, HEAD + quads + PAD:].view(np.uint32) == 0x7fc0dead), (name, offset)  # (the 64-sample rounding: untouched)


def test_ingest_body_ragged_group(host):
    """Streams of unequal length in one group: each buffer is laid out for the longest, the rest of a shorter one zeroed."""
    rng = np.random.default_rng(3)
    lengths = [2049, 1, 700, 5, 1500]
    longest = max(lengths)
    buf = fs.aligned(sum(2 * n + 3 for n in lengths), np.float16)
    buf[:] = values_of(rng, fs.SRC_F16, buf.shape)
    base, at = [], 1
    for n in lengths:
        base.append(at)
        at += 2 * n + 3
    for vec_ok in (True, False):
        # planar rows of each stream's own length would need a stride per stream: the group is interleaved (stride 2, 1)
        pcm, _ = host.ingest(fs.SRC_F16, buf, base, lengths, 2, 1, 2, HEAD, PAD, vec_ok, frames=longest)
        for s, n in enumerate(lengths):
            want = buf[base[s]:base[s] + 2 * n].reshape(n, 2).T.astype(np.float32)
            assert np.array_equal(pcm[s, :, HEAD:HEAD + n].view(np.uint32), want.view(np.uint32))
            assert not pcm[s, :, HEAD + n:HEAD + ((longest + 3) & ~3) + PAD].view(np.uint32).any()


def test_source_extent(host):
    ext = host.extent
    # positive strides: planar stereo rows of 100 frames, 4-byte elements, at the start of an allocation that just holds them
    assert ext(2, 100, 100, 1, 4, 0, 800) == (0, 0, 200)
    assert ext(2, 100, 100, 1, 4, 0, 799)[0] == 3                 # one byte short
    assert ext(2, 100, 100, 1, 4, 4, 800)[0] == 3                 # one element over, by the base's offset
    assert ext(2, 100, 101, 1, 4, 0, 800)[0] == 3                 # ... by the row pitch
    assert ext(2, 100, 101, 1, 4, 0, 804) == (0, 0, 201)
    assert ext(2, 100, 1, 2, 2, 0, 400) == (0, 0, 200)            # interleaved
    assert ext(2, 101, 1, 2, 2, 0, 400)[0] == 3
    # zero strides: one row shown to both channels; one frame shown as every frame
    assert ext(2, 100, 0, 1, 2, 0, 200) == (0, 0, 100)
    assert ext(2, 100, 0, 0, 2, 6, 8) == (0, 0, 1)
    assert ext(2, 100, 0, 0, 2, 8, 8)[0] == 3
    # negative strides count downwards from the base
    assert ext(2, 100, 100, -1, 4, 99 * 4, 800) == (0, -99, 101)
    assert ext(2, 100, 100, -1, 4, 98 * 4, 800)[0] == 2           # begins one element before the allocation
    assert ext(2, 100, -100, -1, 4, 199 * 4, 800) == (0, -199, 1)
    assert ext(2, 100, -100, -1, 4, 199 * 4, 799)[0] == 3
    assert ext(2, 100, -100, 1, 4, 400, 800) == (0, -100, 100)
    assert ext(2, 100, -101, 1, 4, 400, 800)[0] == 2
    # frames 0 and 1
    assert ext(2, 0, 1 << 40, 1 << 40, 4, 0, 0) == (0, 0, 0)      # nothing is read, whatever the strides
    assert ext(2, 1, 7, 1 << 40, 4, 0, 32) == (0, 0, 8)           # one frame: the frame stride is never used
    assert ext(2, 1, 7, 1 << 40, 4, 0, 31)[0] == 3
    assert ext(1, 1, 1 << 40, 1 << 40, 2, 0, 2) == (0, 0, 1)
    # strides of 1 << 40 are out of range, not wrapped
    assert ext(2, 100, 1 << 40, 1, 4, 0, 1 << 30)[0] == 3
    assert ext(2, 100, 1, 1 << 40, 4, 0, 1 << 30)[0] == 3
    assert ext(2, 100, -(1 << 40), 1, 4, 0, 1 << 30)[0] == 2
    # products beyond 64 bits are reported, never wrapped into range
    big = (1 << 62) + 1
    assert ext(8, 100, big, 1, 4, 0, 1 << 30)[0] == 1
    assert ext(2, 1 << 30, 1, 1 << 40, 4, 0, 1 << 30)[0] == 1
    assert ext(2, 3, 1 << 62, 1 << 62, 4, 0, 1 << 30)[0] == 1     # the sum of the two
    assert ext(2, 2, (1 << 62) - 1, 0, 4, 0, 1 << 30)[0] == 1     # the bytes
    assert ext(2, 2, 0, -(1 << 62), 4, 0, 1 << 30)[0] == 1
    # refused arguments
    assert ext(0, 1, 1, 1, 4, 0, 8)[0] == 1 and ext(2, -1, 1, 1, 4, 0, 8)[0] == 1 and ext(2, 1, 1, 1, 4, -4, 8)[0] == 1
