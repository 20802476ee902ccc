"""CPU: the decoded signal's output formats (vamd_decode_output; k_synth.h, "the lap in the caller's format") on the one-lane
host build, tests/c/decode_formats_host.cpp under -fsanitize=address,undefined.

* The conversion helpers over a hand-made table of edge values: S16 against ov_read's rule (round to nearest even of
  x * 32768 in double, clipped; beyond 2^31 the header's stated values), F16 / BF16 against torch's CPU conversion, as bits.
* lap_window_as / lap_row in every instantiation over one stream whose blocks form all four (lW, W) pairs: every thread of
  the launch in turn, held to lap_find / lap_sample's floats (tests/c/synth_host.cpp) converted by the same formulas, with
  guard elements in front of, between and behind the rows."""
import os
import subprocess

import numpy as np
import pytest

import vorbis_amd
from tests import hostbuild, synth_host
from tests.decode_formats_cases import DTYPES, ELEM, differ, edge_table, want_bits

GUARD = 16


@pytest.fixture(scope="module")
def exe():
    return hostbuild.program("decode_formats_host.cpp")


def test_the_table_holds_what_it_is_there_for():
    x = edge_table()
    y = x.astype(np.float64) * 32768.0
    assert (np.abs(y[np.isfinite(y)]) >= 2.0 ** 31).any() and (np.abs(y) < 2.0 ** 31).sum() > 40
    assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
    assert ((x != 0) & (np.abs(x) < 1.17549435e-38)).any()                                # fp32 denormals
    assert ((np.abs(x) < 2.0 ** -14) & (np.abs(x) >= 2.0 ** -24)).any()                    # fp16 denormals
    assert float(x[list(x).index(np.float32(65535.99))]) * 32768.0 < 2.0 ** 31


def test_conversion_helpers_on_the_edge_table(exe, tmp_path):
    x = edge_table()
    src, out = os.path.join(str(tmp_path), "table.f32"), os.path.join(str(tmp_path), "table.out")
    x.tofile(src)
    r = subprocess.run([exe, "convert", src, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    raw = np.fromfile(out, np.uint8)
    assert raw.size == 6 * x.size
    got = {"s16": raw[:2 * x.size].view(np.int16), "f16": raw[2 * x.size:4 * x.size].view(np.uint16), "bf16": raw[4 * x.size:].view(np.uint16)}
    for d in ("s16", "f16", "bf16"):
        want = want_bits(x, d)
        bad = [(float(v), int(g), int(w)) for v, g, w, ne in zip(x, got[d], want, differ(got[d], want, d)) if ne]
        assert not bad, (d, bad)
    # the stated values beyond the reference's range, spelled out
    s = dict(zip([repr(float(v)) for v in x], got["s16"]))
    assert s["65536.0"] == 32767 and s["-65536.0"] == -32768 and s["inf"] == 32767 and s["-inf"] == -32768 and s["nan"] == 0


# ---- the lap bodies ----
BLOCK_W = (1, 1, 0, 0, 1, 1)   # long/long, long/short, short/short, short/long
LONG = 3001                    # not a multiple of 8, across all the blocks
CASES = [(start, frames, offset, 3) for frames in (1, 3, 5, 7, 9, LONG) for offset in (0, 1) for start in (0, 37)]


def stream_blocks(ch, bs):
    kinds = {W: list(synth_host.block_set(ch, bs[W], 11 + W).values()) for W in (0, 1)}
    return [(W, kinds[W][(2 * k) % len(kinds[W])]) for k, W in enumerate(BLOCK_W)]


@pytest.mark.parametrize("ch", [1, 2, 3, 6])
def test_lap_bodies_in_every_format(exe, tmp_path, ch):
    blob = vorbis_amd.default_setup_blob("44k_stereo_q4")
    bs = (256, 2048)
    win = synth_host.windows(blob, bs)
    blocks = stream_blocks(ch, bs)
    assert synth_host.lap_cases([W for W, _ in blocks]) == {(0, 0), (0, 1), (1, 0), (1, 1)}
    span = sum(bs[a] // 4 + bs[b] // 4 for a, b in zip(BLOCK_W[:-1], BLOCK_W[1:]))
    assert max(s + f for s, f, _, _ in CASES) <= span and LONG % 8 and LONG > span // 2
    full = synth_host.host_lap(synth_host.build(), tmp_path, bs, win, blocks, span)   # lap_find / lap_sample per frame: [ch][span]
    assert np.abs(full).max() > 0.1
    job, out = os.path.join(str(tmp_path), "formats.job"), os.path.join(str(tmp_path), "formats.out")
    with open(job, "wb") as f:
        f.write(np.array([ch, bs[0], bs[1], len(blocks), len(CASES)], np.int32).tobytes() + np.array(CASES, np.int32).tobytes())
        f.write(np.ascontiguousarray(win[0], np.float32).tobytes() + np.ascontiguousarray(win[1], np.float32).tobytes())
        for W, pcm in blocks:
            f.write(np.int32(W).tobytes() + np.ascontiguousarray(pcm, np.float32).tobytes())
    r = subprocess.run([exe, "lap", job, out], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    raw, at, bad = np.fromfile(out, np.uint8), 0, []
    for d in DTYPES:
        size = np.dtype(ELEM[d]).itemsize
        guard = np.frombuffer(b"\xa5" * size, ELEM[d])[0]
        for il in (False, True):
            for start, frames, offset, pad in CASES:
                stride = frames + pad
                region = frames * ch if il else ch * stride
                total = GUARD + offset + region + GUARD
                buf = raw[at:at + total * size].view(ELEM[d])
                at += total * size
                body = buf[GUARD + offset:GUARD + offset + region]
                want = full[:, start:start + frames]
                if il:
                    got, untouched = body, np.concatenate([buf[:GUARD + offset], buf[GUARD + offset + region:]])
                    want = want_bits(np.ascontiguousarray(want.T).reshape(-1), d)
                else:
                    rows = body.reshape(ch, stride)
                    got, untouched = rows[:, :frames].reshape(-1), np.concatenate([buf[:GUARD + offset], rows[:, frames:].reshape(-1), buf[GUARD + offset + region:]])
                    want = want_bits(np.ascontiguousarray(want).reshape(-1), d)
                if differ(got, want, d).any() or not (untouched == guard).all():
                    bad.append((d, il, start, frames, offset, int(differ(got, want, d).sum()), int((untouched != guard).sum())))
    assert at == raw.size
    assert not bad, bad[:20]
