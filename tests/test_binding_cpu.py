"""CPU suite: the Python binding without the library -- the prototype table against include/vorbis_amd.h (parameter counts,
kinds of return value, what is left unbound), and the Feed's nine synchronous helpers against recorders in the primitive
calls' place: which calls they make, with what, in which order, and that the slot is released once whatever fails."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from tests import checker
from vorbis_amd import DeviceSource, Feed, VamdError, SRC_F32
from vorbis_amd import abi

ROOT = checker.ROOT

UNBOUND = {"vamd_abi_version", "vamd_device_count", "vamd_batcher_create", "vamd_batcher_create_multi", "vamd_batcher_destroy",
           "vamd_batcher_attach", "vamd_batcher_detach", "vamd_batcher_encode_block", "vamd_batcher_last_error",
           "vamd_batcher_stats", "vamd_batcher_context", "vamd_batcher_report"}


def header_functions():
    """name -> (return type as written, number of parameters) of every function include/vorbis_amd.h declares"""
    src = open(os.path.join(ROOT, "include", "vorbis_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)                      # the declarations span lines, comments between them
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"^[ \t]*#(?:[^\n]*\\\n)*[^\n]*", " ", src, flags=re.M)   # preprocessor lines with their continuations
    out = {}
    for ret, name, params in re.findall(r"([A-Za-z_][\w \t\*]*?)\b(vamd_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", src):
        assert name not in out, name
        params = params.strip()
        out[name] = (" ".join(ret.split()), 0 if params in ("", "void") else params.count(",") + 1)
    return out


def test_prototypes_agree_with_the_header():
    hdr = header_functions()
    assert len(hdr) >= 80 and hdr["vamd_abi_version"] == ("int", 0) and hdr["vamd_create_abi"] == ("int", 5)
    assert hdr["vamd_feed_last_error"] == ("const char *", 1) and hdr["vamd_destroy"] == ("void", 1)
    for name, (restype, argtypes) in abi.PROTOTYPES.items():
        assert name in hdr, name + " is not declared in the header"
        ret, nparams = hdr[name]
        assert len(argtypes) == nparams, "%s: %d argtypes, the header has %d parameters" % (name, len(argtypes), nparams)
        if ret == "void":
            assert restype is None, name
        elif ret == "const char *":
            assert restype is C.c_char_p, name
        else:
            assert ret in ("int", "long") and restype in (C.c_int, C.c_long), name
    # a new function of the header is bound, or joins the unbound ones on purpose
    assert set(hdr) - set(abi.PROTOTYPES) == UNBOUND
    assert set(abi.UNBOUND_SYMBOLS) == UNBOUND
    assert sorted(abi.EXPORTED_SYMBOLS) == sorted(hdr) and len(abi.EXPORTED_SYMBOLS) == len(hdr)


# ---- the Feed's helpers over recorders ----
PRIMITIVES = ("buffer", "buffer_on", "device", "wrote", "wrote_live", "wrote_device", "wrote_live_device", "ogg_serials",
              "ogg_comments", "ogg_flush", "packets", "ogg", "decoded", "release")
SLOT = 3
PACKETS = {"nstreams": 3, "nblocks": 3, "stream_start": np.array([0, 2, 2, 3]), "offset": np.array([0, 2, 4]),
           "bits": np.array([16, -1, 9], np.int32), "granulepos": np.array([10, 20, 30]), "info": np.array([0, 1, 3], np.uint8),
           "bytes": np.array([1, 2, 9, 9, 5, 6, 7], np.uint8)}
ROWS = [[(b"\x01\x02", 10, 0, 0), (None, 20, 1, 0)], [], [(b"\x05\x06", 30, 1, 1)]]
OGG = {"nstreams": 3, "stream_offset": np.array([0, 3, 3, 5]), "bytes": np.array([79, 103, 103, 83, 0], np.uint8)}
FILES = [b"Ogg", b"", b"S\x00"]
DECODED = ["dec0", "dec1", "dec2"]


def plain(v):
    if isinstance(v, np.ndarray):
        return v.tolist()
    if isinstance(v, np.generic):
        return v.item()
    if isinstance(v, (list, tuple)):
        return [plain(x) for x in v]
    return v


class Boom(Exception):
    pass


def recording_feed(write_frames=None, lanes=1, dtype=np.int16, fail=None, release_fails=False):
    """A Feed that was never created in the library: the attributes the helpers read, and a recorder for every primitive.
    -> (feed, calls, arena, filled): calls = [(name, {parameter: value})] with each call's arguments bound to the real
    method's signature (defaults applied); filled = the arena's front as it was when the group was handed over."""
    f = Feed.__new__(Feed)
    f.h, f._held, f.write_frames, f.lanes, f.dtype, f.max_streams, f.max_frames, f.fmt = None, {}, write_frames, lanes, dtype, 4, 16, 0
    calls, arena, filled = [], np.full(64, -1, dtype), []
    results = {"buffer": (SLOT, arena), "buffer_on": (SLOT, arena), "device": 0, "packets": PACKETS, "ogg": OGG, "decoded": DECODED}

    def recorder(name):
        sig = inspect.signature(getattr(Feed, name))

        def call(*a, **k):
            b = sig.bind(f, *a, **k)
            b.apply_defaults()
            calls.append((name, {p: plain(v) if not isinstance(v, DeviceSource) else v for p, v in b.arguments.items() if p != "self"}))
            if name.startswith("wrote"):
                filled.append(arena.copy())
            if name == fail:
                raise Boom(name)
            if name == "release" and release_fails:
                raise VamdError(-131, "release refused")
            return results.get(name)
        return call
    for name in PRIMITIVES:
        setattr(f, name, recorder(name))
    return f, calls, arena, filled


SRC = DeviceSource([0x1000, 0x2000, 0], SRC_F32, 8, 1)
SRC_FRAMES = [4, 6, 0]
STEREO = np.arange(20, dtype=np.int16).reshape(2, 5, 2)
RAGGED = [np.arange(6, dtype=np.int16).reshape(3, 2), np.arange(10, 20, dtype=np.int16).reshape(5, 2)]
PIECES = [np.arange(6, dtype=np.int16).reshape(3, 2), np.zeros((0, 2), np.int16), np.zeros(0, np.int16)]   # two streams without frames
MONO = [np.arange(4, dtype=np.int16), np.zeros((0, 1), np.int16)]                                            # a 1-d piece: mono

rel = ("release", {"slot": SLOT})
pk = ("packets", {"slot": SLOT, "copy": True})
og = ("ogg", {"slot": SLOT, "copy": False})
ser = ("ogg_serials", {"slot": SLOT, "serials": [7, 8]})
com = ("ogg_comments", {"slot": SLOT, "comments": [b"c0", None]})
flu = ("ogg_flush", {"slot": SLOT, "flags": [True, False]})
OPTS = {"serials": [7, 8], "comments": [b"c0", None], "flush": [True, False]}


def buf(ch):
    return ("buffer", {"channels": ch})


def wrote(ns, frames):
    return ("wrote", {"slot": SLOT, "nstreams": ns, "frames": frames})


def wrote_live(frames, close):
    return ("wrote_live", {"slot": SLOT, "frames": frames, "close": close})


def wrote_device(stream="s", layout="sfc"):
    return ("wrote_device", {"slot": SLOT, "source": SRC, "frames": SRC_FRAMES, "stream": stream, "layout": layout})


def wrote_live_device(close, stream="s", layout="sfc"):
    return ("wrote_live_device", {"slot": SLOT, "source": SRC, "frames": SRC_FRAMES, "close": close, "stream": stream, "layout": layout})


# (helper, live feed, arguments, the calls the parent's helper makes, its result, what lies in the arena at wrote time)
CASES = [
    ("encode", False, ((STEREO,), {}), [buf(2), wrote(2, 5), pk, rel], ROWS[:2], STEREO.reshape(-1)),
    ("encode", False, ((RAGGED,), {}), [buf(2), wrote(2, [3, 5]), pk, rel], ROWS[:2], np.concatenate([x.reshape(-1) for x in RAGGED])),
    ("encode_ogg", False, ((STEREO,), {}), [buf(2), wrote(2, 5), og, rel], FILES[:2], STEREO.reshape(-1)),
    ("encode_ogg", False, ((RAGGED,), {"serials": [7, 8], "comments": [b"c0", None]}), [buf(2), ser, com, wrote(2, [3, 5]), og, rel], FILES[:2],
     np.concatenate([x.reshape(-1) for x in RAGGED])),
    ("encode_ogg", False, ((STEREO,), {"comments": [b"c0", None]}), [buf(2), com, wrote(2, 5), og, rel], FILES[:2], STEREO.reshape(-1)),
    ("encode_live", True, ((PIECES,), {}), [buf(2), wrote_live([3, 0, 0], None), pk, rel], ROWS, PIECES[0].reshape(-1)),
    ("encode_live", True, ((MONO,), {"close": [0, 1]}), [buf(1), wrote_live([4, 0], [0, 1]), pk, rel], ROWS[:2], MONO[0]),
    ("encode_live_ogg", True, ((PIECES,), {}), [buf(2), wrote_live([3, 0, 0], None), og, rel], FILES, PIECES[0].reshape(-1)),
    ("encode_live_ogg", True, ((MONO,), dict(OPTS, close=[1, 0])), [buf(1), ser, com, flu, wrote_live([4, 0], [1, 0]), og, rel], FILES[:2], MONO[0]),
    ("encode_live_ogg", True, ((MONO,), {"flush": [True, False]}), [buf(1), flu, wrote_live([4, 0], None), og, rel], FILES[:2], MONO[0]),
    ("encode_tensors", False, ((SRC, SRC_FRAMES, "s", "sfc"), {}), [buf(None), wrote_device(), pk, rel], ROWS, None),
    ("encode_tensors", False, ((SRC, SRC_FRAMES), {}), [buf(None), wrote_device(None, "scf"), pk, rel], ROWS, None),
    ("roundtrip_tensors", False, ((SRC, SRC_FRAMES, "s", "sfc"), {}),
     [buf(None), wrote_device(), pk, ("decoded", {"slot": SLOT, "copy": True, "with_status": False}), rel], (ROWS, DECODED), None),
    ("encode_ogg_tensors", False, ((SRC, SRC_FRAMES), {"stream": "s", "layout": "sfc"}), [buf(None), wrote_device(), og, rel], FILES, None),
    ("encode_ogg_tensors", False, ((SRC, SRC_FRAMES, [7, 8], [b"c0", None], "s", "sfc"), {}), [buf(None), ser, com, wrote_device(), og, rel], FILES, None),
    ("encode_live_tensors", True, ((SRC, SRC_FRAMES, [0, 0, 1], "s", "sfc"), {}), [buf(None), wrote_live_device([0, 0, 1]), pk, rel], ROWS, None),
    ("encode_live_tensors", True, ((SRC, SRC_FRAMES), {}), [buf(None), wrote_live_device(None, None, "scf"), pk, rel], ROWS, None),
    ("encode_live_ogg_tensors", True, ((SRC, SRC_FRAMES), {"stream": "s", "layout": "sfc"}), [buf(None), wrote_live_device(None), og, rel], FILES, None),
    ("encode_live_ogg_tensors", True, ((SRC, SRC_FRAMES, [0, 0, 1], [7, 8], [b"c0", None], [True, False], "s", "sfc"), {}),
     [buf(None), ser, com, flu, wrote_live_device([0, 0, 1]), og, rel], FILES, None),
]
IDS = ["%s-%d" % (c[0], i) for i, c in enumerate(CASES)]


@pytest.mark.parametrize("helper,live,args,want,result,samples", CASES, ids=IDS)
def test_helper_makes_the_parents_calls(helper, live, args, want, result, samples):
    f, calls, arena, filled = recording_feed(write_frames=512 if live else None)
    got = getattr(f, helper)(*args[0], **args[1])
    assert calls == want
    assert got == result
    if samples is not None:     # the samples lay flat at the arena's front when the group was handed over, nothing behind them touched
        assert len(filled) == 1 and np.array_equal(filled[0][:samples.size], samples) and (filled[0][samples.size:] == -1).all()


@pytest.mark.parametrize("release_fails", [False, True])
@pytest.mark.parametrize("helper,live,args,want,result,samples", CASES, ids=IDS)
def test_slot_is_released_once_whatever_fails(helper, live, args, want, result, samples, release_fails):
    """Each call between the slot and its release made to raise in turn: the calls up to it are the parent's, release()
    follows exactly once, and that exception comes out -- also when the release itself then fails with a VamdError."""
    for at in range(1, len(want) - 1):
        f, calls, arena, filled = recording_feed(write_frames=512 if live else None, fail=want[at][0], release_fails=release_fails)
        with pytest.raises(Boom) as e:
            getattr(f, helper)(*args[0], **args[1])
        assert e.value.args == (want[at][0],)
        assert calls == want[:at + 1] + [rel]
    # nothing fails but the release: its VamdError is dropped, the result stands
    if release_fails:
        f, calls, arena, filled = recording_feed(write_frames=512 if live else None, release_fails=True)
        assert getattr(f, helper)(*args[0], **args[1]) == result and calls == want


def test_a_fill_that_fails_releases_the_slot():
    """More samples than the arena holds: the copy raises before any group exists, and the slot is given back."""
    f, calls, arena, filled = recording_feed()
    with pytest.raises(ValueError):
        f.encode(np.zeros((1, 40, 2), np.int16))
    assert calls == [buf(2), rel]


LIVE_ARGS = {"encode_live": (PIECES,), "encode_live_ogg": (PIECES,), "encode_live_tensors": (SRC, SRC_FRAMES),
             "encode_live_ogg_tensors": (SRC, SRC_FRAMES)}
NOT_LIVE = {"encode_live": "encode_live needs a live feed (Feed(..., write_frames=...))",
            "encode_live_ogg": "encode_live_ogg needs a live feed (Feed(..., write_frames=..., ogg_headers=...))",
            "encode_live_tensors": "encode_live_tensors needs a live feed (Feed(..., write_frames=...))",
            "encode_live_ogg_tensors": "encode_live_ogg_tensors needs a live feed (Feed(..., write_frames=..., ogg_headers=...))"}
TWO_LANES = {"encode_live": "encode_live drives a feed with one lane; with more, use buffer / wrote_live / packets / release",
             "encode_live_ogg": "encode_live_ogg drives a feed with one lane; with more, use buffer / wrote_live / ogg / release",
             "encode_live_tensors": "encode_live_tensors drives a feed with one lane; with more, use buffer_on / wrote_live_device / packets / release",
             "encode_live_ogg_tensors": "encode_live_ogg_tensors drives a feed with one lane; with more, use buffer_on / wrote_live_device / ogg / release"}


@pytest.mark.parametrize("helper", sorted(LIVE_ARGS))
def test_live_helpers_need_a_live_feed_with_one_lane(helper):
    f, calls, arena, filled = recording_feed(write_frames=None)
    with pytest.raises(ValueError) as e:
        getattr(f, helper)(*LIVE_ARGS[helper])
    assert str(e.value) == NOT_LIVE[helper] and calls == []
    f, calls, arena, filled = recording_feed(write_frames=512, lanes=2)
    with pytest.raises(ValueError) as e:
        getattr(f, helper)(*LIVE_ARGS[helper])
    assert str(e.value) == TWO_LANES[helper] and calls == []


def test_a_live_group_without_pieces_takes_no_slot():
    f, calls, arena, filled = recording_feed(write_frames=512)
    for helper in ("encode_live", "encode_live_ogg"):
        with pytest.raises(ValueError):
            getattr(f, helper)([])
    assert calls == []


def test_rows_and_files_of_a_hand_made_result():
    """A block with bits < 0 has no packet (None), a stream may have no blocks; a packet is the first (bits + 7) / 8 bytes
    at its offset, W and e_o_s are info's low bits; a file is its slice of the bytes, empty where the stream has none."""
    assert Feed._rows(PACKETS, 3) == ROWS and Feed._rows(PACKETS, 1) == ROWS[:1] and Feed._rows(PACKETS, 0) == []
    f, calls, arena, filled = recording_feed()
    assert f._rows(PACKETS, 2) == ROWS[:2]
    assert Feed._files(OGG) == FILES and Feed._files(OGG, 3) == FILES and Feed._files(OGG, 1) == [b"Ogg"]
    assert all(type(x) is bytes for x in Feed._files(OGG))
