"""ctypes mirror of include/vorbis_amd.h: its constants, its structures, the prototypes of the functions the binding calls
(PROTOTYPES, one table) and the loader.  Names and argument meaning follow the C ABI, which in turn follows libvorbis
(mapping0_forward's variables and OV_* return codes)."""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))

VAMD_OK, VAMD_EFAULT, VAMD_EIMPL, VAMD_EINVAL, VAMD_EVERSION, VAMD_EDOMAIN, VAMD_ENONFINITE = 0, -129, -130, -131, -134, -140, -141
VAMD_ENOTVORBIS, VAMD_EBADHEADER = -132, -133  # vamd_create_decoder: what vorbis_synthesis_headerin answers for a header packet
ABI_VERSION = 9             # VAMD_ABI_VERSION of the header this mirror was written against
QUANT_LIMIT_SQUARE, QUANT_LIMIT_INT = 46340, 0x7fffff80
STATUS_RANGE, STATUS_NONFINITE = 1, 2   # bits of the `status` output (vorbis_amd.h, "Input domain")
STATUS_NOTAUDIO, STATUS_BADCODE, STATUS_TRUNCATED = 4, 8, 16  # a decoded stream's status (vorbis_amd.h, "the packet decoder")
STATUS_PARTIAL = 128  # informative, under Analyzer.keep_partial: a packet of the stream was decoded in part, as libvorbis decodes it
STATUS_BADPAGE, STATUS_BADHEADER = 32, 64  # ... of a decoded file on top (vorbis_amd.h, "Ogg Vorbis files in")
LEVEL_TRANSFORM, LEVEL_PSY, LEVEL_FULL = 1, 2, 3
POSTS_STRIDE = 32
BLOCKTYPE_IMPULSE, BLOCKTYPE_PADDING, BLOCKTYPE_TRANSITION, BLOCKTYPE_LONG = 0, 1, 0, 1
PACKETBLOBS = 15
RES_CLASS_STRIDE = 512
MAX_CH = 8

FEED_S16, FEED_F32 = 0, 1
FEED_NO_ARENA = 0x100                       # or'ed into fmt: no pinned input arena, device-fed groups only
FEED_DECODED = 0x200                        # or'ed into fmt: the decoded signal beside the packets (Feed(decoded=True))
SRC_S16, SRC_F32, SRC_F16, SRC_BF16 = 0, 1, 2, 3   # VAMD_SRC_*: a device-fed group's element type
PCM_F32, PCM_S16, PCM_F16, PCM_BF16 = 0, 1, 2, 3   # VAMD_PCM_*: the decoded signal's element type (vamd_decode_output)

_vp = C.c_void_p


class _Plan(C.Structure):
    _fields_ = [("nstreams", C.c_int64), ("nblocks", C.c_int64 * 2), ("lW", _vp * 2), ("nW", _vp * 2), ("blocktype", _vp * 2),
                ("src", _vp * 2), ("order", _vp), ("stream_start", _vp)]


class _FeedResult(C.Structure):  # vamd_feed_result
    _fields_ = [("nstreams", C.c_int64), ("nblocks", C.c_int64), ("stream_start", _vp), ("offset", _vp), ("bits", _vp),
                ("granulepos", _vp), ("info", _vp), ("bytes", _vp), ("total_bytes", C.c_int64), ("upload_ms", C.c_double),
                ("device_ms", C.c_double), ("total_ms", C.c_double)]


class _FeedSource(C.Structure):  # vamd_feed_source
    _fields_ = [("base", _vp), ("dtype", C.c_int), ("channel_stride", C.c_int64), ("frame_stride", C.c_int64), ("producer", _vp)]


class _FeedOggResult(C.Structure):  # vamd_feed_ogg_result
    _fields_ = [("nstreams", C.c_int64), ("stream_offset", _vp), ("npages", _vp), ("status", _vp), ("bytes", _vp),
                ("total_bytes", C.c_int64)]


class _FeedDecodedResult(C.Structure):  # vamd_feed_decoded_result
    _fields_ = [("nstreams", C.c_int64), ("channels", C.c_int32), ("frames", _vp), ("offset", _vp), ("status", _vp), ("pcm", _vp),
                ("total_floats", C.c_int64)]


class _DecodeDesc(C.Structure):  # vamd_decode_desc
    _fields_ = [("nstreams", C.c_int64), ("npackets", C.c_int64), ("bytes", _vp), ("offset", _vp), ("stream_start", _vp), ("end_granule", _vp)]


class _DecodeMarks(C.Structure):  # vamd_decode_marks
    _fields_ = [("granule", _vp), ("eos", _vp)]


class _OggLink(C.Structure):  # vamd_ogg_link
    _fields_ = [("begin", C.c_int64), ("end", C.c_int64), ("serial", C.c_uint32)]


class _PcmFormat(C.Structure):  # vamd_pcm_format
    _fields_ = [("dtype", C.c_int), ("interleaved", C.c_int)]


class _DecodeLiveDesc(C.Structure):  # vamd_decode_live_desc
    _fields_ = [("nstreams", C.c_int64), ("npackets", C.c_int64), ("slot", _vp), ("bytes", _vp), ("offset", _vp), ("stream_start", _vp),
                ("close", _vp), ("end_granule", _vp)]


class _DecodeOggDesc(C.Structure):  # vamd_decode_ogg_desc
    _fields_ = [("nstreams", C.c_int64), ("bytes", _vp), ("file_offset", _vp), ("setup_header", _vp), ("setup_header_bytes", C.c_int64)]


class _OggWindowDesc(C.Structure):  # vamd_ogg_window_desc
    _fields_ = [("nwindows", C.c_int64), ("stream", _vp), ("start", _vp), ("count", _vp), ("bytes", _vp), ("file_offset", _vp),
                ("channel_stride", _vp)]


class _DecodeOggLiveOpts(C.Structure):  # vamd_decode_ogg_live_opts
    _fields_ = [("setup_header", _vp), ("setup_header_bytes", C.c_int64), ("max_packet_bytes", C.c_int64), ("max_header_bytes", C.c_int64)]


class _DecodeOggLiveDesc(C.Structure):  # vamd_decode_ogg_live_desc
    _fields_ = [("nstreams", C.c_int64), ("slot", _vp), ("bytes", _vp), ("piece_offset", _vp), ("close", _vp)]


class _Desc(C.Structure):
    _fields_ = [("W", C.c_int), ("nblocks", C.c_long), ("lW", _vp), ("nW", _vp), ("blocktype", _vp),
                ("ampmax_in", _vp), ("uniform_lW", C.c_int), ("uniform_nW", C.c_int),
                ("uniform_blocktype", C.c_int), ("uniform_ampmax_in", C.c_float)]


_IO_FIELDS = ["pcm", "mdct_raw", "logfft", "logmdct", "noise", "tone", "logmask", "mdct", "posts", "post_valid",
              "ilogmask", "iwork", "nonzero", "local_ampmax", "ampmax_out", "res_class", "res_entries", "res_count"]


class _IO(C.Structure):
    _fields_ = [(k, _vp) for k in _IO_FIELDS] + [("packets", _vp), ("packet_bits", _vp), ("packet_stride", C.c_int64),
                                                 ("status", _vp), ("pcm_src", _vp), ("pcm_channel_stride", C.c_int64)]


class _MIO(C.Structure):  # vamd_managed_io
    _fields_ = [(k, _vp) for k in ("posts", "post_valid", "iwork", "nonzero", "res_class", "res_entries", "res_count",
                                   "packets", "packet_bits")] + [("packet_stride", C.c_int64)]


class EnvelopeState(C.Structure):
    """vamd_envelope_state (include/vorbis_amd.h); all-zero = start of a stream."""
    _fields_ = [("steps", C.c_int64), ("stretch", C.c_int32), ("pad", C.c_int32),
                ("near_hist", C.c_float * 30 * MAX_CH), ("amp_hist", C.c_float * 8 * 16 * MAX_CH)]


class VamdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("vorbis_amd error %d: %s" % (code, msg))
        self.code = code


_int, _long, _size, _float = C.c_int, C.c_long, C.c_size_t, C.c_float
_pvp, _pint, _plong, _pfloat, _pi32 = C.POINTER(_vp), C.POINTER(C.c_int), C.POINTER(C.c_long), C.POINTER(C.c_float), C.POINTER(C.c_int32)
_pDesc, _pIO, _pMIO, _pPlan, _pDecode = C.POINTER(_Desc), C.POINTER(_IO), C.POINTER(_MIO), C.POINTER(_Plan), C.POINTER(_DecodeDesc)
_pDecodeOgg, _pDecodeLive = C.POINTER(_DecodeOggDesc), C.POINTER(_DecodeLiveDesc)
_pDecodeOggLive, _pDecodeOggLiveOpts = C.POINTER(_DecodeOggLiveDesc), C.POINTER(_DecodeOggLiveOpts)
_pOggWindow, _pMarks = C.POINTER(_OggWindowDesc), C.POINTER(_DecodeMarks)
_vp2 = _vp * 2
_block = [_vp, _pvp, _int, _int, _int, _int, _float]   # (ctx, pcm[ch], lW, W, nW, blocktype, ampmax_in): how every per-block call begins

# name -> (restype, argtypes) of every function of include/vorbis_amd.h the binding calls; load_library() applies it.
# tests/test_binding_cpu.py holds each entry against the header's declaration (parameter count, kind of return value).
PROTOTYPES = {
    "vamd_create_abi": (_int, [_pvp, _vp, _size, _int, _int]),
    "vamd_create_decoder": (_int, [_pvp, _vp, _size, _vp, _size, _int]),
    "vamd_ogg_read_headers": (_int, [_vp, C.c_int64, _vp, C.c_int64, _vp]),
    "vamd_quant_limit": (_int, [_vp, _int, _int, _pint, _pint, _pint]),
    "vamd_clock_probe": (_int, [_vp, _vp]),
    "vamd_config_string": (C.c_char_p, [_vp]),
    "vamd_destroy": (None, [_vp]),
    "vamd_last_error": (C.c_char_p, [_vp]),
    "vamd_set_stream": (_int, [_vp, _vp]),
    "vamd_input_status": (_int, [_vp, _plong, _plong]),
    "vamd_reserve": (_int, [_vp, _int, _long]),
    "vamd_channels": (_int, [_vp]),
    "vamd_blocksize": (_int, [_vp, _int]),
    "vamd_posts": (_int, [_vp, _int]),
    "vamd_mdct_forward_batch": (_int, [_vp, _int, _vp, _vp, _long]),
    "vamd_analyze_batch": (_int, [_vp, _pDesc, _pIO, _int]),
    "vamd_analyze_stream": (_int, [_vp, _pDesc, _pIO, _pfloat]),
    "vamd_analyze_block": (_int, _block + [_vp, _vp, _vp, _vp, _vp, _vp, _pfloat]),
    "vamd_debug_cycles": (_int, [_vp, _int, _vp]),
    "vamd_debug_survivors": (_int, [_vp, _int, _long, _vp, _vp, _vp, _pi32, _pi32]),
    "vamd_launch_record": (C.c_char_p, [_vp, _int]),
    "vamd_calib_copy": (_int, [_vp, _vp, _vp, _size]),
    "vamd_analyze_stream_mixed": (_int, [_vp, _pDesc, _pIO, _pDesc, _pIO, _vp, _long, _pfloat]),
    "vamd_analyze_streams_mixed": (_int, [_vp, _pDesc, _pIO, _pDesc, _pIO, _vp, _vp, _long, _long, _vp]),
    "vamd_envelope_search_batch": (_int, [_vp, _vp, _long, _long, _long, _long, _vp, _vp]),
    "vamd_envelope_search": (_int, [_vp, _pvp, _long, _vp, _vp]),
    "vamd_envelope_geometry": (_int, [_vp, _pint, _pint]),
    "vamd_residue_capacity": (_int, [_vp, _int]),
    "vamd_analyze_block_res": (_int, _block + [_vp] * 10),
    "vamd_analyze_batch_managed": (_int, [_vp, _pDesc, _pIO, _pMIO]),
    "vamd_analyze_batch_synth": (_int, [_vp, _pDesc, _pIO, _vp]),
    "vamd_synth_check": (_int, [_vp, _int]),
    "vamd_synth_streams": (_int, [_vp, _pPlan, _long, _long, _vp, _vp, _vp, _vp, _vp]),
    "vamd_decode_plan": (_int, [_vp, _pDecode, _vp, _vp]),
    "vamd_decode_streams": (_int, [_vp, _pDecode, _vp, _vp, _vp]),
    "vamd_decode_partial": (_int, [_vp, _int]),
    "vamd_decode_plan_marked": (_int, [_vp, _pDecode, _pMarks, _vp, _vp]),
    "vamd_decode_streams_marked": (_int, [_vp, _pDecode, _pMarks, _vp, _vp, _vp]),
    "vamd_decode_follow": (_int, [_vp, _int]),
    "vamd_decode_output": (_int, [_vp, C.POINTER(_PcmFormat)]),
    "vamd_pcm_convert": (_int, [_vp, _vp, C.c_int64, _int, C.POINTER(_PcmFormat), _vp]),
    "vamd_ogg_links": (_int, [_vp, C.c_int64, _vp, C.c_int64, _vp]),
    "vamd_ogg_read_headers_serial": (_int, [_vp, C.c_int64, C.c_uint32, _vp, C.c_int64, _vp]),
    "vamd_decode_live_create": (_int, [_vp, C.c_int64, _pvp]),
    "vamd_decode_live_destroy": (None, [_vp]),
    "vamd_decode_live_plan": (_int, [_vp, _pDecodeLive, _vp, _vp]),
    "vamd_decode_live_wrote": (_int, [_vp, _pDecodeLive, _vp, _vp, _vp]),
    "vamd_decode_ogg_plan": (_int, [_vp, _pDecodeOgg, _vp, _vp]),
    "vamd_decode_ogg": (_int, [_vp, _pDecodeOgg, _vp, _vp, _vp]),
    "vamd_decode_window_plan": (_int, [_vp, _pDecode, C.c_int64, _vp, _vp, _vp, _vp, _vp]),
    "vamd_decode_window": (_int, [_vp, _pDecode, C.c_int64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "vamd_ogg_index_create": (_int, [_vp, _pDecodeOgg, _pvp]),
    "vamd_ogg_index_destroy": (None, [_vp]),
    "vamd_ogg_index_info": (_int, [_vp, _vp, _vp, _vp]),
    "vamd_decode_ogg_window_plan": (_int, [_vp, _vp, _pOggWindow, _vp, _vp, _vp]),
    "vamd_decode_ogg_window": (_int, [_vp, _vp, _pOggWindow, _vp, _vp, _vp]),
    "vamd_decode_ogg_live_create": (_int, [_vp, C.c_int64, _pDecodeOggLiveOpts, _pvp]),
    "vamd_decode_ogg_live_destroy": (None, [_vp]),
    "vamd_decode_ogg_live_plan": (_int, [_vp, _pDecodeOggLive, _vp, _vp]),
    "vamd_decode_ogg_live_wrote": (_int, [_vp, _pDecodeOggLive, _vp, _vp, _vp]),
    "vamd_analyze_block_managed": (_int, _block + [_vp] * 9),
    "vamd_plan_streams": (_int, [_vp, _vp, _long, _long, _long, _long, _vp, _pPlan]),
    "vamd_gather_blocks": (_int, [_vp, _pPlan, _int, _vp, _long, _vp]),
    "vamd_plan_streams_whole": (_int, [_vp, _vp, _long, _long, _long, _long, _vp, _pPlan]),
    "vamd_plan_streams_whole_v": (_int, [_vp, _vp, _long, _long, _long, _long, _vp, _vp, _pPlan]),
    "vamd_feed_wrote_v": (_int, [_vp, _int, _long, _vp]),
    "vamd_feed_create": (_int, [_pvp, _vp, _size, _pint, _int, _int, _long, _long, _int]),
    "vamd_feed_create_live": (_int, [_pvp, _vp, _size, _pint, _int, _int, _long, _long, _int, _int]),
    "vamd_feed_wrote_live": (_int, [_vp, _int, _long, _vp, _vp]),
    "vamd_feed_destroy": (None, [_vp]),
    "vamd_feed_lanes": (_int, [_vp]),
    "vamd_feed_device": (_int, [_vp, _int]),
    "vamd_feed_buffer": (_int, [_vp, _pvp]),
    "vamd_feed_wrote": (_int, [_vp, _int, _long, _long]),
    "vamd_feed_packets": (_int, [_vp, _int, C.POINTER(_FeedResult)]),
    "vamd_feed_release": (_int, [_vp, _int]),
    "vamd_feed_ogg_headers": (_int, [_vp, _vp, _long, _vp, _long, _vp, _long]),
    "vamd_feed_ogg_headers_live": (_int, [_vp, _vp, _long, _vp, _long, _vp, _long]),
    "vamd_feed_ogg_serials": (_int, [_vp, _int, _vp, _long]),
    "vamd_feed_ogg_comments": (_int, [_vp, _int, _vp, _vp, _long]),
    "vamd_feed_ogg_flush": (_int, [_vp, _int, _vp, _long]),
    "vamd_feed_ogg": (_int, [_vp, _int, C.POINTER(_FeedOggResult)]),
    "vamd_feed_buffer_on": (_int, [_vp, _int, _pvp]),
    "vamd_feed_wrote_device": (_int, [_vp, _int, _long, _vp, C.POINTER(_FeedSource)]),
    "vamd_feed_wrote_live_device": (_int, [_vp, _int, _long, _vp, _vp, C.POINTER(_FeedSource)]),
    "vamd_feed_source_done": (_int, [_vp, _int, _vp, _int]),
    "vamd_feed_decoded": (_int, [_vp, _int, C.POINTER(_FeedDecodedResult)]),
    "vamd_feed_last_error": (C.c_char_p, [_vp]),
    "vamd_analyze_streams_mixed_managed": (_int, [_vp, _pDesc, _pIO, _pMIO, _pDesc, _pIO, _pMIO, _vp, _vp, _long, _long, _vp]),
    "vamd_bitrate_init_states": (_int, [_vp, _vp, _long]),
    "vamd_bitrate_walk": (_int, [_vp, _vp, _vp, _long, _vp2, _vp2, _vp, _vp2, _vp2]),
    "vamd_plan_fetch": (_int, [_vp, _pPlan, _vp2, _vp2, _vp2, _vp2, _vp, _vp]),
    "vamd_packet_capacity": (_int, [_vp, _int]),
    "vamd_submaps": (_int, [_vp, _int]),
    "vamd_residue_offset": (_int, [_vp, _int, _int]),
    "vamd_encode_block": (_int, _block + [_int, _vp, _vp, _long, _vp]),
    "vamd_encode_blocks": (_int, [_vp, _long, _pvp, _vp, _vp, _vp, _vp, _float, _int, _vp, _vp, _vp, _long, _vp, _vp]),
    "vamd_profile": (_int, [_vp, _int]),
    "vamd_stage_ms": (_int, [_vp, _pfloat, _int, _pint]),
}

# what the header declares and this binding does not call: the batcher is driven from C (integration/mapping0_vamd.c,
# tests/c/multi_gpu.c), the two queries are put to the raw library by the tests that need them
UNBOUND_SYMBOLS = ["vamd_abi_version", "vamd_device_count", "vamd_batcher_create", "vamd_batcher_create_multi", "vamd_batcher_destroy",
                   "vamd_batcher_attach", "vamd_batcher_detach", "vamd_batcher_encode_block", "vamd_batcher_last_error",
                   "vamd_batcher_stats", "vamd_batcher_context", "vamd_batcher_report"]

# every symbol include/vorbis_amd.h declares
EXPORTED_SYMBOLS = list(PROTOTYPES) + UNBOUND_SYMBOLS


def library_path():
    return os.path.join(_HERE, "libvorbis_amd.so")


_lib = None


def load_library():
    """Load libvorbis_amd.so.  Raises (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = library_path()
    if not os.path.exists(path):
        raise ImportError("vorbis_amd: %s is missing -- build it with `python -c 'import __graft_entry__ as g; "
                          "g.build()'` (hipcc --offload-arch=gfx950). There is no CPU fallback." % path)
    # The library and torch must share ONE HIP runtime (device pointers and streams cross between them): torch
    # ships its own libamdhip64, so it is loaded first and the dlopen below binds to the copy already in the
    # process.  Loaded the other way round, the system runtime and torch's both initialise and this library's
    # sees no device.
    import torch  # noqa: F401
    L = C.CDLL(path)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def default_setup_blob(name="44k_stereo_q4"):
    """A committed setup blob (vorbis_amd/data/setup_<name>.bin), produced by the reference's own
    libvorbisenc + vorbis_analysis_init through integration/vamd_pack_setup.c (tools/make_setup_blobs.py)."""
    path = os.path.join(_HERE, "data", "setup_%s.bin" % name)
    return np.fromfile(path, dtype=np.uint8)
