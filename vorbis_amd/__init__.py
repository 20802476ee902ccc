"""vorbis_amd -- MI355X-native per-block Vorbis encode analysis (libvorbis' mapping0_forward
numeric path) behind a C ABI (include/vorbis_amd.h).

This package is only plumbing: it loads libvorbis_amd.so (hand-written HIP for gfx950, built by
`__graft_entry__.build()`: one hipcc command, see there), hands it device pointers of torch tensors and
mirrors the C entry points one-to-one.  There is no CPU fallback: without the HIP library, or
without a GPU, every compute call raises.
"""
from .api import (Analyzer, LiveDecoder, LiveOggDecoder, OggIndex, Feed, decode, decode_ogg, decode_ogg_files, ogg_index, ogg_links, read_ogg_headers, pcm_convert, PCM_F32, PCM_S16, PCM_F16, PCM_BF16, STATUS_RANGE, STATUS_NONFINITE, STATUS_NOTAUDIO, STATUS_BADCODE, STATUS_TRUNCATED, STATUS_PARTIAL, STATUS_BADPAGE, STATUS_BADHEADER, FEED_S16, FEED_F32, FEED_NO_ARENA, FEED_DECODED, SRC_S16, SRC_F32, SRC_F16, SRC_BF16, DeviceSource, device_source, VamdError, load_library, library_path, default_setup_blob, LEVEL_TRANSFORM,
                  LEVEL_PSY, LEVEL_FULL, POSTS_STRIDE, BLOCKTYPE_IMPULSE, BLOCKTYPE_PADDING,
                  BLOCKTYPE_TRANSITION, BLOCKTYPE_LONG, EXPORTED_SYMBOLS, EnvelopeState, envelope_marks, packet_bytes,
                  comment_packet, comment_fields, VAMD_OK, VAMD_EFAULT, VAMD_EIMPL, VAMD_EINVAL, VAMD_EVERSION, VAMD_EDOMAIN, VAMD_ENONFINITE, VAMD_ENOTVORBIS, VAMD_EBADHEADER)

__all__ = ["Analyzer", "LiveDecoder", "LiveOggDecoder", "OggIndex", "Feed", "decode", "decode_ogg", "decode_ogg_files", "ogg_index", "ogg_links", "read_ogg_headers", "pcm_convert", "PCM_F32", "PCM_S16", "PCM_F16", "PCM_BF16", "STATUS_RANGE", "STATUS_NONFINITE", "STATUS_NOTAUDIO", "STATUS_BADCODE", "STATUS_TRUNCATED", "STATUS_PARTIAL", "STATUS_BADPAGE", "STATUS_BADHEADER", "FEED_S16", "FEED_F32", "FEED_NO_ARENA", "FEED_DECODED", "SRC_S16", "SRC_F32", "SRC_F16", "SRC_BF16", "DeviceSource", "device_source", "VamdError", "load_library", "library_path", "default_setup_blob", "LEVEL_TRANSFORM",
           "LEVEL_PSY", "LEVEL_FULL", "POSTS_STRIDE", "BLOCKTYPE_IMPULSE", "BLOCKTYPE_PADDING",
           "BLOCKTYPE_TRANSITION", "BLOCKTYPE_LONG", "EXPORTED_SYMBOLS", "EnvelopeState", "envelope_marks", "packet_bytes",
           "comment_packet", "comment_fields",
           "VAMD_OK", "VAMD_EFAULT", "VAMD_EIMPL", "VAMD_EINVAL", "VAMD_EVERSION", "VAMD_EDOMAIN", "VAMD_ENONFINITE", "VAMD_ENOTVORBIS", "VAMD_EBADHEADER"]
