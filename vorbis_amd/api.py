"""The binding under its first name: everything lives in a module of its own topic -- abi.py (the ctypes mirror of
include/vorbis_amd.h and the loader), packets.py (packet and comment helpers), analyzer.py (Analyzer, LiveDecoder, LiveOggDecoder, OggIndex, decode, decode_ogg, decode_ogg_files, ogg_index, ogg_links, read_ogg_headers) and
feed.py (Feed, DeviceSource, device_source) -- and is importable from here as before."""
from .abi import (PCM_BF16, PCM_F16, PCM_F32, PCM_S16,  # noqa: F401
                  ABI_VERSION, BLOCKTYPE_IMPULSE, BLOCKTYPE_LONG, BLOCKTYPE_PADDING, BLOCKTYPE_TRANSITION, EXPORTED_SYMBOLS,  # noqa: F401
                  FEED_DECODED, FEED_F32, FEED_NO_ARENA, FEED_S16, LEVEL_FULL, LEVEL_PSY, LEVEL_TRANSFORM, MAX_CH, PACKETBLOBS,
                  POSTS_STRIDE, PROTOTYPES, QUANT_LIMIT_INT, QUANT_LIMIT_SQUARE, RES_CLASS_STRIDE, SRC_BF16, SRC_F16, SRC_F32, SRC_S16,
                  STATUS_BADCODE, STATUS_BADHEADER, STATUS_BADPAGE, STATUS_NONFINITE, STATUS_NOTAUDIO, STATUS_PARTIAL, STATUS_RANGE, STATUS_TRUNCATED, UNBOUND_SYMBOLS, VAMD_EDOMAIN,
                  VAMD_EBADHEADER, VAMD_EFAULT, VAMD_EIMPL, VAMD_EINVAL, VAMD_ENONFINITE, VAMD_ENOTVORBIS, VAMD_EVERSION, VAMD_OK, EnvelopeState, VamdError,
                  default_setup_blob, library_path, load_library)
from .analyzer import (Analyzer, LiveDecoder, LiveOggDecoder, OggIndex, decode, decode_ogg, decode_ogg_files, ogg_index, ogg_links,  # noqa: F401
                       pcm_convert, read_ogg_headers)
from .feed import DeviceSource, Feed, device_source  # noqa: F401
from .packets import comment_fields, comment_packet, envelope_marks, packet_bytes  # noqa: F401
