"""The oracle for the CONTENTS of what the feed and the decoder handle, through ctypes on the reference build
(oracle/_ref/libvorbis_ref.so): the three header packets vorbis_analysis_headerout() gives (for a setup, or for ANY
RefEncoder, coupling switched off included), the reference decoder over a file's packets, vb->pcm as vorbis_synthesis()
leaves it for one packet, mdct_backward, and the reference's own reading of a comment header."""
import ctypes as C

import numpy as np

from tests import checker

_f32p = C.POINTER(C.c_float)


class OggPacket(C.Structure):  # ogg_packet (oracle/shim/ogg/ogg.h)
    _fields_ = [("packet", C.c_void_p), ("bytes", C.c_long), ("b_o_s", C.c_long), ("e_o_s", C.c_long),
                ("granulepos", C.c_int64), ("packetno", C.c_int64)]


def _reflib():
    from oracle import ref
    L = C.CDLL(ref.LIB_PATH)
    for name in ("vorbis_info_init", "vorbis_comment_init", "vorbis_info_clear", "vorbis_comment_clear", "vorbis_dsp_clear",
                 "vorbis_block_clear"):
        getattr(L, name).argtypes = [C.c_void_p]
    for name in ("vorbis_synthesis_init", "vorbis_block_init", "vorbis_synthesis", "vorbis_synthesis_blockin",
                 "vorbis_synthesis_pcmout", "vorbis_analysis_init"):
        getattr(L, name).argtypes = [C.c_void_p] * 2
    L.vorbis_synthesis_headerin.argtypes = [C.c_void_p] * 3
    L.vorbis_analysis_headerout.argtypes = [C.c_void_p] * 5
    return L


def encoder(name):
    """the reference encoder of a setup of checker.ENCODERS"""
    from oracle import ref
    ch, rate, q, coupled = checker.ENCODERS[name]
    return ref.RefEncoder(ch, rate, q, coupled=coupled)


def _op(p, i, granule=0, eos=0):
    """packet number i of a stream as an ogg_packet (which keeps its bytes alive)"""
    p = bytes(p)
    o = OggPacket(None, len(p), 1 if i == 0 else 0, eos, granule, i)
    o.keep = C.create_string_buffer(p, max(len(p), 1))  # (exactly as long: a read past the end is a read past the buffer)
    o.packet = C.cast(o.keep, C.c_void_p)
    return o


def _headerin(L, packets):
    """vorbis_synthesis_headerin over the packets in turn -> (the return codes, up to the first failure; vi, vc)"""
    vi, vc = C.create_string_buffer(4096), C.create_string_buffer(4096)
    L.vorbis_info_init(vi)
    L.vorbis_comment_init(vc)
    codes = []
    for i, p in enumerate(packets):
        codes.append(int(L.vorbis_synthesis_headerin(vi, vc, C.byref(_op(p, i)))))
        if codes[-1]:
            break
    return codes, vi, vc


def _headers_in(L, headers):
    """a stream's three headers, all of which the reference must accept -> (vi, vc)"""
    codes, vi, vc = _headerin(L, headers)
    assert codes == [0, 0, 0], "vorbis_synthesis_headerin(%d) = %d" % (len(codes) - 1, codes[-1])
    return vi, vc


def _headerout(L, vd, vc):
    ops = (OggPacket * 3)()
    assert L.vorbis_analysis_headerout(vd, vc, C.byref(ops[0]), C.byref(ops[1]), C.byref(ops[2])) == 0
    return [C.string_at(o.packet, o.bytes) for o in ops]


# ---- headers out ----
def reference_headers(ch, rate, q=None, managed=None, tags=(("ENCODER", "vorbis_amd feed"),)):
    """[identification, comment, setup] of vorbis_analysis_headerout() for vorbis_encode_init_vbr(ch, rate, q), or for
    vorbis_encode_init(ch, rate, *managed) with managed = (max, nominal, min)."""
    L = _reflib()
    vi, vc, vd = (C.create_string_buffer(4096) for _ in range(3))
    L.vorbis_info_init(vi)
    if managed is None:
        L.vorbis_encode_init_vbr.argtypes = [C.c_void_p, C.c_long, C.c_long, C.c_float]
        assert L.vorbis_encode_init_vbr(vi, ch, rate, q) == 0
    else:
        L.vorbis_encode_init.argtypes = [C.c_void_p] + [C.c_long] * 5
        assert L.vorbis_encode_init(vi, ch, rate, *[int(v) for v in managed]) == 0
    L.vorbis_comment_init(vc)
    L.vorbis_comment_add_tag.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p]
    for k, v in tags:
        L.vorbis_comment_add_tag(vc, k.encode(), v.encode())
    assert L.vorbis_analysis_init(vd, vi) == 0
    out = _headerout(L, vd, vc)
    L.vorbis_dsp_clear(vd)
    L.vorbis_comment_clear(vc)
    L.vorbis_info_clear(vi)
    return out


_VD_OFFSET = 56  # sizeof(vorbis_info), include/vorbis/codec.h:28-52: ref_enc (oracle/ref_harness.c) keeps its vorbis_dsp_state behind it


def encoder_headers(enc):
    """[identification, comment, setup] of vorbis_analysis_headerout() on a RefEncoder's own state"""
    L = _reflib()
    vc = C.create_string_buffer(4096)
    L.vorbis_comment_init(vc)
    out = _headerout(L, C.c_void_p(enc.h + _VD_OFFSET), vc)
    L.vorbis_comment_clear(vc)
    # (the identification header, Vorbis I 4.2.2, names the encoder it came from: a drift of ref_enc's layout would not)
    assert out[0][:7] == b"\x01vorbis" and out[0][11] == enc.channels and int.from_bytes(out[0][12:16], "little") == enc.rate
    return out


# ---- packets in ----
def reference_decode(packets, granules):
    """The reference decoder over a demuxed file: packets = the three headers, then the audio packets; granules[i] the
    granule position of audio packet i where its page gives one, else -1 (ogg_framing.page_granules); e_o_s on the last
    packet.  -> float32 [channels, frames]"""
    L = _reflib()
    vi, vc = _headers_in(L, packets[:3])
    vd, vb = C.create_string_buffer(4096), C.create_string_buffer(4096)
    L.vorbis_synthesis_read.argtypes = [C.c_void_p, C.c_int]
    assert L.vorbis_synthesis_init(vd, vi) == 0
    L.vorbis_block_init(vd, vb)
    ch = C.cast(vi, C.POINTER(C.c_int))[1]  # vorbis_info.channels
    pcm = C.POINTER(_f32p)()
    out = [[np.zeros(0, np.float32)] for _ in range(ch)]
    for i in range(3, len(packets)):
        o = _op(packets[i], i, granules[i - 3], 1 if i == len(packets) - 1 else 0)
        if L.vorbis_synthesis(vb, C.byref(o)) == 0:
            L.vorbis_synthesis_blockin(vd, vb)
        while True:
            n = L.vorbis_synthesis_pcmout(vd, C.byref(pcm))
            if n <= 0:
                break
            for c in range(ch):
                out[c].append(np.ctypeslib.as_array(pcm[c], (n,)).copy())
            L.vorbis_synthesis_read(vd, n)
    L.vorbis_block_clear(vb)
    L.vorbis_dsp_clear(vd)
    L.vorbis_comment_clear(vc)
    L.vorbis_info_clear(vi)
    return np.stack([np.concatenate(o) for o in out])


class BlockDecoder:
    """vorbis_synthesis_headerin x 3, vorbis_synthesis_init, vorbis_block_init; then vb->pcm per packet"""

    def __init__(self, headers):
        self.L = L = _reflib()
        self.vi, self.vc = _headers_in(L, headers[:3])
        self.vd, self.vb = C.create_string_buffer(4096), C.create_string_buffer(4096)
        L.vorbis_info_blocksize.argtypes = [C.c_void_p, C.c_int]
        assert L.vorbis_synthesis_init(self.vd, self.vi) == 0
        L.vorbis_block_init(self.vd, self.vb)
        self.channels = C.cast(self.vi, C.POINTER(C.c_int))[1]
        self.bs = (L.vorbis_info_blocksize(self.vi, 0), L.vorbis_info_blocksize(self.vi, 1))
        self.n, self.keep = 3, []

    def _synthesis(self, packet):
        o = _op(packet, self.n, -1)
        self.keep = self.keep[-8:] + [o]
        self.n += 1
        return self.L.vorbis_synthesis(self.vb, C.byref(o))

    def _pcm(self, W):
        """vb->pcm, the first field of vorbis_block (include/vorbis/codec.h:87-89), as [ch][blocksizes[W]]"""
        pcm = C.cast(self.vb, C.POINTER(C.POINTER(_f32p)))[0]
        return np.stack([np.ctypeslib.as_array(pcm[c], (self.bs[W],)).copy() for c in range(self.channels)])

    def block(self, packet, W):
        assert self._synthesis(packet) == 0
        return self._pcm(W)

    def synthesis(self, packet):
        """(vorbis_synthesis()'s return value, vb->pcm) for ANY packet: the block's size is the one the packet's own head
        names (two block sizes are two modes: bit 1 of the first byte); None for vb->pcm where the return value is nonzero"""
        r = self._synthesis(packet)
        if r:
            return r, None
        return 0, self._pcm((packet[0] >> 1) & 1 if self.bs[0] != self.bs[1] else 0)

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


# ---- the reference's reading of a comment header ----
class _Comment(C.Structure):  # vorbis_comment (include/vorbis/codec.h)
    _fields_ = [("user_comments", C.POINTER(C.c_void_p)), ("comment_lengths", C.POINTER(C.c_int)), ("comments", C.c_int),
                ("vendor", C.c_char_p)]


def reference_headerin(ident, candidate):
    """The reference's vorbis_synthesis_headerin, given the identification header and then `candidate` as the second
    header packet -> its return code for the candidate (0: accepted)"""
    L = _reflib()
    codes, vi, vc = _headerin(L, [ident, candidate])
    assert codes[0] == 0, "the identification header is refused: %d" % codes[0]
    L.vorbis_comment_clear(vc)
    L.vorbis_info_clear(vi)
    return codes[1]


def reference_tags(headers, keys):
    """A file's three headers through vorbis_synthesis_headerin -> (the vendor string, the number of comments, per key
    the values vorbis_comment_query returns, in order) -- bytes throughout"""
    L = _reflib()
    vi, vc = _headers_in(L, headers)
    L.vorbis_comment_query.argtypes = [C.c_void_p, C.c_char_p, C.c_int]
    L.vorbis_comment_query.restype = C.c_char_p
    L.vorbis_comment_query_count.argtypes = [C.c_void_p, C.c_char_p]
    c = C.cast(vc, C.POINTER(_Comment)).contents
    vendor, count = c.vendor, int(c.comments)
    out = {}
    for k in keys:
        kb = k.encode()
        out[k] = [L.vorbis_comment_query(vc, kb, i) for i in range(L.vorbis_comment_query_count(vc, kb))]
    L.vorbis_comment_clear(vc)
    L.vorbis_info_clear(vi)
    return vendor, count, out
