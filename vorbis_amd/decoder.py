"""The decoder in Python: what an Analyzer decodes with (DecodeMixin: packets, Ogg files, windows, the output format),
the handles that belong to an Analyzer -- LiveDecoder and LiveOggDecoder for continuing streams in pieces of packets and
of Ogg bytes, OggIndex for windows of files -- and decode() / decode_ogg() / decode_ogg_files() / ogg_index() /
pcm_convert() for a caller who holds packets, files or a tensor and no context."""
import contextlib
import ctypes as C

import numpy as np

from .abi import (PCM_BF16, PCM_F16, PCM_F32, PCM_S16, STATUS_BADHEADER, STATUS_PARTIAL, VAMD_EINVAL, VAMD_OK, VamdError, _DecodeDesc,
                  _DecodeLiveDesc, _DecodeMarks, _DecodeOggDesc, _DecodeOggLiveDesc, _DecodeOggLiveOpts, _OggLink, _OggWindowDesc, _PcmFormat,
                  _vp, load_library)

_PCM_CODES = {"float32": PCM_F32, "int16": PCM_S16, "float16": PCM_F16, "bfloat16": PCM_BF16}


def _starts(lengths):
    """-> int64 [n + 1]: where each of n things laid end to end begins, and where the last ends"""
    lengths = np.asarray(lengths, np.int64) if isinstance(lengths, np.ndarray) else np.fromiter(lengths, np.int64)
    off = np.zeros(lengths.size + 1, np.int64)
    np.cumsum(lengths, out=off[1:])
    return off


def _joined(an, chunks, offsets=None, what=None):
    """`chunks` (a list of bytes-like objects) end to end as the descriptors take them -> (the uint8 array, 8 bytes of padding behind it; the
    int64 offsets [len(chunks) + 1]).  offsets: a test hook, the array as given in place of the derived one -- it must have
    its size, or ValueError(what)."""
    data = np.frombuffer(b"".join(chunks) + b"\0" * 8, np.uint8)
    if offsets is None:
        return data, _starts(len(c) for c in chunks)
    off = np.ascontiguousarray(offsets, np.int64)
    an._need(off.size == len(chunks) + 1, what)
    return data, off


def _slots_check(an, name, handle, slots, pieces):
    """what a live call asks first: a decoder that is open, a piece per slot"""
    an._need(handle.h is not None, name + ": closed")
    an._need(len(slots) == len(pieces), name + ": one piece per slot")


def _slot_arrays(an, name, slots, close):
    """a live call's slots and, per slot, whether its stream ends with this piece -> (int64, uint8), each with one spare
    entry (never an empty array: its pointer is read as non-null)"""
    slot = np.array([int(s) for s in slots] + [0], np.int64)
    closing = set(int(s) for s in close)
    an._need(closing <= set(int(s) for s in slots), name + ": a closing slot that this call does not name")
    return slot, np.array([int(s) in closing for s in slots] + [0], np.uint8)


def _analyzer():
    from .analyzer import Analyzer  # (analyzer.py imports this module: Analyzer inherits DecodeMixin)
    return Analyzer


@contextlib.contextmanager
def _context(setup_blob, device, keep_partial=None, hand_over=False):
    """An Analyzer for one call of a caller who holds no context: made, keep_partial set where given, closed behind the
    call -- or, with hand_over, only where the call fails: what it returns owns the context."""
    a = _analyzer()(setup_blob, device)
    done = False
    try:
        if keep_partial is not None:
            a.keep_partial = keep_partial
        yield a
        done = True
    finally:
        if not (done and hand_over):
            a.close()


class DecodeMixin:
    """Analyzer's decode methods (vamd_decode_*): the Analyzer gives self.L, self.h, self.torch, the checks and _live."""

    def decode_prepare(self, streams, granules=None, offset=None, stream_start=None, packet_granules=None, eos=None):
        """The descriptor of decode_streams()'s group (vamd_decode_desc) with the host arrays it points into; with
        packet_granules, also the marks (vamd_decode_marks)."""
        ns = len(streams)
        for row in streams:
            for p in row:
                self._need(isinstance(p, (bytes, bytearray, memoryview)), "decode_streams: a packet must be bytes (a missing packet is not decodable)")
        flat = [bytes(p) for row in streams for p in row]
        data, off = _joined(self, flat, offset, "decode_streams: offset must hold npackets + 1 values")
        start = _starts(len(row) for row in streams)
        if stream_start is not None:
            start = np.ascontiguousarray(stream_start, np.int64)
            self._need(start.size == ns + 1, "decode_streams: stream_start must hold nstreams + 1 values")
        gran = None
        if granules is not None:
            self._need(len(granules) == ns, "decode_streams: one granule position per stream")
            gran = np.array([-1 if g is None else int(g) for g in granules], np.int64)
        d = _DecodeDesc(ns, len(flat), _vp(data.ctypes.data), _vp(off.ctypes.data), _vp(start.ctypes.data), _vp(gran.ctypes.data) if gran is not None else None)
        marks = pg = pe = None
        self._need(eos is None or packet_granules is not None, "decode_streams: eos goes with packet_granules")
        if packet_granules is not None:
            self._need(granules is None, "decode_streams: packet_granules take the place of granules")
            self._need(len(packet_granules) == ns and all(len(g) == len(row) for g, row in zip(packet_granules, streams)),
                       "decode_streams: one granule position per packet (-1: none)")
            pg = np.array([-1 if v is None else int(v) for g in packet_granules for v in g] + [-1], np.int64)
            if eos is not None:
                self._need(len(eos) == ns and all(len(e) == len(row) for e, row in zip(eos, streams)), "decode_streams: one eos flag per packet")
                pe = np.array([1 if v else 0 for e in eos for v in e] + [0], np.uint8)
            marks = _DecodeMarks(_vp(pg.ctypes.data), _vp(pe.ctypes.data) if pe is not None else None)
        return dict(desc=d, keep=(data, off, start, gran, pg, pe), nstreams=ns, npackets=len(flat), marks=marks)

    def decode_run(self, prep, pcm=None):
        """vamd_decode_plan + vamd_decode_streams over decode_prepare()'s descriptor.  pcm: a tensor of pcm_dtype on the
        context's device to decode into (at least the planned frames x channels elements), or None: one is made.
        -> (pcm, frames, offset, status): stream s, channel c, frame k at pcm[offset[s] + c * frames[s] + k]; under
        pcm_interleaved at pcm[offset[s] + k * channels + c]"""
        args, m = (self.h, C.byref(prep["desc"])), prep.get("marks")
        if m is not None:  # (vamd_decode_plan_marked + vamd_decode_streams_marked: the marks ride behind the descriptor)
            return self._plan_run(self.L.vamd_decode_plan_marked, self.L.vamd_decode_streams_marked, args + (C.byref(m),), prep["nstreams"], pcm)
        return self._plan_run(self.L.vamd_decode_plan, self.L.vamd_decode_streams, args, prep["nstreams"], pcm)

    def _plan_run(self, plan, run, args, n, pcm, stride=None):
        """the plan call, the output tensor, the decode call -- plan(*args, frames, nblocks), then run(*args, offset, pcm,
        status) -- of every entry alike: n streams, or a window per "stream".  stride: None, or every row's channel stride
        in a pcm the caller made (row w at w * channels * stride)"""
        t = self.torch
        frames, nblocks = np.zeros(max(n, 1), np.int64), np.zeros(2, np.int64)
        self._check(plan(*args, _vp(frames.ctypes.data), _vp(nblocks.ctypes.data)))
        per = frames if stride is None else np.full(max(n, 1), int(stride), np.int64)
        ends = _starts(per[:n] * self.channels)
        out_off, total = ends[:max(n, 1)], int(ends[-1])
        if pcm is None:
            pcm = t.zeros(total + 4, dtype=self._pcm_dtype, device=self._dev())
        self._need_tensor(pcm, self._pcm_dtype, "pcm")
        self._need(pcm.numel() >= total, "pcm must hold %d elements" % total)
        status = np.zeros(max(n, 1), np.uint8)
        self._bind_stream()
        self._check(run(*args, _vp(out_off.ctypes.data), _vp(pcm.data_ptr()), _vp(status.ctypes.data)))
        return pcm, frames[:n], out_off[:n], status[:n]

    @property
    def keep_partial(self):
        """vamd_decode_partial: whether every decode call on this context decodes a packet that stops being read early to
        what libvorbis makes of it (vorbis_synthesis() returns 0: a floor that meets the end is no floor, a residue keeps
        what it has) and gives its stream its frames, with STATUS_PARTIAL in its status -- instead of flagging the stream
        STATUS_TRUNCATED, the default.  Packets libvorbis refuses flag their stream either way."""
        r = self.L.vamd_decode_partial(self.h, -1)  # (a negative value asks and changes nothing)
        self._check(min(r, 0))
        return r > 0

    @keep_partial.setter
    def keep_partial(self, keep):
        self._check(min(self.L.vamd_decode_partial(self.h, 1 if keep else 0), 0))

    @property
    def follow_links(self):
        """vamd_decode_follow: whether decode_ogg() on this context reads files as a reader does -- chained files link after
        link (each from a fresh lap, the frames end to end), pages of foreign serial numbers passed over, and every link's
        frames cut by its pages' granule positions (a start at a nonzero granule, the first page's trim) -- instead of
        flagging a second serial number STATUS_BADPAGE and cutting against a count from 0, the default.  The live, index
        and window decoders do not read it."""
        r = self.L.vamd_decode_follow(self.h, -1)  # (a negative value asks and changes nothing)
        self._check(min(r, 0))
        return r > 0

    @follow_links.setter
    def follow_links(self, on):
        self._check(min(self.L.vamd_decode_follow(self.h, 1 if on else 0), 0))

    def _pcm_format(self, dtype, interleaved, name):
        """-> the vamd_pcm_format of a torch dtype and a layout; name: the argument's, for the text"""
        code = _PCM_CODES.get(str(dtype).replace("torch.", "")) if isinstance(dtype, self.torch.dtype) else None
        self._need(code is not None, "%s must be torch.float32, int16, float16 or bfloat16 (it is %r)" % (name, dtype))
        return _PcmFormat(code, 1 if interleaved else 0)

    def _set_output(self, dtype, interleaved):
        fmt = self._pcm_format(dtype, interleaved, "pcm_dtype")
        self._check(self.L.vamd_decode_output(self.h, C.byref(fmt)))
        self._pcm_dtype, self._pcm_interleaved = dtype, bool(interleaved)

    @property
    def pcm_dtype(self):
        """vamd_decode_output: the element type of every decode call's tensors on this context -- torch.float32 (the
        default), int16 (ov_read's conversion: round to nearest even of x * 32768, clipped), float16 or bfloat16 (round to
        nearest even) -- converted in the last kernel's store.  A live decoder reads it at each write."""
        return self._pcm_dtype

    @pcm_dtype.setter
    def pcm_dtype(self, dtype):
        self._set_output(dtype, self._pcm_interleaved)

    @property
    def pcm_interleaved(self):
        """vamd_decode_output: whether every decode call on this context gives [frames, ch] tensors (crops: [n, length, ch])
        instead of [ch, frames], the default."""
        return self._pcm_interleaved

    @pcm_interleaved.setter
    def pcm_interleaved(self, on):
        self._set_output(self._pcm_dtype, on)

    def _with_output(self, dtype, interleaved, call):
        """call() under pcm_dtype / pcm_interleaved for this call alone (None: as the context stands)"""
        was = (self._pcm_dtype, self._pcm_interleaved)
        want = (was[0] if dtype is None else dtype, was[1] if interleaved is None else bool(interleaved))
        if want == was:
            return call()
        self._set_output(*want)
        try:
            return call()
        finally:
            self._set_output(*was)

    def pcm_convert(self, tensor, dtype, interleaved=False):
        """vamd_pcm_convert: a float32 [ch, frames] tensor on the context's device -> a new tensor of `dtype`, [ch, frames]
        or, interleaved, [frames, ch]: the conversion of pcm_dtype / pcm_interleaved over a signal that exists already (a
        Feed's decoded tensors)."""
        t = self.torch
        self._need_tensor(tensor, t.float32, "tensor")
        self._need(tensor.dim() == 2 and 1 <= tensor.shape[0] <= 8, "tensor must be [ch, frames] with 1 .. 8 channels")
        fmt = self._pcm_format(dtype, interleaved, "dtype")
        ch, frames = int(tensor.shape[0]), int(tensor.shape[1])
        out = t.empty((frames, ch) if interleaved else (ch, frames), dtype=dtype, device=self._dev())
        self._bind_stream()
        self._check(self.L.vamd_pcm_convert(self.h, _vp(tensor.data_ptr()), frames, ch, C.byref(fmt), _vp(out.data_ptr())))
        return out

    def _decoded_tensors(self, n, pcm, frames, out_off, status, with_status):
        out = []
        for s in range(n):
            f = 0 if int(status[s]) & ~STATUS_PARTIAL else int(frames[s])  # (a packet kept under keep_partial costs its stream nothing)
            flat = pcm[int(out_off[s]):int(out_off[s]) + self.channels * f]
            out.append(flat.view(f, self.channels) if self._pcm_interleaved else flat.view(self.channels, f))
        return (out, status.copy()) if with_status else out

    def decode_streams(self, streams, granules=None, with_status=False, offset=None, stream_start=None, packet_granules=None, eos=None,
                       dtype=None, interleaved=None):
        """vamd_decode_plan + vamd_decode_streams: audio packets of this context's setup in, PCM out -- k_unpack, k_synth and
        the lap on the GPU.  streams: a list of lists of `bytes`, one list per stream (a Feed's rows plug in as
        [[p for p, _, _, _ in row] for row in rows]); granules: per stream the last packet's granule position (None or -1:
        none), which cuts the last block's frames.  offset / stream_start: test hooks, the descriptor's arrays as given
        instead of as derived.  -> a list of float32 tensors [ch, frames] on the context's device; with_status, also the
        streams' status bytes (numpy uint8): a flagged stream -- STATUS_NOTAUDIO / _BADCODE / _TRUNCATED -- has no frames
        (STATUS_PARTIAL alone, under keep_partial, is no flag: the stream has its frames).
        packet_granules (in granules' place): per stream a list with, per packet, the granule position of the page on which
        it completes where it is the last to complete there, else -1 or None; eos: per stream a list of libogg's e_o_s per
        packet (None: each stream's last packet) -- vamd_decode_streams_marked, the frames a reader of the container keeps:
        a start at a nonzero granule, the first page's trim.
        dtype / interleaved: pcm_dtype / pcm_interleaved for this call (None: as the context stands); interleaved, the
        tensors are [frames, ch]."""
        prep = self.decode_prepare(streams, granules, offset, stream_start, packet_granules, eos)
        return self._with_output(dtype, interleaved, lambda: self._decoded_tensors(len(streams), *self.decode_run(prep), with_status))

    def live_decoder(self, max_streams):
        """vamd_decode_live_create: a LiveDecoder for up to max_streams continuing streams on this context.  Closing the
        Analyzer closes it."""
        return LiveDecoder(self, max_streams)

    def live_ogg_decoder(self, max_streams, setup_header=None, max_packet_bytes=0, max_header_bytes=0):
        """vamd_decode_ogg_live_create: a LiveOggDecoder for up to max_streams continuing Ogg Vorbis streams on this context.
        setup_header: the setup header packet every stream's third packet must equal, or None; max_packet_bytes: the longest
        audio packet that may stay open between pieces (0: the larger packet capacity); max_header_bytes: what the three
        header packets may hold together (0: 1 MiB).  Closing the Analyzer closes it."""
        return LiveOggDecoder(self, max_streams, setup_header, max_packet_bytes, max_header_bytes)

    def decode_ogg_prepare(self, files, setup_header=None, file_offset=None):
        """The descriptor of decode_ogg()'s group (vamd_decode_ogg_desc) with the host arrays it points into."""
        for f in files:
            self._need(isinstance(f, (bytes, bytearray, memoryview)), "decode_ogg: a file must be bytes")
        ns = len(files)
        data, off = _joined(self, files, file_offset, "decode_ogg: file_offset must hold nstreams + 1 values")
        hdr = np.frombuffer(bytes(setup_header), np.uint8) if setup_header is not None else None
        d = _DecodeOggDesc(ns, _vp(data.ctypes.data), _vp(off.ctypes.data), _vp(hdr.ctypes.data) if hdr is not None and hdr.size else None,
                           hdr.size if hdr is not None else 0)
        return dict(desc=d, keep=(data, off, hdr), nstreams=ns)

    def decode_ogg_run(self, prep, pcm=None):
        """vamd_decode_ogg_plan + vamd_decode_ogg over decode_ogg_prepare()'s descriptor; pcm and the result as decode_run's"""
        return self._plan_run(self.L.vamd_decode_ogg_plan, self.L.vamd_decode_ogg, (self.h, C.byref(prep["desc"])), prep["nstreams"], pcm)

    def decode_ogg(self, files, setup_header=None, with_status=False, file_offset=None, follow_links=None, dtype=None, interleaved=None):
        """vamd_decode_ogg_plan + vamd_decode_ogg: whole Ogg Vorbis files of this context's setup in, PCM out -- the page
        walk on the host, checksums and unpaging (k_ogg_depage), k_unpack, k_synth and the lap on the GPU.  files: a list of
        `bytes`, one file per stream (a Feed's Ogg output plugs in as it is); setup_header: the setup header packet every
        file's third packet must equal, or None: only its type is looked at.  file_offset: a test hook, the descriptor's
        array as given.  -> as decode_streams(); a flagged stream -- STATUS_BADPAGE / _BADHEADER or the packet decoder's
        bits -- has no frames.  follow_links: Analyzer.follow_links for this call (None: as the context stands); dtype /
        interleaved: pcm_dtype / pcm_interleaved likewise."""
        was = self.follow_links
        if follow_links is not None:
            self.follow_links = follow_links
        try:
            prep = self.decode_ogg_prepare(files, setup_header, file_offset)
            return self._with_output(dtype, interleaved, lambda: self._decoded_tensors(len(files), *self.decode_ogg_run(prep), with_status))
        finally:
            self.follow_links = was

    @staticmethod
    def _window_arrays(stream, start, count):
        """the three int64 lists of a window call, one entry per window (never empty arrays: their pointers are read as non-null)"""
        cols = [np.array([int(v) for v in col] + [0], np.int64) for col in (stream, start, count)]
        return len(stream), cols

    def decode_window(self, streams, granules, stream, start, count, with_status=False, offset=None, stream_start=None):
        """vamd_decode_window_plan + vamd_decode_window: windows of packet streams.  streams / granules (or None) as
        decode_streams() takes them; window w is frames [start[w], start[w] + count[w]) of streams[stream[w]], cut to the
        stream's end.  Only the packets of the blocks a window needs go up.  -> a list of float32 tensors [ch, frames], one
        per window, bit for bit those frames of decode_streams()'s tensors; with_status, also the windows' status bytes."""
        self._need(len(stream) == len(start) == len(count), "decode_window: stream, start and count must be as long as each other")
        prep = self.decode_prepare(streams, granules, offset, stream_start)
        nw, (ws, wa, wc) = self._window_arrays(stream, start, count)
        args = (self.h, C.byref(prep["desc"]), nw, _vp(ws.ctypes.data), _vp(wa.ctypes.data), _vp(wc.ctypes.data))
        res = self._plan_run(self.L.vamd_decode_window_plan, self.L.vamd_decode_window, args, nw, None)
        return self._decoded_tensors(nw, *res, with_status)

    def ogg_index(self, files, setup_header=None, file_offset=None):
        """vamd_ogg_index_create: one walk of whole Ogg Vorbis files, kept -> an OggIndex, whose decode() / crops() give
        windows of those files without walking or uploading them whole again.  files / setup_header / file_offset as
        decode_ogg() takes them; the index keeps the files' bytes (one joined copy).  Closing the Analyzer closes it."""
        return OggIndex(self, files, setup_header, file_offset)


class _Handle:
    """A handle of the library's that belongs to an Analyzer: listed in the Analyzer's _live, so that closing the Analyzer
    closes it; with own, the other way round -- closing it closes the Analyzer, which does not list it."""
    h = None

    def _adopt(self, analyzer, h, destroy, own=False):
        self.an, self.h, self._destroy, self._own = analyzer, h, destroy, own
        if not own:
            analyzer._live.append(self)

    def close(self):
        if getattr(self, "h", None):
            self._destroy(self.h)
            self.h = None
            if self in self.an._live:
                self.an._live.remove(self)
            if self._own:
                self.an.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class LiveDecoder(_Handle):
    """vamd_decode_live: continuing streams decoded in pieces, a stream per slot (Analyzer.live_decoder).  A stream's
    pieces laid end to end are what Analyzer.decode_streams gives for the whole stream, at any cut of its packet list."""

    def __init__(self, analyzer, max_streams):
        self.max_streams = int(max_streams)
        h = _vp()
        analyzer._check(analyzer.L.vamd_decode_live_create(analyzer.h, self.max_streams, C.byref(h)))
        self._adopt(analyzer, h, analyzer.L.vamd_decode_live_destroy)

    def prepare(self, slots, pieces, close=(), end_granules=None):
        """The descriptor of a call (vamd_decode_live_desc) with the host arrays it points into.  slots: the slots this call
        names; pieces[i]: the list of packets (bytes) of slot slots[i], in order -- it may be empty; close: the slots whose
        stream ends with this piece; end_granules: {slot: the granule position of the stream's last packet} for closing
        slots (a live feed's closing group carries it), a sequence with one value per slot of the call (None or -1: none),
        or None."""
        an = self.an
        _slots_check(an, "live decoder", self, slots, pieces)
        for row in pieces:
            for p in row:
                an._need(isinstance(p, (bytes, bytearray, memoryview)), "live decoder: a packet must be bytes")
        ns = len(slots)
        flat = [bytes(p) for row in pieces for p in row]
        data, off = _joined(an, flat)
        start = _starts(len(row) for row in pieces)
        slot, cl = _slot_arrays(an, "live decoder", slots, close)
        if end_granules is not None and not isinstance(end_granules, dict):  # (a sequence: one per slot of the call)
            an._need(len(end_granules) == ns, "live decoder: one end granule per slot of the call")
            end_granules = {int(s): g for s, g in zip(slots, end_granules)}
        end_granules = end_granules or {}
        gran = np.array([-1 if end_granules.get(int(s)) is None else int(end_granules[int(s)]) for s in slots] + [-1], np.int64)
        d = _DecodeLiveDesc(ns, len(flat), _vp(slot.ctypes.data), _vp(data.ctypes.data), _vp(off.ctypes.data), _vp(start.ctypes.data),
                            _vp(cl.ctypes.data), _vp(gran.ctypes.data))
        return dict(desc=d, keep=(data, off, start, slot, cl, gran), nstreams=ns, npackets=len(flat))

    def run(self, prep, pcm=None):
        """vamd_decode_live_plan + vamd_decode_live_wrote over prepare()'s descriptor; pcm and the result as
        Analyzer.decode_run's: (pcm, frames, offset, status)"""
        an, h = self.an, self.h
        an._need(h is not None, "live decoder: closed")
        return an._plan_run(an.L.vamd_decode_live_plan, an.L.vamd_decode_live_wrote, (h, C.byref(prep["desc"])), prep["nstreams"], pcm)

    def write(self, slots, pieces, close=(), end_granules=None, with_status=False):
        """The next piece of each named slot's stream -> a list of float32 tensors [ch, frames] on the context's device, one
        per slot of the call; a dead stream -- one that has held a flagged packet -- gives [ch, 0] until a piece closes it.
        with_status, also the status bytes (numpy uint8).  See prepare() for the arguments."""
        return self.an._decoded_tensors(len(slots), *self.run(self.prepare(slots, pieces, close, end_granules)), with_status)


class LiveOggDecoder(_Handle):
    """vamd_decode_ogg_live: continuing Ogg Vorbis streams decoded in pieces of bytes, a stream per slot
    (Analyzer.live_ogg_decoder).  The pieces may be cut at any byte; for a clean stream that ends in an end-of-stream page
    their samples laid end to end are what Analyzer.decode_ogg gives for the whole file."""

    def __init__(self, analyzer, max_streams, setup_header=None, max_packet_bytes=0, max_header_bytes=0):
        self.max_streams = int(max_streams)
        hdr = np.frombuffer(bytes(setup_header), np.uint8) if setup_header is not None else None
        opts = _DecodeOggLiveOpts(_vp(hdr.ctypes.data) if hdr is not None and hdr.size else None, hdr.size if hdr is not None else 0,
                                  int(max_packet_bytes), int(max_header_bytes))
        h = _vp()
        analyzer._check(analyzer.L.vamd_decode_ogg_live_create(analyzer.h, self.max_streams, C.byref(opts), C.byref(h)))
        self._adopt(analyzer, h, analyzer.L.vamd_decode_ogg_live_destroy)

    def prepare(self, slots, pieces, close=(), piece_offset=None):
        """The descriptor of a call (vamd_decode_ogg_live_desc) with the host arrays it points into.  slots: the slots this
        call names; pieces[i]: the next bytes of slot slots[i]'s stream -- any number of them, none included; close: the slots
        whose stream ends with this piece.  piece_offset: a test hook, the descriptor's array as given."""
        an = self.an
        _slots_check(an, "live Ogg decoder", self, slots, pieces)
        for p in pieces:
            an._need(isinstance(p, (bytes, bytearray, memoryview)), "live Ogg decoder: a piece must be bytes")
        ns = len(slots)
        data, off = _joined(an, pieces, piece_offset, "live Ogg decoder: piece_offset must hold nstreams + 1 values")
        slot, cl = _slot_arrays(an, "live Ogg decoder", slots, close)
        d = _DecodeOggLiveDesc(ns, _vp(slot.ctypes.data), _vp(data.ctypes.data), _vp(off.ctypes.data), _vp(cl.ctypes.data))
        return dict(desc=d, keep=(data, off, slot, cl), nstreams=ns)

    def run(self, prep, pcm=None):
        """vamd_decode_ogg_live_plan + vamd_decode_ogg_live_wrote over prepare()'s descriptor; pcm and the result as
        Analyzer.decode_run's: (pcm, frames, offset, status)"""
        an, h = self.an, self.h
        an._need(h is not None, "live Ogg decoder: closed")
        return an._plan_run(an.L.vamd_decode_ogg_live_plan, an.L.vamd_decode_ogg_live_wrote, (h, C.byref(prep["desc"])), prep["nstreams"], pcm)

    def write(self, slots, pieces, close=(), with_status=False):
        """The next bytes of each named slot's stream -> a list of float32 tensors [ch, frames] on the context's device, one
        per slot of the call: the samples of the audio packets those bytes complete; a dead stream -- one that has been
        flagged -- gives [ch, 0] until a piece closes it.  with_status, also the status bytes (numpy uint8)."""
        return self.an._decoded_tensors(len(slots), *self.run(self.prepare(slots, pieces, close)), with_status)


class OggIndex(_Handle):
    """vamd_ogg_index: the seek index of a group of Ogg Vorbis files (Analyzer.ogg_index).  frames[s] and status[s] are what
    a whole decode_ogg() plans for file s on the host; decode() and crops() give windows of the files, bit for bit the same
    frames of the whole decode.  Damage outside a window's own pages is not seen by that window."""

    def __init__(self, analyzer, files, setup_header=None, file_offset=None, own=False):
        prep = analyzer.decode_ogg_prepare(files, setup_header, file_offset)
        self._data, self._off = prep["keep"][0], prep["keep"][1]
        self.nstreams = prep["nstreams"]
        h = _vp()
        analyzer._check(analyzer.L.vamd_ogg_index_create(analyzer.h, C.byref(prep["desc"]), C.byref(h)))
        self._adopt(analyzer, h, analyzer.L.vamd_ogg_index_destroy, own)
        self.frames, self.status = np.zeros(max(self.nstreams, 1), np.int64), np.zeros(max(self.nstreams, 1), np.uint8)
        try:
            analyzer._check(analyzer.L.vamd_ogg_index_info(h, None, _vp(self.frames.ctypes.data), _vp(self.status.ctypes.data)))
        except Exception:  # (an index that was not made is in nobody's list)
            self.close()
            raise
        self.frames, self.status = self.frames[:self.nstreams], self.status[:self.nstreams]

    def _run(self, stream, start, count, pcm=None, stride=None, files=None, file_offset=None, row=None):
        """vamd_decode_ogg_window_plan + vamd_decode_ogg_window -> (pcm, frames, offset, status) per window.  files /
        file_offset: test hooks, other bytes than the index was made of."""
        an = self.an
        an._need(self.h is not None, "ogg index: closed")
        an._need(len(stream) == len(start) == len(count), "ogg index: stream, start and count must be as long as each other")
        data, off = self._data, self._off
        if files is not None:
            data, off = _joined(an, files)
            an._need(len(files) == self.nstreams, "ogg index: as many files as the index has")
        if file_offset is not None:
            off = np.ascontiguousarray(file_offset, np.int64)
            an._need(off.size == self.nstreams + 1, "ogg index: file_offset must hold nstreams + 1 values")
        nw, (ws, wa, wc) = an._window_arrays(stream, start, count)
        cs = np.full(max(nw, 1), int(stride), np.int64) if stride is not None else None
        d = _OggWindowDesc(nw, _vp(ws.ctypes.data), _vp(wa.ctypes.data), _vp(wc.ctypes.data), _vp(data.ctypes.data), _vp(off.ctypes.data),
                           _vp(cs.ctypes.data) if cs is not None else None)
        args = (an.h, self.h, C.byref(d))
        return an._plan_run(lambda *a: an.L.vamd_decode_ogg_window_plan(*a, None), an.L.vamd_decode_ogg_window, args, nw, pcm, stride if row is None else row)

    def decode(self, stream, start, count, with_status=False, files=None, file_offset=None, dtype=None, interleaved=None):
        """Window w = frames [start[w], start[w] + count[w]) of file stream[w], cut to the file's end -> a list of float32
        tensors [ch, frames] on the context's device, one per window; a flagged window has no frames.  with_status, also
        the windows' status bytes (numpy uint8).  dtype / interleaved: Analyzer.pcm_dtype / pcm_interleaved for this call
        (None: as the context stands); interleaved, the tensors are [frames, ch]."""
        an = self.an
        return an._with_output(dtype, interleaved, lambda: an._decoded_tensors(len(stream), *self._run(stream, start, count, files=files, file_offset=file_offset),
                                                                              with_status))

    def crops(self, stream, start, length, with_status=False, dtype=None, interleaved=None):
        """Crops of ONE length: -> (a float32 tensor [n, ch, length] on the context's device, the valid lengths (numpy int64
        [n])).  Row w holds frames [start[w], start[w] + length) of file stream[w]; behind what the file's end (or a flag)
        cut short the row is zero: the tensor is made zeroed and the kernel writes the valid part alone.  dtype /
        interleaved: Analyzer.pcm_dtype / pcm_interleaved for this call (None: as the context stands); the tensor has that
        dtype and, interleaved, is [n, length, ch]."""
        an = self.an
        return an._with_output(dtype, interleaved, lambda: self._crops(stream, start, length, with_status))

    def _crops(self, stream, start, length, with_status):
        an, t = self.an, self.an.torch
        n, length = len(stream), int(length)
        an._need(length >= 0, "crops: a negative length")
        if an.pcm_interleaved:  # (a crop is one row of length * ch elements: no stride, the windows lie length * ch apart)
            pcm = t.zeros((n, length, an.channels), dtype=an.pcm_dtype, device=an._dev())
            _, frames, _, status = self._run(stream, start, [length] * n, pcm=pcm.view(-1), row=length)
        else:
            pcm = t.zeros((n, an.channels, length), dtype=an.pcm_dtype, device=an._dev())
            _, frames, _, status = self._run(stream, start, [length] * n, pcm=pcm.view(-1), stride=length)
        flagged = (status & ~np.uint8(STATUS_PARTIAL)) != 0
        valid = np.where(flagged, 0, frames).astype(np.int64)
        for w in np.nonzero(flagged & (frames > 0))[0]:  # (a window the device flagged has no frames: its row goes back to zero)
            pcm[int(w)].zero_()
        return (pcm, valid, status.copy()) if with_status else (pcm, valid)


def ogg_index(setup_blob, files, setup_header=None, device=None, dtype=None, interleaved=None):
    """Analyzer(setup_blob).ogg_index(...) for a caller who holds files and no context: closing the index closes the context.
    dtype / interleaved: the context's pcm_dtype / pcm_interleaved, so what the index's decode() and crops() give."""
    with _context(setup_blob, device, hand_over=True) as a:
        a._set_output(a.pcm_dtype if dtype is None else dtype, bool(interleaved))
        return OggIndex(a, files, setup_header, own=True)


def decode(setup_blob, streams, granules=None, with_status=False, device=None, keep_partial=False, dtype=None, interleaved=None):
    """Analyzer(setup_blob).decode_streams(...) for a caller who holds packets and no context: the packets must come from an
    encoder of that setup.  keep_partial: Analyzer.keep_partial for the call; dtype / interleaved: Analyzer.pcm_dtype /
    pcm_interleaved for the call."""
    with _context(setup_blob, device, keep_partial) as a:
        return a.decode_streams(streams, granules, with_status, dtype=dtype, interleaved=interleaved)


def ogg_links(file):
    """vamd_ogg_links: the links of an Ogg file as Analyzer.follow_links reads them -> [(begin, end, serial)], the link
    file[begin:end] and the serial number of its Vorbis stream (its first page's where it has none).  Raises
    VamdError(VAMD_EBADHEADER) where a page does not hold against the file."""
    L = load_library()
    data = bytes(file)
    n = C.c_int64(0)
    r = L.vamd_ogg_links(data, len(data), None, 0, C.byref(n))
    rows = (_OggLink * max(int(n.value), 1))()
    if r == VAMD_EINVAL and n.value > 0:
        r = L.vamd_ogg_links(data, len(data), rows, n.value, C.byref(n))
    if r != VAMD_OK:
        raise VamdError(r, "ogg_links: a page of the file does not hold against its length")
    return [(int(v.begin), int(v.end), int(v.serial)) for v in rows[:n.value]]


def read_ogg_headers(file, serial=None):
    """vamd_ogg_read_headers: (identification, comment, setup) -- the three header packets of an Ogg file's first logical
    stream, as `bytes`; with serial, of its first stream of that serial number (vamd_ogg_read_headers_serial).  Raises
    VamdError(VAMD_EBADHEADER) where the file's pages do not hold three packets."""
    L = load_library()
    data = bytes(file)
    lens = (C.c_int64 * 3)()
    out = C.create_string_buffer(max(len(data), 1))  # (the packets are part of the file: never longer)
    if serial is None:
        r = L.vamd_ogg_read_headers(data, len(data), out, len(data), lens)
    else:
        r = L.vamd_ogg_read_headers_serial(data, len(data), int(serial), out, len(data), lens)
    if r != VAMD_OK:
        raise VamdError(r, "read_ogg_headers: the file's pages do not hold three header packets")
    a, b, c = (int(v) for v in lens)
    return out.raw[:a], out.raw[a:a + b], out.raw[a + b:a + b + c]


def pcm_convert(tensor, dtype, interleaved=False):
    """vamd_pcm_convert for a caller who holds a float32 [ch, frames] tensor on a GPU and no context (a context of the
    default setup is made for the call: any context converts alike) -> a tensor of `dtype`, [ch, frames] or [frames, ch]."""
    from .abi import default_setup_blob
    with _context(default_setup_blob(), tensor.device.index if hasattr(tensor, "device") and tensor.device.index is not None else None) as a:
        return a.pcm_convert(tensor, dtype, interleaved)


def _decode_ogg_linked(files, with_status, device, keep_partial, links, dtype=None, interleaved=None):
    """decode_ogg_files(follow_links=True): the files split at their link boundaries (ogg_links; a file whose pages do not
    hold stays whole and is flagged by the decode), the links decoded as files -- grouped by setup, one context each, the
    policy on -- and put back together per file."""
    import torch
    parts, owner, serials = [], [], []
    for i, f in enumerate(files):
        f = bytes(f)
        try:
            spans = ogg_links(f) or [(0, len(f), None)]
        except VamdError:
            spans = [(0, len(f), None)]
        for a, b, serial in spans:
            parts.append(f[a:b]), owner.append(i), serials.append(serial)
    pcm, st = _decode_ogg_grouped(parts, device, keep_partial, serials, dtype, interleaved)
    cdim = 1 if interleaved else 0  # (the tensors' channel dimension)
    out, status = [], np.zeros(len(files), np.uint8)
    for i in range(len(files)):
        mine = [k for k, o in enumerate(owner) if o == i]
        for k in mine:
            status[i] |= st[k]
        flagged = bool(int(status[i]) & ~STATUS_PARTIAL)
        if links:
            out.append([pcm[k] for k in mine])
        elif flagged:
            out.append(torch.zeros((0, 0), dtype=dtype or torch.float32, device=pcm[mine[0]].device))
        else:
            if len({int(pcm[k].shape[cdim]) for k in mine}) != 1:
                raise ValueError("decode_ogg_files: file %d has links of differing channel counts; links=True gives a tensor per link" % i)
            out.append(pcm[mine[0]] if len(mine) == 1 else torch.cat([pcm[k] for k in mine], dim=1 - cdim))
    return (out, status) if with_status else out


def _decode_ogg_grouped(files, device, keep_partial, serials=None, dtype=None, interleaved=None):
    """decode_ogg_files' work: the files (or, with serials -- per file the serial number of its Vorbis stream, None: its
    first stream's -- the links, read under Analyzer.follow_links) grouped by setup, a context per group -> (tensors, status)"""
    import torch
    groups, out, status = {}, [None] * len(files), np.zeros(len(files), np.uint8)
    for i, f in enumerate(files):
        try:
            ident, _, setup = read_ogg_headers(f, serials[i] if serials else None)
            groups.setdefault((ident[7:16] + ident[28:29], setup), (ident, []))[1].append(i)  # version, channels, rate; the block sizes
        except VamdError:
            status[i] = STATUS_BADHEADER
    for (_, setup), (ident, members) in groups.items():
        try:
            a = _analyzer().from_headers(ident, setup, device)
        except VamdError:
            status[members] = STATUS_BADHEADER
            continue
        try:
            a.keep_partial = keep_partial
            pcm, st = a.decode_ogg([files[i] for i in members], with_status=True, follow_links=serials is not None, dtype=dtype, interleaved=interleaved)
            for i, p, v in zip(members, pcm, st):
                out[i], status[i] = p.clone(), v
        finally:
            a.close()
    dev = torch.device("cuda", torch.cuda.current_device() if device is None else int(device))
    out = [torch.zeros((0, 0), dtype=dtype or torch.float32, device=dev) if p is None else p for p in out]
    return out, status


def decode_ogg_files(files, with_status=False, device=None, keep_partial=False, follow_links=False, links=False, dtype=None, interleaved=None):
    """Ogg Vorbis files of ANY covered setups in, PCM out: no blob and no settings.  Each file's headers are read
    (read_ogg_headers); the files are grouped by (identification fields, setup header bytes); one decode-only context is
    made per distinct setup (Analyzer.from_headers) and decodes its group in one decode_ogg call.  -> a list of float32
    tensors [ch, frames] in the caller's order; with_status, also the status bytes.  A file whose headers are rejected or
    refused gets a [0, 0] tensor and STATUS_BADHEADER: it costs only itself.  keep_partial: Analyzer.keep_partial for every context.
    follow_links: files are read as a reader reads them (Analyzer.follow_links): they are split at their link boundaries
    and the LINKS are grouped by setup, so a chained file may change its setup from link to link; the result per file is
    its links' signal end to end where they share a channel count (else ValueError: ask for links=True), a flagged link
    flags its file.  links=True (with follow_links): per file a list of tensors, one per link.
    dtype / interleaved: Analyzer.pcm_dtype / pcm_interleaved for every context: tensors of that dtype, interleaved [frames, ch]."""
    if follow_links:
        return _decode_ogg_linked(files, with_status, device, keep_partial, links, dtype, interleaved)
    if links:
        raise ValueError("decode_ogg_files: links=True goes with follow_links=True")
    out, status = _decode_ogg_grouped(files, device, keep_partial, None, dtype, interleaved)
    return (out, status) if with_status else out


def decode_ogg(setup_blob, files, setup_header=None, with_status=False, device=None, keep_partial=False, follow_links=False, dtype=None,
               interleaved=None):
    """Analyzer(setup_blob).decode_ogg(...) for a caller who holds files and no context: the files must come from an
    encoder of that setup.  keep_partial / follow_links / dtype / interleaved: Analyzer.keep_partial / .follow_links /
    .pcm_dtype / .pcm_interleaved for the call."""
    with _context(setup_blob, device, keep_partial) as a:
        return a.decode_ogg(files, setup_header, with_status, follow_links=follow_links, dtype=dtype, interleaved=interleaved)
