"""vamd_feed in Python: the Feed with its primitive calls (one per C entry point), the synchronous helpers that drive one
group through them, and DeviceSource / device_source for groups that are already in device memory."""
import ctypes as C

import numpy as np

from .abi import (FEED_DECODED, FEED_NO_ARENA, FEED_S16, SRC_BF16, SRC_F16, SRC_F32, SRC_S16, VamdError, _FeedDecodedResult,
                  _FeedOggResult, _FeedResult, _FeedSource, _vp, load_library)


class _DeviceFloats:
    """`count` floats of device memory at `ptr`, for torch.as_tensor (the CUDA array interface: a view, no copy)"""

    def __init__(self, ptr, count):
        self.__cuda_array_interface__ = {"shape": (int(count),), "typestr": "<f4", "data": (int(ptr), False), "version": 2}


def _view(p, ct, n, copy):
    """`n` elements of C type `ct` at pointer `p` as a numpy array: a view of that memory, or a copy of it."""
    if n == 0:
        return np.zeros(0, np.dtype(ct))
    a = np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,))
    return a.copy() if copy else a


class DeviceSource:
    """A device-fed group's source spelled out, as vamd_feed_source has it: base = one device pointer per stream (ints; 0
    where the stream has no frames), dtype = SRC_*, the strides in elements.  keep: whatever owns the memory."""

    def __init__(self, base, dtype, channel_stride, frame_stride, keep=None):
        self.base, self.dtype, self.channel_stride, self.frame_stride, self.keep = list(base), dtype, channel_stride, frame_stride, keep


def _torch_src_dtype(t):
    import torch
    table = {torch.int16: SRC_S16, torch.float32: SRC_F32, torch.float16: SRC_F16, torch.bfloat16: SRC_BF16}
    if t.dtype not in table:
        raise ValueError("a device-fed group takes int16, float32, float16 or bfloat16 tensors, not %s" % t.dtype)
    return table[t.dtype]


def device_source(source, frames=None, layout="scf"):
    """-> (DeviceSource, frames [nstreams] int64, device index or None) of what Feed.wrote_device takes: one tensor
    (streams, channels, frames) -- (streams, frames, channels) with layout="sfc" -- or a list of per-stream tensors (channels,
    frames_s) -- (frames_s, channels) with "sfc".  The strides are the tensors' own: nothing is made contiguous, nothing copied."""
    if isinstance(source, DeviceSource):
        if frames is None:
            raise ValueError("a DeviceSource needs frames")
        return source, np.ascontiguousarray(frames, dtype=np.int64).reshape(-1), None
    if layout not in ("scf", "sfc"):
        raise ValueError("layout is 'scf' or 'sfc'")
    ci, fi = (0, 1) if layout == "scf" else (1, 0)
    if isinstance(source, (list, tuple)):
        if not source:
            raise ValueError("no streams")
        for t in source:
            if t.dim() != 2:
                raise ValueError("a list holds one 2-d tensor per stream")
        # (the stride of an axis of length 1 is never used, and a stream without frames reads nothing: its strides are no one's)
        sig = lambda t: (t.dtype, t.device, t.shape[ci], t.stride(ci) if t.shape[ci] > 1 and t.shape[fi] else None,
                         t.stride(fi) if t.shape[fi] > 1 else None)
        first = next((t for t in source if t.shape[fi] > 1), next((t for t in source if t.shape[fi]), source[0]))
        for t in source:
            a, b = sig(t), sig(first)
            if a[:3] != b[:3] or any(x is not None and y is not None and x != y for x, y in zip(a[3:], b[3:])):
                raise ValueError("the tensors of a device-fed group must agree in dtype, device, channels and strides")
        have = np.array([t.shape[fi] for t in source], np.int64)
        base = [t.data_ptr() if t.shape[fi] else 0 for t in source]
        t0 = first
    else:
        t0 = source
        if t0.dim() != 3:
            raise ValueError("a tensor source is (streams, channels, frames), or (streams, frames, channels) with layout='sfc'")
        ci, fi = ci + 1, fi + 1
        have = np.full(t0.shape[0], t0.shape[fi], np.int64)
        base = [t0.data_ptr() + s * t0.stride(0) * t0.element_size() for s in range(t0.shape[0])]
    if not t0.is_cuda:
        raise ValueError("a device-fed group reads device memory: the tensors must be on the GPU (a host array goes through buffer() / wrote())")
    fr = have if frames is None else np.ascontiguousarray(frames, dtype=np.int64).reshape(-1)
    if fr.shape != have.shape or (fr > have).any() or (fr < 0).any():
        raise ValueError("frames must hold one length per stream, none longer than its tensor")
    src = DeviceSource(base, _torch_src_dtype(t0), t0.stride(ci) if t0.shape[ci] > 1 and t0.shape[fi] else 0, t0.stride(fi) if t0.shape[fi] > 1 else 1,
                       keep=source)
    return src, fr, t0.device.index


class Feed:
    """vamd_feed: whole streams from HOST memory in (interleaved int16 / float32), finished packets back to host
    memory, over one or several GPUs (include/vorbis_amd.h, "the host-fed farm").  The call sequence is libvorbis'
    own, for a group of streams: buffer() -> fill -> wrote() -> packets() -> release().

    write_frames (an int): a LIVE feed (vamd_feed_create_live) -- every lane keeps max_streams continuing streams, fed in
    pieces of at most max_frames frames: buffer() -> fill -> wrote_live() -> packets() -> release(); its packets are the
    reference's when it gets the samples write_frames at a time.

    ogg_headers = (identification, comment, setup), the packets vorbis_analysis_headerout() gives for the blob's encoder
    setup: an OGG feed (vamd_feed_ogg_headers) -- besides packets(), ogg() returns one complete Ogg Vorbis I file per
    stream, framed on the device: buffer() -> fill -> [ogg_serials()] [ogg_comments()] -> wrote() -> ogg() / packets() ->
    release().  The comment packet given here is the feed's own; ogg_comments() gives a group's streams their own.
    With write_frames: a LIVE OGG feed (vamd_feed_ogg_headers_live) -- ogg() returns per stream the next bytes of its file,
    the pages it completed in the group; a stream's pieces laid end to end are its file (encode_live_ogg).

    DEVICE-fed groups (vamd_feed_wrote_device): streams that are already in device memory, as torch tensors of int16 /
    float32 / float16 / bfloat16 with any strides, read where they lie: buffer() or buffer_on(device) -> wrote_device() /
    wrote_live_device() in wrote()'s / wrote_live()'s place -> [source_done()] -> packets() / ogg() -> release(); the
    synchronous helpers are encode_tensors, encode_ogg_tensors, encode_live_tensors and encode_live_ogg_tensors.
    fmt | FEED_NO_ARENA: a feed for such groups only, without pinned input arenas.

    decoded=True (vamd_feed_create with VAMD_FEED_DECODED): every group also leaves, in device memory, the signal a listener
    gets back from its packets -- bit for bit libvorbis' decoder's, aligned sample for sample with the input: decoded(slot)
    beside packets(slot); roundtrip_tensors for device tensors in, (packets, decoded tensors) out."""

    def __init__(self, setup_blob, devices=None, lanes_per_device=2, max_streams=256, max_frames=131072, fmt=FEED_S16,
                 write_frames=None, ogg_headers=None, decoded=False):
        if decoded:
            fmt |= FEED_DECODED
        self.L = load_library()
        blob = np.ascontiguousarray(setup_blob, dtype=np.uint8)
        devs = list(devices) if devices else []
        arr = (C.c_int * max(1, len(devs)))(*devs)
        h = _vp()
        if write_frames is None:
            r = self.L.vamd_feed_create(C.byref(h), _vp(blob.ctypes.data), blob.size, arr if devs else None, len(devs), lanes_per_device,
                                        max_streams, max_frames, fmt)
        else:
            r = self.L.vamd_feed_create_live(C.byref(h), _vp(blob.ctypes.data), blob.size, arr if devs else None, len(devs),
                                             lanes_per_device, max_streams, max_frames, fmt, int(write_frames))
        self.write_frames = write_frames
        if r:
            why = self.L.vamd_feed_last_error(None).decode()
            raise VamdError(r, "vamd_feed_create failed: " + (why or "setup without GPU-assembled packets, bad arguments, or a HIP failure"))
        self.h = h
        self.no_arena = bool(fmt & FEED_NO_ARENA)
        self.is_decoded = bool(fmt & FEED_DECODED)
        fmt &= ~(FEED_NO_ARENA | FEED_DECODED)
        self._held = {}   # slot -> the tensors of its device-fed group, kept alive until the group has read them
        self.max_streams, self.max_frames, self.fmt = max_streams, max_frames, fmt
        self.dtype = np.int16 if fmt == FEED_S16 else np.float32
        self.lanes = self.L.vamd_feed_lanes(self.h)
        if ogg_headers is not None:
            try:
                (self.ogg_headers if write_frames is None else self.ogg_headers_live)(*ogg_headers)
            except Exception:
                self.close()
                raise

    def close(self):
        if getattr(self, "h", None):
            self.L.vamd_feed_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, r):
        if r < 0:
            raise VamdError(r, self.L.vamd_feed_last_error(self.h).decode())
        return r

    # ---- the primitive calls: one per entry point of the C ABI ----
    def _ogg_headers(self, call, ident, comment, setup):
        pk = [bytes(p) for p in (ident, comment, setup)]
        self._check(call(self.h, pk[0], len(pk[0]), pk[1], len(pk[1]), pk[2], len(pk[2])))

    def ogg_headers(self, ident, comment, setup):
        """Makes the feed an Ogg feed; before the first buffer()."""
        self._ogg_headers(self.L.vamd_feed_ogg_headers, ident, comment, setup)

    def ogg_headers_live(self, ident, comment, setup):
        """Makes a live feed a live Ogg feed (files in pieces); before the first buffer()."""
        self._ogg_headers(self.L.vamd_feed_ogg_headers_live, ident, comment, setup)

    def ogg_serials(self, slot, serials):
        """The stream serial numbers of the group being filled in `slot` (between buffer() and wrote()).  A live feed: of
        the streams that begin with this group; an open stream keeps its own."""
        a = np.ascontiguousarray(serials, dtype=np.uint32).reshape(-1)
        self._check(self.L.vamd_feed_ogg_serials(self.h, slot, _vp(a.ctypes.data), a.size))

    def ogg_comments(self, slot, comments):
        """The comment headers of the group being filled in `slot` (between buffer() and wrote()): comments[s] the packet
        (bytes, e.g. comment_packet(...)) of stream s, or None for the feed's own; streams beyond the list keep the feed's.
        For this group only.  A live feed: of the streams that begin with this group."""
        pk = [None if c is None else bytes(c) for c in comments]
        n = len(pk)
        ptr = (C.c_char_p * max(n, 1))(*pk)
        size = (C.c_long * max(n, 1))(*[0 if c is None else len(c) for c in pk])
        self._check(self.L.vamd_feed_ogg_comments(self.h, slot, C.cast(ptr, _vp), C.cast(size, _vp), n))

    def ogg_flush(self, slot, flags=True):
        """A live Ogg feed: the streams of the group being filled in `slot` (between buffer() and wrote_live()) whose open
        page leaves with this group.  flags: a sequence, stream s is flushed where flags[s] is true and streams beyond it
        are not; True: every stream the feed can hold; False or None: none.  For this group only."""
        if flags is True:
            self._check(self.L.vamd_feed_ogg_flush(self.h, slot, None, self.max_streams))
            return
        a = np.ascontiguousarray([] if flags is None or flags is False else [bool(v) for v in flags], dtype=np.uint8).reshape(-1)
        self._check(self.L.vamd_feed_ogg_flush(self.h, slot, _vp(a.ctypes.data) if a.size else None, a.size))

    def device(self, slot):
        return self._check(self.L.vamd_feed_device(self.h, slot))

    def buffer(self, channels=None):
        """-> (slot, array [max_streams * max_frames * channels] of the feed's sample type over the lane's pinned input arena;
        None on a FEED_NO_ARENA feed, and where channels is None: a slot for a device-fed group)"""
        p = _vp()
        return self._arena(self._check(self.L.vamd_feed_buffer(self.h, C.byref(p))), p, channels)

    def buffer_on(self, device, channels=None):
        """buffer() restricted to the lanes on `device` (an ordinal): waits for one of those."""
        p = _vp()
        return self._arena(self._check(self.L.vamd_feed_buffer_on(self.h, int(device), C.byref(p))), p, channels)

    def _arena(self, slot, p, channels):
        if not p.value or channels is None:
            return slot, None
        n = self.max_streams * self.max_frames * channels
        ct = C.c_int16 if self.fmt == FEED_S16 else C.c_float
        arr = np.ctypeslib.as_array(C.cast(p, C.POINTER(ct)), shape=(n,))
        return slot, arr

    def wrote(self, slot, nstreams, frames):
        """frames: one length for every stream, or one per stream (the streams then lie back to back in the arena)"""
        if np.ndim(frames) == 0:
            self._check(self.L.vamd_feed_wrote(self.h, slot, nstreams, int(frames)))
        else:
            fr = np.ascontiguousarray(frames, dtype=np.int64)
            if fr.shape != (nstreams,):
                raise ValueError("frames must hold one length per stream")
            self._check(self.L.vamd_feed_wrote_v(self.h, slot, nstreams, _vp(fr.ctypes.data)))

    @staticmethod
    def _close_flags(close, fr):
        """A live group's `close` as the C calls take it: -> (pointer or None, the array it points into)"""
        if close is None:
            return None, None
        cl = np.ascontiguousarray(close, dtype=np.uint8).reshape(-1)
        if cl.shape != fr.shape:
            raise ValueError("close must hold one flag per stream")
        return _vp(cl.ctypes.data), cl

    def wrote_live(self, slot, frames, close=None):
        """A live feed: frames[s] new frames of the lane's stream s (0 .. max_frames each, laid back to back in the arena);
        close[s] true ends stream s after its piece."""
        fr = np.ascontiguousarray(frames, dtype=np.int64).reshape(-1)
        cl, keep = self._close_flags(close, fr)
        self._check(self.L.vamd_feed_wrote_live(self.h, slot, fr.size, _vp(fr.ctypes.data), cl))

    def _source(self, source, frames, layout, stream, slot):
        src, fr, dev = device_source(source, frames, layout)
        lane_dev = self.device(slot)
        if dev is not None and dev != lane_dev:
            raise ValueError("the tensors are on device %d, the slot's lane on device %d (buffer_on)" % (dev, lane_dev))
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(lane_dev).cuda_stream
        ptrs = (_vp * max(1, len(src.base)))(*[_vp(int(b) or None) for b in src.base])
        cs = _FeedSource(C.cast(ptrs, _vp), int(src.dtype), int(src.channel_stride), int(src.frame_stride), _vp(int(stream) or None))
        if fr.size != len(src.base):
            raise ValueError("frames must hold one length per stream")
        return src, fr, cs, ptrs

    def wrote_device(self, slot, source, frames=None, stream=None, layout="scf"):
        """A group from DEVICE memory (vamd_feed_wrote_device) in wrote()'s place: source as device_source() takes it -- one
        tensor, a list of per-stream tensors, or a DeviceSource -- read where it lies with its own strides; frames: one length
        per stream (default: the tensors').  stream: the HIP stream (a handle, an int) whose work so far produces the samples;
        default torch's current stream on the lane's device.  The tensors stay referenced until packets() / ogg() /
        source_done(wait=True) has returned for the slot."""
        src, fr, cs, ptrs = self._source(source, frames, layout, stream, slot)
        self._check(self.L.vamd_feed_wrote_device(self.h, slot, fr.size, _vp(fr.ctypes.data), C.byref(cs)))
        self._held[slot] = src

    def wrote_live_device(self, slot, source, frames=None, close=None, stream=None, layout="scf"):
        """A live feed's pieces from DEVICE memory (vamd_feed_wrote_live_device) in wrote_live()'s place."""
        src, fr, cs, ptrs = self._source(source, frames, layout, stream, slot)
        cl, keep = self._close_flags(close, fr)
        self._check(self.L.vamd_feed_wrote_live_device(self.h, slot, fr.size, _vp(fr.ctypes.data), cl, C.byref(cs)))
        self._held[slot] = src

    def source_done(self, slot, stream=None, wait=False):
        """Of a device-fed group: returns once its ingest is enqueued; stream (a HIP stream handle): work enqueued on it from
        now on runs behind the ingest and may overwrite the source; wait: blocks until the ingest has finished."""
        self._check(self.L.vamd_feed_source_done(self.h, slot, _vp(int(stream)) if stream else None, 1 if wait else 0))
        if wait:
            self._held.pop(slot, None)

    def packets(self, slot, copy=True):
        """Waits for the group.  -> dict: nstreams, nblocks, stream_start, offset, bits, granulepos, info (numpy views over
        the lane's pinned output arena, or copies), choice (info >> 4: the bitrate manager's candidate, 0 on a VBR setup),
        bytes, total_bytes, upload_ms, device_ms, total_ms."""
        r = _FeedResult()
        try:
            self._check(self.L.vamd_feed_packets(self.h, slot, C.byref(r)))
        finally:
            self._held.pop(slot, None)
        nb, ns = int(r.nblocks), int(r.nstreams)
        return {"nstreams": ns, "nblocks": nb, "stream_start": _view(r.stream_start, C.c_int64, ns + 1, copy),
                "offset": _view(r.offset, C.c_int64, nb, copy), "bits": _view(r.bits, C.c_int32, nb, copy),
                "granulepos": _view(r.granulepos, C.c_int64, nb, copy), "info": _view(r.info, C.c_uint8, nb, copy),
                "choice": (_view(r.info, C.c_uint8, nb, copy) >> 4).astype(np.int32),
                "bytes": _view(r.bytes, C.c_uint8, int(r.total_bytes), copy), "total_bytes": int(r.total_bytes),
                "upload_ms": r.upload_ms, "device_ms": r.device_ms, "total_ms": r.total_ms}

    def ogg(self, slot, copy=True):
        """Waits for the group.  -> dict: nstreams, stream_offset [nstreams + 1], npages, status [nstreams], bytes (a view
        over the lane's pinned file arena, or a copy), total_bytes: stream s's file is bytes[stream_offset[s]:stream_offset[s + 1]]
        (empty, with status[s] = the VAMD_STATUS_* bits, where a block of the stream has no packet)."""
        r = _FeedOggResult()
        try:
            self._check(self.L.vamd_feed_ogg(self.h, slot, C.byref(r)))
        finally:
            self._held.pop(slot, None)
        ns = int(r.nstreams)
        return {"nstreams": ns, "stream_offset": _view(r.stream_offset, C.c_int64, ns + 1, copy), "npages": _view(r.npages, C.c_int32, ns, copy),
                "status": _view(r.status, C.c_uint8, ns, copy), "bytes": _view(r.bytes, C.c_uint8, int(r.total_bytes), copy),
                "total_bytes": int(r.total_bytes)}

    def decoded(self, slot, copy=True, with_status=False):
        """Waits for the group and its decoded signal (vamd_feed_decoded).  -> per stream a float32 torch tensor (channels,
        frames) on the lane's device: what libvorbis' decoder returns for the stream's packets.  A stream that lost a packet
        has no frames.  copy=True: clones, which survive release(); else views of the lane's decoded arena, valid until
        release().  with_status: -> (tensors, status), status[s] the STATUS_* that cost stream s its signal, or 0."""
        import torch
        r = _FeedDecodedResult()
        self._check(self.L.vamd_feed_decoded(self.h, slot, C.byref(r)))
        ns, ch = int(r.nstreams), int(r.channels)
        frames = _view(r.frames, C.c_int64, ns, True)
        offset = _view(r.offset, C.c_int64, ns + 1, True)
        status = _view(r.status, C.c_uint8, ns, True)
        dev = torch.device("cuda", self.device(slot))
        total = int(r.total_floats)
        arena = torch.as_tensor(_DeviceFloats(r.pcm, total), device=dev) if total else torch.empty(0, dtype=torch.float32, device=dev)
        out = []
        for s in range(ns):
            v = arena[int(offset[s]):int(offset[s]) + ch * int(frames[s])].view(ch, int(frames[s]))
            out.append(v.clone() if copy else v)
        if copy:
            torch.cuda.synchronize(dev)  # (the clones are done before release() lets the lane's next group at the arena)
        return (out, status) if with_status else out

    def release(self, slot):
        self._check(self.L.vamd_feed_release(self.h, slot))
        self._held.pop(slot, None)

    # ---- one group, synchronously: the nine helpers, their one driver and what they share around it ----
    def _slot_for(self, source, layout):
        src, _, dev = device_source(source, [0] * len(source.base) if isinstance(source, DeviceSource) else None, layout)
        return self.buffer()[0] if dev is None else self.buffer_on(dev)[0]

    def _release_quietly(self, slot):
        try:
            self.release(slot)
        except VamdError:
            pass

    def _group(self, slot, wrote, fetch, fill=None, serials=None, comments=None, flush=None):
        """The sequence every synchronous helper is, from its slot on: fill = (arena, samples) copied in, this group's
        serials, comments and flush where given, wrote(), fetch() -- whose result is returned -- and release() whatever
        happened before it.  A VamdError of that release is dropped, so an earlier exception is the one that comes out."""
        try:
            if fill is not None:
                buf, flat = fill
                buf[:flat.size] = flat
            if serials is not None:
                self.ogg_serials(slot, serials)
            if comments is not None:
                self.ogg_comments(slot, comments)
            if flush is not None:
                self.ogg_flush(slot, flush)
            wrote()
            return fetch()
        finally:
            self._release_quietly(slot)

    def _flat_streams(self, pcm):
        """Whole streams from the host -> (nstreams, channels, frames -- one int, or one per stream --, the samples flat)"""
        if isinstance(pcm, (list, tuple)):
            parts = [np.ascontiguousarray(x, dtype=self.dtype) for x in pcm]
            ns, ch = len(parts), parts[0].shape[1]
            frames = np.array([x.shape[0] for x in parts], np.int64)
            flat = np.concatenate([x.reshape(-1) for x in parts])
        else:
            pcm = np.ascontiguousarray(pcm, dtype=self.dtype)
            ns, frames, ch = pcm.shape
            flat = pcm.reshape(-1)
        return ns, ch, frames, flat

    def _flat_pieces(self, pieces):
        """A live group's pieces from the host ([frames_s, ch] each; [frames_s] counts as mono, and a stream may have no
        frames) -> (nstreams, channels, frames per stream, the samples flat)"""
        parts = [np.ascontiguousarray(x, dtype=self.dtype) for x in pieces]
        ch = max(x.shape[1] if x.ndim == 2 else 1 for x in parts)
        parts = [x.reshape(-1, ch) for x in parts]
        frames = np.array([x.shape[0] for x in parts], np.int64)
        flat = np.concatenate([x.reshape(-1) for x in parts]) if parts else np.zeros(0, self.dtype)
        return len(parts), ch, frames, flat

    def _need_live_one_lane(self, name, fetch, device_fed):
        """What the four live helpers need of the feed; the texts name the helper and the primitive calls to use instead."""
        if self.write_frames is None:
            raise ValueError("%s needs a live feed (Feed(..., write_frames=...%s))" % (name, ", ogg_headers=..." if fetch == "ogg" else ""))
        if self.lanes != 1:
            raise ValueError("%s drives a feed with one lane; with more, use %s / %s / release"
                             % (name, "buffer_on / wrote_live_device" if device_fed else "buffer / wrote_live", fetch))

    @staticmethod
    def _rows(r, ns):
        out = []
        for s in range(ns):
            row = []
            for k in range(int(r["stream_start"][s]), int(r["stream_start"][s + 1])):
                bits = int(r["bits"][k])
                o = int(r["offset"][k])
                data = bytes(r["bytes"][o:o + (bits + 7) // 8]) if bits >= 0 else None
                row.append((data, int(r["granulepos"][k]), int(r["info"][k]) & 1, (int(r["info"][k]) >> 1) & 1))
            out.append(row)
        return out

    @staticmethod
    def _files(r, ns=None):
        """An ogg() result cut into one `bytes` per stream (copies: they survive release()), of the first `ns` streams or of
        all the result holds"""
        off = r["stream_offset"]
        ns = r["nstreams"] if ns is None else ns
        return [bytes(r["bytes"][int(off[s]):int(off[s + 1])]) for s in range(ns)]

    def encode(self, pcm):
        """One group, synchronously: pcm [nstreams, frames, ch] of the feed's sample type (host), or a list of [frames_s, ch]
        arrays of unequal length.  -> per stream a list of (packet bytes, granulepos, W, e_o_s)."""
        ns, ch, frames, flat = self._flat_streams(pcm)
        slot, buf = self.buffer(ch)
        r = self._group(slot, lambda: self.wrote(slot, ns, frames), lambda: self.packets(slot), fill=(buf, flat))
        return self._rows(r, ns)

    def encode_ogg(self, pcm, serials=None, comments=None):
        """One group of an Ogg feed, synchronously: pcm as encode() takes it; serials and comments (optional) as ogg_serials
        and ogg_comments take them.  -> list[bytes], one complete Ogg Vorbis file per stream (b"" for a stream without
        one: see ogg())."""
        ns, ch, frames, flat = self._flat_streams(pcm)
        slot, buf = self.buffer(ch)
        return self._group(slot, lambda: self.wrote(slot, ns, frames), lambda: self._files(self.ogg(slot, copy=False), ns),
                           fill=(buf, flat), serials=serials, comments=comments)

    def encode_live(self, pieces, close=None):
        """One group of a live feed with ONE lane, synchronously: pieces = the next [frames_s, ch] samples of streams
        0 .. len(pieces)-1 (the feed's sample type; 0 frames allowed); close[s] true ends stream s after its piece.
        -> per stream the packets its blocks the samples so far determine, as (bytes, granulepos, W, e_o_s) tuples."""
        self._need_live_one_lane("encode_live", "packets", False)
        ns, ch, frames, flat = self._flat_pieces(pieces)
        slot, buf = self.buffer(ch)
        r = self._group(slot, lambda: self.wrote_live(slot, frames, close), lambda: self.packets(slot), fill=(buf, flat))
        return self._rows(r, ns)

    def encode_live_ogg(self, pieces, close=None, serials=None, comments=None, flush=None):
        """One group of a live Ogg feed with ONE lane, synchronously: pieces and close as encode_live takes them; serials,
        comments and flush (optional; this group's) as ogg_serials, ogg_comments and ogg_flush take them.  -> per stream the
        next bytes of its Ogg file: the pages it completed in this group, with a flush its open page too (b"" where none,
        or where the stream has lost a packet: see ogg())."""
        self._need_live_one_lane("encode_live_ogg", "ogg", False)
        ns, ch, frames, flat = self._flat_pieces(pieces)
        slot, buf = self.buffer(ch)
        return self._group(slot, lambda: self.wrote_live(slot, frames, close), lambda: self._files(self.ogg(slot, copy=False), ns),
                           fill=(buf, flat), serials=serials, comments=comments, flush=flush)

    def encode_tensors(self, source, frames=None, stream=None, layout="scf"):
        """encode() of streams that are in DEVICE memory: source, frames, stream and layout as wrote_device takes them.
        -> per stream a list of (packet bytes, granulepos, W, e_o_s)."""
        slot = self._slot_for(source, layout)
        r = self._group(slot, lambda: self.wrote_device(slot, source, frames, stream, layout), lambda: self.packets(slot))
        return self._rows(r, r["nstreams"])

    def roundtrip_tensors(self, source, frames=None, stream=None, layout="scf"):
        """encode_tensors() of a decoded feed: -> (packets, decoded): per stream the list of (packet bytes, granulepos, W,
        e_o_s), and per stream the decoded (channels, frames) tensor on the lane's device (decoded(), copy=True)."""
        slot = self._slot_for(source, layout)
        r, dec = self._group(slot, lambda: self.wrote_device(slot, source, frames, stream, layout),
                             lambda: (self.packets(slot), self.decoded(slot, copy=True)))
        return self._rows(r, r["nstreams"]), dec

    def encode_ogg_tensors(self, source, frames=None, serials=None, comments=None, stream=None, layout="scf"):
        """encode_ogg() of streams that are in DEVICE memory.  -> list[bytes], one Ogg Vorbis file per stream."""
        slot = self._slot_for(source, layout)
        return self._group(slot, lambda: self.wrote_device(slot, source, frames, stream, layout),
                           lambda: self._files(self.ogg(slot, copy=False)), serials=serials, comments=comments)

    def encode_live_tensors(self, source, frames=None, close=None, stream=None, layout="scf"):
        """encode_live() of pieces that are in DEVICE memory (a live feed with ONE lane): stream s of the lane gets frames[s]
        frames (default: the tensors') from source; close[s] true ends it after its piece."""
        self._need_live_one_lane("encode_live_tensors", "packets", True)
        slot = self._slot_for(source, layout)
        r = self._group(slot, lambda: self.wrote_live_device(slot, source, frames, close, stream, layout), lambda: self.packets(slot))
        return self._rows(r, r["nstreams"])

    def encode_live_ogg_tensors(self, source, frames=None, close=None, serials=None, comments=None, flush=None, stream=None, layout="scf"):
        """encode_live_ogg() of pieces that are in DEVICE memory (a live Ogg feed with ONE lane).  -> per stream the next
        bytes of its Ogg file."""
        self._need_live_one_lane("encode_live_ogg_tensors", "ogg", True)
        slot = self._slot_for(source, layout)
        return self._group(slot, lambda: self.wrote_live_device(slot, source, frames, close, stream, layout),
                           lambda: self._files(self.ogg(slot, copy=False)), serials=serials, comments=comments, flush=flush)
