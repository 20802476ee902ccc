"""vamd_ctx in Python: the Analyzer -- batches, streams, plans, the bitrate manager's candidates, the detector, the packet
decoder for packets and for Ogg files, the LiveDecoder and the LiveOggDecoder for continuing streams in pieces of packets and
of Ogg bytes; OggIndex, windows of files -- and decode() / decode_ogg() / ogg_index() for
a caller who holds packets or files and no context."""
import ctypes as C

import numpy as np

from .abi import (ABI_VERSION, BLOCKTYPE_LONG, LEVEL_FULL, LEVEL_PSY, LEVEL_TRANSFORM, PACKETBLOBS, POSTS_STRIDE, QUANT_LIMIT_INT,
                  QUANT_LIMIT_SQUARE, RES_CLASS_STRIDE, STATUS_BADHEADER, STATUS_PARTIAL, STATUS_RANGE, VAMD_EDOMAIN, VAMD_EINVAL, VAMD_ENONFINITE, VAMD_OK, EnvelopeState, VamdError,
                  PCM_BF16, PCM_F16, PCM_F32, PCM_S16, _PcmFormat,
                  _DecodeDesc, _DecodeLiveDesc, _DecodeMarks, _OggLink, _DecodeOggDesc, _DecodeOggLiveDesc, _DecodeOggLiveOpts, _Desc, _OggWindowDesc, _IO, _MIO, _Plan, _vp, load_library)
from .packets import packet_bytes


def _spectrum(a, W):
    return (a.channels, a.blocksizes[W] // 2)


# The outputs alloc_outputs() makes (vamd_batch_io's, and vamd_analyze_batch_synth's `synth`): name -> (torch dtype, the
# shape behind the block axis as a function of the Analyzer and the size class, zeroed).  Zeroed ones are read by kernels
# that rely on it; the others are written in full.
_OUTPUTS = {
    "mdct_raw": ("float32", _spectrum, False),
    "logfft": ("float32", _spectrum, False),
    "logmdct": ("float32", _spectrum, False),
    "noise": ("float32", _spectrum, False),
    "tone": ("float32", _spectrum, False),
    "logmask": ("float32", _spectrum, False),
    "mdct": ("float32", _spectrum, False),
    "ilogmask": ("int32", _spectrum, False),
    "iwork": ("int32", _spectrum, False),
    "posts": ("int32", lambda a, W: (a.channels, POSTS_STRIDE), False),
    "post_valid": ("int32", lambda a, W: (a.channels,), False),
    "nonzero": ("int32", lambda a, W: (a.channels,), False),
    "local_ampmax": ("float32", lambda a, W: (a.channels,), False),
    "ampmax_out": ("float32", lambda a, W: (), False),
    # (modes with two submaps: one more axis, [nb, 2, ...], here and in res_count)
    "res_class": ("int32", lambda a, W: a._sub(W) + (RES_CLASS_STRIDE,), True),
    "res_entries": ("int16", lambda a, W: (a.residue_capacity(W),), True),  # uint16 payload
    "res_count": ("int32", lambda a, W: a._sub(W) + (2,), True),
    "packets": ("uint8", lambda a, W: (a.packet_capacity(W),), True),
    "packet_bits": ("int32", lambda a, W: (), True),
    # STATUS_* bits: the channel-block was outside the input domain (vorbis_amd.h)
    "status": ("uint8", lambda a, W: (a.channels,), True),
    # vb->pcm of the block's packet, un-windowed (vamd_analyze_batch_synth)
    "synth": ("float32", lambda a, W: (a.channels, a.blocksizes[W]), False),
}


class Analyzer:
    """One vamd_ctx: the GPU-side counterpart of a vorbis_dsp_state's lookups."""

    def __init__(self, setup_blob, device=None, _headers=None):
        import torch
        self.torch = torch
        self.L = load_library()
        if not torch.cuda.is_available():
            raise RuntimeError("vorbis_amd needs a ROCm GPU (torch.cuda.is_available() is False); no CPU fallback")
        self.device = torch.cuda.current_device() if device is None else int(device)
        h = _vp()
        self.decode_only = _headers is not None
        if self.decode_only:
            ident, setup = (bytes(p) for p in _headers)
            r = self.L.vamd_create_decoder(C.byref(h), ident, len(ident), setup, len(setup), self.device)
            if r != VAMD_OK:
                raise VamdError(r, self.L.vamd_last_error(None).decode())
        else:
            blob = np.ascontiguousarray(np.frombuffer(bytes(setup_blob), dtype=np.uint8) if not isinstance(setup_blob, np.ndarray)
                                        else setup_blob.astype(np.uint8))
            r = self.L.vamd_create_abi(C.byref(h), blob.ctypes.data_as(_vp), blob.size, self.device, ABI_VERSION)
            if r != VAMD_OK:
                raise VamdError(r, "vamd_create failed (see stderr)")
        self.h = h
        self.channels = self.L.vamd_channels(h)
        self.blocksizes = (self.L.vamd_blocksize(h, 0), self.L.vamd_blocksize(h, 1))
        self.posts = (self.L.vamd_posts(h, 0), self.L.vamd_posts(h, 1))
        self._pcm_dtype, self._pcm_interleaved = torch.float32, False

    @classmethod
    def from_headers(cls, id_header, setup_header, device=None):
        """vamd_create_decoder: a DECODE-ONLY Analyzer out of a stream's identification and setup header packets (`bytes`;
        read_ogg_headers() gives a file's).  decode_streams, decode_ogg, decode_window, ogg_index, live_decoder and
        live_ogg_decoder work as on a blob context -- the Ogg ones hold every file's third packet to setup_header unless
        they are given another -- and the encode methods raise VamdError(VAMD_EIMPL).  Raises VamdError with
        VAMD_ENOTVORBIS / _EBADHEADER / _EVERSION for headers libvorbis refuses, VAMD_EIMPL (and the reason) for a setup
        outside the covered shape."""
        return cls(None, device, _headers=(id_header, setup_header))

    def close(self):
        if getattr(self, "h", None):
            for d in list(getattr(self, "_live", ())):  # (a live decoder does not outlive its context)
                d.close()
            self.L.vamd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, r):
        if r != VAMD_OK:
            raise VamdError(r, self.L.vamd_last_error(self.h).decode())

    def _dev(self):
        return self.torch.device("cuda", self.device)

    def _need(self, ok, what):
        """Argument checks that survive `python -O`: raw pointers go to the kernels, so a wrong dtype, device or
        stride must stop here."""
        if not ok:
            raise ValueError("vorbis_amd: " + what)

    def _need_tensor(self, v, dtype, name, numel=None, shape=None):
        t = self.torch
        self._need(t.is_tensor(v), "%s must be a torch tensor" % name)
        self._need(v.is_cuda and v.device.index == self.device, "%s must live on cuda:%d (it is on %s)" % (name, self.device, v.device))
        self._need(dtype is None or v.dtype == dtype, "%s must be %s (it is %s)" % (name, dtype, v.dtype))
        self._need(v.is_contiguous(), "%s must be contiguous" % name)
        if numel is not None:
            self._need(v.numel() == numel, "%s must hold %d elements (it holds %d)" % (name, numel, v.numel()))
        if shape is not None:
            self._need(tuple(v.shape) == tuple(shape), "%s must have shape %s (it has %s)" % (name, tuple(shape), tuple(v.shape)))

    def _need_batch(self, pcm, n):
        """pcm is a batch of blocks: cuda float32 [blocks, ch, n]"""
        self._need_tensor(pcm, self.torch.float32, "pcm")
        self._need(pcm.dim() == 3 and tuple(pcm.shape[1:]) == (self.channels, n),
                   "pcm must be [blocks, %d, %d] (it is %s)" % (self.channels, n, tuple(pcm.shape)))

    def _need_plan_streams(self, plan, streams):
        """streams has the layout the plan was made for: float32, on this device, contiguous [nstreams, ch, nsamples], 16-byte rows"""
        self._need_tensor(streams, self.torch.float32, "streams")
        self._need(streams.dim() == 3 and streams.shape[1] == self.channels and streams.shape[0] == plan.nstreams,
                   "streams must be the [%d, %d, nsamples] tensor the plan was made from" % (plan.nstreams, self.channels))
        self._need(streams.shape[2] % 4 == 0, "nsamples must be a multiple of 4 (16-byte lanes)")

    def _host_block(self, pcm, W):
        """One block from the host, pcm[ch][n] -> (the contiguous float32 array, its per-channel pointer array)"""
        ch, n = self.channels, self.blocksizes[W]
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        self._need(pcm.shape == (ch, n), "pcm must be [%d][%d] (it is %s)" % (ch, n, pcm.shape))
        return pcm, self._row_pointers(pcm)

    @staticmethod
    def _row_pointers(pcm):
        return (_vp * len(pcm))(*[_vp(row.ctypes.data) for row in pcm])

    def _fresh_states(self, ns):
        """The detector's state of `ns` streams at their start: cuda uint8 [ns, sizeof(vamd_envelope_state)] of zeros"""
        return self.torch.zeros((ns, C.sizeof(EnvelopeState)), dtype=self.torch.uint8, device=self._dev())

    def _bind_stream(self):
        s = self.torch.cuda.current_stream(self.device)
        self._check(self.L.vamd_set_stream(self.h, _vp(s.cuda_stream)))

    STAGES = ("transform", "ampmax", "noisemask", "tonemask", "floor", "couple", "residue", "pack")

    def profile(self, enable=True):
        self._bind_stream()
        self._check(self.L.vamd_profile(self.h, 1 if enable else 0))

    def stage_ms(self):
        """(dict stage -> summed ms, number of batches) since the last call; synchronises."""
        ms = (C.c_float * 8)()
        runs = C.c_int(0)
        self._check(self.L.vamd_stage_ms(self.h, ms, 8, C.byref(runs)))
        return dict(zip(self.STAGES, [float(x) for x in ms])), runs.value

    def clock_probe(self, acc):
        """vamd_clock_probe(): while `acc` (a zeroed cuda int64 tensor of 3: shader ticks, 100 MHz ticks, samples) is
        set, every large batch adds a sample of the shader clock taken beside its noise mask; None switches it off.
        After a synchronise: acc[0] / acc[1] * 0.1 = the shader clock in GHz."""
        if acc is not None:
            self._need_tensor(acc, self.torch.int64, "acc", numel=3)
        self._clk = acc   # (kept alive: the library holds the raw pointer)
        self._check(self.L.vamd_clock_probe(self.h, _vp(acc.data_ptr()) if acc is not None else None))

    def debug_cycles(self, enable=True, read=False):
        """Arm/disarm the in-kernel phase stopwatch; with read=True returns the 5x16 tick sums first."""
        out = np.zeros(80, dtype=np.uint64)
        self._check(self.L.vamd_debug_cycles(self.h, 1 if enable else 0, _vp(out.ctypes.data) if read else None))
        return out.reshape(5, 16)

    def debug_survivors(self, W, channel_blocks):
        """vamd_debug_survivors(): (seed [cb][row], surv [cb][row] uint16, nsurv [cb], lines) of the last batch of size class W."""
        row, nl = C.c_int32(), C.c_int32()
        self._check(self.L.vamd_debug_survivors(self.h, W, 0, None, None, None, C.byref(row), C.byref(nl)))
        seed = np.zeros((channel_blocks, row.value), np.float32)
        surv = np.zeros((channel_blocks, row.value), np.uint16)
        nsurv = np.zeros(channel_blocks, np.int32)
        self._check(self.L.vamd_debug_survivors(self.h, W, channel_blocks, _vp(seed.ctypes.data), _vp(surv.ctypes.data),
                                                _vp(nsurv.ctypes.data), None, None))
        return seed, surv, nsurv, nl.value

    def launch_record(self, W):
        """vamd_launch_record(): the kernels the last batch call launched for size class W, a list of words in launch order
        ("k_couple/64": the kernel, and the workgroup's threads where the launch code chooses them)."""
        return self.L.vamd_launch_record(self.h, W).decode().split()

    def calib_copy(self, dst, src):
        """vamd_calib_copy(): src -> dst (device tensors of equal byte size) with the library's named copy kernel."""
        nbytes = src.numel() * src.element_size()
        assert dst.numel() * dst.element_size() == nbytes
        self._check(self.L.vamd_calib_copy(self.h, _vp(dst.data_ptr()), _vp(src.data_ptr()), nbytes))

    def reserve(self, W, max_blocks):
        self._check(self.L.vamd_reserve(self.h, W, max_blocks))

    def input_status(self):
        """vamd_input_status(): synchronise, then (channel-blocks, detector steps) issued since the last call that
        were outside the input domain (a NaN / Inf sample, or quantised values beyond quant_limit()); resets the
        counts.  (0, 0) means every result since then is the reference's, bit for bit.  `last_input_code` keeps the
        call's verdict: VAMD_OK, VAMD_EDOMAIN (finite, beyond the integer bound) or VAMD_ENONFINITE."""
        a, b = C.c_long(0), C.c_long(0)
        r = self.L.vamd_input_status(self.h, C.byref(a), C.byref(b))
        if r not in (VAMD_OK, VAMD_EDOMAIN, VAMD_ENONFINITE):
            self._check(r)
        self.last_input_code = r
        return int(a.value), int(b.value)

    def config_string(self):
        """vamd_config_string(): the environment knobs this context read at vamd_create, as "NAME=value" words."""
        return self.L.vamd_config_string(self.h).decode()

    def quant_limit(self, W, channel=0):
        """vamd_quant_limit(): (Q, first_bin, end_bin, square_bin) -- Q bounds |quantised value| of `channel` at the bins
        [first_bin, end_bin) its residue codes, QUANT_LIMIT_SQUARE those from square_bin on (noise normalisation),
        QUANT_LIMIT_INT all of them: up to there the reference's integer arithmetic is defined."""
        a, b, sq = C.c_int(0), C.c_int(0), C.c_int(0)
        q = int(self.L.vamd_quant_limit(self.h, W, channel, C.byref(a), C.byref(b), C.byref(sq)))
        self._need(q >= 0, "vamd_quant_limit(%d, %d)" % (W, channel))
        return q, a.value, b.value, sq.value

    def beyond_quant_limit(self, W, iwork, residue=True):
        """Which channels of a block's quantised values iwork[ch][n/2] (a numpy array; e.g. the reference's own) lie
        outside the input domain's integer edge: uint8 [ch] of STATUS_RANGE / 0 -- what `status` must say of them.
        residue=False: the call ran no residue search (no res_* / packets asked for), so only the coupling stage's
        bounds were tested."""
        out = np.zeros(iwork.shape[0], np.uint8)
        for c in range(iwork.shape[0]):
            q, lo, hi, sq = self.quant_limit(W, c)
            v = np.abs(iwork[c].astype(np.int64))
            lim = np.full(v.shape, QUANT_LIMIT_INT, np.int64)
            lim[sq:] = QUANT_LIMIT_SQUARE
            if residue:
                lim[lo:hi] = np.minimum(lim[lo:hi], q)
            out[c] = STATUS_RANGE if (v > lim).any() else 0
        return out

    # mdct_forward(lookup, in, out) batched -- BASELINE config 2
    def mdct_forward(self, W, frames, out=None):
        t = self.torch
        n = self.blocksizes[W]
        self._need_tensor(frames, t.float32, "frames")
        self._need(frames.dim() >= 1 and frames.shape[-1] == n, "frames must end in %d samples" % n)
        nf = frames.numel() // n
        if out is None:
            out = t.empty(frames.shape[:-1] + (n // 2,), dtype=t.float32, device=frames.device)
        else:
            self._need_tensor(out, t.float32, "out", numel=nf * (n // 2))
        self._bind_stream()
        self._check(self.L.vamd_mdct_forward_batch(self.h, W, _vp(frames.data_ptr()), _vp(out.data_ptr()), nf))
        return out

    def _desc(self, W, nb, lW, nW, blocktype, ampmax_in, keep):
        t = self.torch
        d = _Desc()
        d.W, d.nblocks = W, nb

        def arr(v, dtype, name, uni):
            if isinstance(v, (list, tuple, np.ndarray)):   # per-block values from the host
                v = t.as_tensor(np.asarray(v), dtype=dtype).to(self._dev())
            if t.is_tensor(v):
                self._need_tensor(v, dtype, name, numel=nb)
                keep.append(v)
                setattr(d, name, _vp(v.data_ptr()))
            else:
                setattr(d, name, None)
                setattr(d, uni, v)
        arr(lW, t.int32, "lW", "uniform_lW")
        arr(nW, t.int32, "nW", "uniform_nW")
        arr(blocktype, t.int32, "blocktype", "uniform_blocktype")
        arr(ampmax_in, t.float32, "ampmax_in", "uniform_ampmax_in")
        return d

    def _plan_desc(self, plan, W):
        """The planned blocks of size class W: their lW / nW / blocktype are the plan's device arrays"""
        d = _Desc()
        d.W, d.nblocks = W, plan.nblocks[W]
        d.lW, d.nW, d.blocktype, d.ampmax_in = plan.lW[W], plan.nW[W], plan.blocktype[W], None
        return d

    def alloc_outputs(self, W, nb, want):
        """Output tensors for `want` (names from vamd_batch_io)."""
        t = self.torch
        dev = self._dev()
        o = {}
        for k in want:
            dtype, shape, zeroed = _OUTPUTS[k]
            o[k] = (t.zeros if zeroed else t.empty)((nb,) + shape(self, W), dtype=getattr(t, dtype), device=dev)
        return o

    def submaps(self, W):
        return int(self.L.vamd_submaps(self.h, W))

    def _sub(self, W):
        S = self.submaps(W)
        return (S,) if S > 1 else ()

    def residue_lists(self, W, cls, ent, cnt):
        """One block's residue rows -> (classes, entries) with the submaps one after the other, the order the
        reference classifies / emits them in.  cls / ent / cnt: numpy rows of res_class / res_entries / res_count."""
        S = self.submaps(W)
        cls, cnt = np.asarray(cls).reshape(S, RES_CLASS_STRIDE), np.asarray(cnt).reshape(S, 2)
        ent = np.asarray(ent).view(np.uint16)
        offs = [int(self.L.vamd_residue_offset(self.h, W, sm)) for sm in range(S)]
        return (np.concatenate([cls[sm, :cnt[sm, 0]] for sm in range(S)]),
                np.concatenate([ent[offs[sm]:offs[sm] + cnt[sm, 1]] for sm in range(S)]))

    def residue_capacity(self, W):
        """Row length of res_entries for size class W; 0 when the GPU does not cover this mode's residue."""
        return int(self.L.vamd_residue_capacity(self.h, W))

    def packet_capacity(self, W):
        """Bytes the longest possible packet of size class W takes; 0 when packets are not assembled on the GPU."""
        return int(self.L.vamd_packet_capacity(self.h, W))

    def _out_dtype(self, k):
        # (a field of vamd_batch_io that alloc_outputs does not make counts as int32)
        return getattr(self.torch, _OUTPUTS[k][0] if k in _OUTPUTS else "int32")

    def _io(self, pcm, outs, nb=None, synth_ok=False):
        io = _IO()
        io.pcm = _vp(pcm.data_ptr())
        nb = pcm.shape[0] if nb is None else nb
        for k, v in outs.items():
            if k == "synth":  # (not a field of vamd_batch_io: vamd_analyze_batch_synth's own argument)
                self._need(synth_ok, "the synth output is analyze()'s alone (vamd_analyze_batch_synth)")
                continue
            self._need(hasattr(io, k), "unknown output %r" % (k,))
            self._need_tensor(v, self._out_dtype(k), "outs[%r]" % k)
            self._need(v.dim() >= 1 and v.shape[0] == nb, "outs[%r] must have one row per block (%d)" % (k, nb))
            setattr(io, k, _vp(v.data_ptr()))
        if "packets" in outs:
            io.packet_stride = outs["packets"].shape[-1]
        return io

    _DEFAULT_WANT = {LEVEL_TRANSFORM: ("mdct_raw", "logfft", "logmdct", "local_ampmax"),
                     LEVEL_PSY: ("mdct_raw", "noise", "tone"),
                     LEVEL_FULL: ("mdct", "logmask", "posts", "post_valid", "iwork", "nonzero", "ampmax_out")}

    def analyze(self, pcm, W=1, lW=1, nW=1, blocktype=BLOCKTYPE_LONG, ampmax_in=-9999.0, level=LEVEL_FULL,
                want=None, outs=None):
        """vamd_analyze_batch.  pcm: cuda float32 [nblocks, ch, n].  Returns dict name -> tensor.  With "synth" among the
        outputs (level FULL): vamd_analyze_batch_synth, synth [nblocks, ch, n] = what a decoder's vorbis_synthesis() leaves
        in vb->pcm for each block's packet."""
        t = self.torch
        n = self.blocksizes[W]
        self._need(W in (0, 1), "W must be 0 or 1")
        self._need_batch(pcm, n)
        nb = pcm.shape[0]
        if outs is None:
            outs = self.alloc_outputs(W, nb, self._DEFAULT_WANT[level] if want is None else want)
        keep = []
        d = self._desc(W, nb, lW, nW, blocktype, ampmax_in, keep)
        io = self._io(pcm, outs, synth_ok=True)
        self._bind_stream()
        if "synth" in outs:
            self._need(level == LEVEL_FULL, "synth needs level FULL")
            self._need_tensor(outs["synth"], t.float32, "outs['synth']", shape=(nb, self.channels, n))
            self._check(self.L.vamd_analyze_batch_synth(self.h, C.byref(d), C.byref(io), _vp(outs["synth"].data_ptr())))
        else:
            self._check(self.L.vamd_analyze_batch(self.h, C.byref(d), C.byref(io), level))
        return outs

    def analyze_stream(self, pcm, ampmax_state, W=1, lW=1, nW=1, blocktype=BLOCKTYPE_LONG, want=None, outs=None):
        """vamd_analyze_stream.  Returns (outs, new ampmax_state)."""
        self._need_batch(pcm, self.blocksizes[W])
        nb = pcm.shape[0]
        if outs is None:
            outs = self.alloc_outputs(W, nb, self._DEFAULT_WANT[LEVEL_FULL] if want is None else want)
        keep = []
        d = self._desc(W, nb, lW, nW, blocktype, 0.0, keep)
        io = self._io(pcm, outs)
        st = C.c_float(ampmax_state)
        self._bind_stream()
        self._check(self.L.vamd_analyze_stream(self.h, C.byref(d), C.byref(io), C.byref(st)))
        return outs, st.value

    def _bucket(self, blocks, want):
        """A stream-ordered list of blocks (dicts with keys pcm (numpy [ch][n]), W, lW, nW, blocktype) sorted into its two
        size classes for the *_mixed calls.  -> (order: per block W << 30 | its index in the class, as a list and as a cuda
        int32 tensor; per class the _Desc, the _IO and the output dict; keep: what the descriptors point into)"""
        t = self.torch
        want = self._DEFAULT_WANT[LEVEL_FULL] if want is None else want
        idx = {0: [], 1: []}
        order = []
        for b in blocks:
            order.append((b["W"] << 30) | len(idx[b["W"]]))
            idx[b["W"]].append(b)
        descs, ios, outs, keep = {}, {}, {}, []
        for W in (0, 1):
            sel = idx[W]
            nb = len(sel)
            n = self.blocksizes[W]
            pcm = t.from_numpy(np.stack([b["pcm"] for b in sel]).astype(np.float32)).to(self._dev()) if nb else \
                t.empty((0, self.channels, n), device=self._dev())
            dv = lambda k: t.tensor([b[k] for b in sel], dtype=t.int32, device=self._dev()) if nb else 0  # noqa: E731
            outs[W] = self.alloc_outputs(W, nb, want)
            descs[W] = self._desc(W, nb, dv("lW"), dv("nW"), dv("blocktype"), 0.0, keep)
            ios[W] = self._io(pcm, outs[W])
            keep.append(pcm)
        od = t.tensor(order, dtype=t.int32, device=self._dev())
        return order, od, descs, ios, outs, keep

    @staticmethod
    def _unbucket(order, outs):
        """_bucket()'s outputs on the host, back in stream order: per block the dict of its rows"""
        host = {W: {k: v.cpu().numpy() for k, v in outs[W].items()} for W in (0, 1)}
        res = []
        for o in order:
            W, i = (o >> 30) & 1, o & 0x3fffffff
            res.append({k: v[i] for k, v in host[W].items()})
        return res

    def analyze_stream_mixed(self, blocks, ampmax_state, want=None):
        """vamd_analyze_stream_mixed.  `blocks`: stream-ordered list of dicts with keys pcm (numpy
        [ch][n]), W, lW, nW, blocktype.  Returns (per-block list of output dicts in stream order, state)."""
        order, od, descs, ios, outs, keep = self._bucket(blocks, want)
        st = C.c_float(ampmax_state)
        self._bind_stream()
        self._check(self.L.vamd_analyze_stream_mixed(self.h, C.byref(descs[0]), C.byref(ios[0]), C.byref(descs[1]),
                                                     C.byref(ios[1]), _vp(od.data_ptr()), len(order), C.byref(st)))
        return self._unbucket(order, outs), st.value

    def analyze_streams_mixed(self, streams, ampmax_states, want=None):
        """vamd_analyze_streams_mixed.  `streams`: list of stream-ordered block lists (dicts as for
        analyze_stream_mixed); `ampmax_states`: one float per stream.  One call for all of them.
        Returns (per stream: per-block list of output dicts, new states as numpy)."""
        t = self.torch
        start = [0]
        for blocks in streams:
            start.append(start[-1] + len(blocks))
        order, od, descs, ios, outs, keep = self._bucket([b for blocks in streams for b in blocks], want)
        sd = t.tensor(start, dtype=t.int64, device=self._dev())
        st = t.tensor(list(ampmax_states), dtype=t.float32, device=self._dev())
        self._bind_stream()
        self._check(self.L.vamd_analyze_streams_mixed(self.h, C.byref(descs[0]), C.byref(ios[0]), C.byref(descs[1]),
                                                      C.byref(ios[1]), _vp(od.data_ptr()), _vp(sd.data_ptr()), len(streams),
                                                      len(order), _vp(st.data_ptr())))
        t.cuda.synchronize()
        res = self._unbucket(order, outs)
        return [res[start[s]:start[s + 1]] for s in range(len(streams))], st.cpu().numpy()

    # ---- device-resident stream control: whole streams in, block lists out (vamd_plan_streams) ----
    def plan_streams(self, streams, states=None):
        """streams: cuda float32 [nstreams, ch, nsamples], each laid out as the encoder's own PCM buffer (first block
        centred at blocksizes[1]/2).  Returns (plan, states): the plan struct (its device arrays belong to the
        context and stay valid until the next plan_streams) and the detector states tensor."""
        t = self.torch
        self._need_tensor(streams, t.float32, "streams")
        self._need(streams.dim() == 3 and streams.shape[1] == self.channels, "streams must be [nstreams, %d, nsamples]" % self.channels)
        ns, ch, ln = streams.shape
        if states is None:
            states = self._fresh_states(ns)
        plan = _Plan()
        self._bind_stream()
        self._check(self.L.vamd_plan_streams(self.h, _vp(streams.data_ptr()), ch * ln, ln, ns, ln, _vp(states.data_ptr()),
                                             C.byref(plan)))
        return plan, states

    def plan_streams_whole(self, streams, nframes, states=None):
        """vamd_plan_streams_whole: COMPLETE streams.  streams: cuda float32 [nstreams, ch, row], every channel row laid
        out [blocksizes[1]/2 of room | nframes real samples | >= 3 * blocksizes[1] of room]; the call fills the room
        either end with the reference's LPC extrapolations (lib/block.c:417-458, :474-512), so `streams` is written.
        Returns (plan, states) as plan_streams; the plan runs to each stream's last block."""
        t = self.torch
        self._need_tensor(streams, t.float32, "streams")
        self._need(streams.dim() == 3 and streams.shape[1] == self.channels, "streams must be [nstreams, %d, row]" % self.channels)
        ns, ch, ln = streams.shape
        self._need(ln % 4 == 0 and ln >= self.blocksizes[1] // 2 + int(np.max(nframes)) + 3 * self.blocksizes[1],
                   "a channel row needs blocksizes[1]/2 + nframes + 3 * blocksizes[1] samples (a multiple of 4)")
        if states is None:
            states = self._fresh_states(ns)
        plan = _Plan()
        self._bind_stream()
        if np.ndim(nframes) == 0:
            self._check(self.L.vamd_plan_streams_whole(self.h, _vp(streams.data_ptr()), ch * ln, ln, ns, int(nframes), _vp(states.data_ptr()),
                                                       C.byref(plan)))
        else:  # streams of unequal length: every buffer laid out for the longest, zero behind a shorter stream's samples
            fr = np.ascontiguousarray(nframes, dtype=np.int64)
            self._need(fr.shape == (ns,), "nframes must hold one length per stream")
            self._check(self.L.vamd_plan_streams_whole_v(self.h, _vp(streams.data_ptr()), ch * ln, ln, ns, int(fr.max()), _vp(fr.ctypes.data),
                                                         _vp(states.data_ptr()), C.byref(plan)))
        return plan, states

    def plan_lists(self, plan):
        """A plan on the host: dict with per size class lW / nW / blocktype / src arrays, order and stream_start."""
        out = {}
        arrs = {}
        for name, dt in (("lW", np.int32), ("nW", np.int32), ("blocktype", np.int32), ("src", np.int64)):
            arrs[name] = [np.zeros(max(1, plan.nblocks[W]), dt) for W in (0, 1)]
        order = np.zeros(max(1, plan.nblocks[0] + plan.nblocks[1]), np.int32)
        start = np.zeros(plan.nstreams + 1, np.int64)
        pair = lambda k: (_vp * 2)(_vp(arrs[k][0].ctypes.data), _vp(arrs[k][1].ctypes.data))  # noqa: E731
        self._check(self.L.vamd_plan_fetch(self.h, C.byref(plan), pair("lW"), pair("nW"), pair("blocktype"), pair("src"),
                                           _vp(order.ctypes.data), _vp(start.ctypes.data)))
        for k, v in arrs.items():
            out[k] = [v[W][:plan.nblocks[W]] for W in (0, 1)]
        out["order"] = order[:plan.nblocks[0] + plan.nblocks[1]]
        out["stream_start"] = start
        return out

    def gather_blocks(self, plan, W, streams, out=None):
        """The planned blocks of size class W copied out of `streams` into [nblocks[W], ch, blocksize[W]]."""
        t = self.torch
        n = self.blocksizes[W]
        self._need_plan_streams(plan, streams)
        if out is None:
            out = t.empty((plan.nblocks[W], self.channels, n), dtype=t.float32, device=self._dev())
        else:
            self._need_tensor(out, t.float32, "out", numel=plan.nblocks[W] * self.channels * n)
        self._bind_stream()
        self._check(self.L.vamd_gather_blocks(self.h, C.byref(plan), W, _vp(streams.data_ptr()), streams.shape[2], _vp(out.data_ptr())))
        return out

    def analyze_plan(self, plan, pcm_blocks, outs, ampmax_states, streams=None):
        """vamd_analyze_streams_mixed over a plan: outs = per size class (index 0 short, 1 long) the output dict;
        ampmax_states: cuda float32 [nstreams], updated in place.  The blocks' samples: either pcm_blocks = per size class
        the gathered batch (gather_blocks), or -- pcm_blocks None -- `streams`, the very [nstreams, ch, nsamples] tensor the
        plan was made from, read in place through the plan's offsets (vamd_batch_io::pcm_src: no gathered copy)."""
        t = self.torch
        descs, ios = [], []
        if pcm_blocks is None:
            self._need_plan_streams(plan, streams)
        for W in (0, 1):
            descs.append(self._plan_desc(plan, W))
            if not plan.nblocks[W]:
                ios.append(_IO())
            elif pcm_blocks is None:
                io = self._io(streams, outs[W], nb=plan.nblocks[W])
                io.pcm_src, io.pcm_channel_stride = plan.src[W], streams.shape[2]
                ios.append(io)
            else:
                self._need_tensor(pcm_blocks[W], t.float32, "pcm_blocks[%d]" % W, numel=plan.nblocks[W] * self.channels * self.blocksizes[W])
                ios.append(self._io(pcm_blocks[W].reshape(plan.nblocks[W], self.channels, self.blocksizes[W]), outs[W]))
        self._need_tensor(ampmax_states, t.float32, "ampmax_states", numel=plan.nstreams)
        self._bind_stream()
        self._check(self.L.vamd_analyze_streams_mixed(self.h, C.byref(descs[0]), C.byref(ios[0]), C.byref(descs[1]), C.byref(ios[1]),
                                                      plan.order, plan.stream_start, plan.nstreams, plan.nblocks[0] + plan.nblocks[1],
                                                      _vp(ampmax_states.data_ptr())))

    # ---- bitrate-managed whole streams: fifteen candidates per planned block, the manager's walk ----
    def _managed_outputs(self, W, nb, dev, residue=False, packets=False):
        """The fifteen candidates' outputs of `nb` blocks of size class W.  -> (dict name -> tensor: posts [nb,15,ch,32],
        post_valid / nonzero [nb,15,ch], iwork [nb,15,ch,n/2]; with residue, res_class / res_entries / res_count; with
        packets, packets [nb,15,packet_capacity] uint8 and packet_bits [nb,15]; the vamd_managed_io that points at them)"""
        t = self.torch
        ch, n2 = self.channels, self.blocksizes[W] // 2
        mo = {"posts": t.empty((nb, PACKETBLOBS, ch, POSTS_STRIDE), dtype=t.int32, device=dev),
              "post_valid": t.empty((nb, PACKETBLOBS, ch), dtype=t.int32, device=dev),
              "iwork": t.empty((nb, PACKETBLOBS, ch, n2), dtype=t.int32, device=dev),
              "nonzero": t.empty((nb, PACKETBLOBS, ch), dtype=t.int32, device=dev)}
        if residue:
            mo["res_class"] = t.zeros((nb, PACKETBLOBS) + self._sub(W) + (RES_CLASS_STRIDE,), dtype=t.int32, device=dev)
            mo["res_entries"] = t.zeros((nb, PACKETBLOBS, self.residue_capacity(W)), dtype=t.int16, device=dev)
            mo["res_count"] = t.zeros((nb, PACKETBLOBS) + self._sub(W) + (2,), dtype=t.int32, device=dev)
        if packets:
            mo["packets"] = t.zeros((nb, PACKETBLOBS, self.packet_capacity(W)), dtype=t.uint8, device=dev)
            mo["packet_bits"] = t.zeros((nb, PACKETBLOBS), dtype=t.int32, device=dev)
        m = _MIO()
        for k, v in mo.items():
            setattr(m, k, _vp(v.data_ptr()))
        if packets:
            m.packet_stride = mo["packets"].shape[-1]
        return mo, m

    def analyze_plan_managed(self, plan, streams, ampmax_states):
        """vamd_analyze_streams_mixed_managed over a plan, the blocks read in place from `streams` (the [nstreams, ch,
        nsamples] tensor the plan was made from).  ampmax_states: cuda float32 [nstreams], updated in place.  Returns per
        size class (index 0 short, 1 long) a dict with `m_packets` [nb,15,packet_capacity] uint8, `m_packet_bits` [nb,15],
        `status` [nb,ch] and the candidates' `m_posts` / `m_post_valid` / `m_iwork` / `m_nonzero`."""
        t = self.torch
        self._need_plan_streams(plan, streams)
        self._need_tensor(ampmax_states, t.float32, "ampmax_states", numel=plan.nstreams)
        dev = self._dev()
        descs, ios, mios, outs = [], [], [], []
        for W in (0, 1):
            nb = plan.nblocks[W]
            descs.append(self._plan_desc(plan, W))
            o = {}
            io, m = _IO(), _MIO()
            if nb:
                o = {"status": t.zeros((nb, self.channels), dtype=t.uint8, device=dev)}
                mo, m = self._managed_outputs(W, nb, dev, packets=True)
                o.update(("m_" + k, v) for k, v in mo.items())
                io.pcm, io.status = _vp(streams.data_ptr()), _vp(o["status"].data_ptr())
                io.pcm_src, io.pcm_channel_stride = plan.src[W], streams.shape[2]
            ios.append(io)
            mios.append(m)
            outs.append(o)
        self._bind_stream()
        self._check(self.L.vamd_analyze_streams_mixed_managed(self.h, C.byref(descs[0]), C.byref(ios[0]), C.byref(mios[0]),
                                                              C.byref(descs[1]), C.byref(ios[1]), C.byref(mios[1]), plan.order,
                                                              plan.stream_start, plan.nstreams, plan.nblocks[0] + plan.nblocks[1],
                                                              _vp(ampmax_states.data_ptr())))
        return outs

    def bitrate_init_states(self, nstreams):
        """vamd_bitrate_init_states: cuda uint8 [nstreams, 32] (vamd_bitrate_state each) at a stream's start."""
        t = self.torch
        states = t.zeros((nstreams, 32), dtype=t.uint8, device=self._dev())
        self._bind_stream()
        self._check(self.L.vamd_bitrate_init_states(self.h, _vp(states.data_ptr()), nstreams))
        return states

    def bitrate_walk(self, order, stream_start, packet_bits, states, status=None):
        """vamd_bitrate_walk.  order: cuda int32 [nb] (W << 30 | index), stream_start: cuda int64 [nstreams + 1],
        packet_bits: per size class a cuda int32 [nb_W, 15] (or None where the class has no blocks), status: per class
        cuda uint8 [nb_W, ch] or None, states: bitrate_init_states() (updated).  -> (choice, final_bits), per class cuda
        int32 [nb_W] (None where the class has no blocks)."""
        t = self.torch
        self._need_tensor(order, t.int32, "order")
        self._need_tensor(stream_start, t.int64, "stream_start")
        self._need_tensor(states, t.uint8, "states", numel=(stream_start.numel() - 1) * 32)
        choice, final = [None, None], [None, None]
        pb, st, ch_p, fb_p = _vp * 2, _vp * 2, _vp * 2, _vp * 2
        pb, st, ch_p, fb_p = pb(), st(), ch_p(), fb_p()
        for W in (0, 1):
            if packet_bits[W] is None:
                continue
            self._need_tensor(packet_bits[W], t.int32, "packet_bits[%d]" % W)
            nb = packet_bits[W].shape[0]
            choice[W] = t.full((nb,), -7, dtype=t.int32, device=self._dev())
            final[W] = t.full((nb,), -7, dtype=t.int32, device=self._dev())
            pb[W], ch_p[W], fb_p[W] = packet_bits[W].data_ptr(), choice[W].data_ptr(), final[W].data_ptr()
            if status is not None and status[W] is not None:
                self._need_tensor(status[W], t.uint8, "status[%d]" % W, numel=nb * self.channels)
                st[W] = status[W].data_ptr()
        self._bind_stream()
        self._check(self.L.vamd_bitrate_walk(self.h, _vp(order.data_ptr()), _vp(stream_start.data_ptr()), stream_start.numel() - 1,
                                             pb, st, _vp(states.data_ptr()), ch_p, fb_p))
        return choice, final

    def decode_prepare(self, streams, granules=None, offset=None, stream_start=None, packet_granules=None, eos=None):
        """The descriptor of decode_streams()'s group (vamd_decode_desc) with the host arrays it points into; with
        packet_granules, also the marks (vamd_decode_marks)."""
        ns = len(streams)
        for row in streams:
            for p in row:
                self._need(isinstance(p, (bytes, bytearray, memoryview)), "decode_streams: a packet must be bytes (a missing packet is not decodable)")
        flat = [bytes(p) for row in streams for p in row]
        data = np.frombuffer(b"".join(flat) + b"\0" * 8, np.uint8)
        off = np.zeros(len(flat) + 1, np.int64)
        np.cumsum([len(p) for p in flat], out=off[1:])
        start = np.zeros(ns + 1, np.int64)
        np.cumsum([len(row) for row in streams], out=start[1:])
        if offset is not None:
            off = np.ascontiguousarray(offset, np.int64)
            self._need(off.size == len(flat) + 1, "decode_streams: offset must hold npackets + 1 values")
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
        m = prep.get("marks")
        if m is not None:  # (vamd_decode_plan_marked + vamd_decode_streams_marked: the marks ride behind the descriptor)
            return self._decode_run(lambda h, d, *a: self.L.vamd_decode_plan_marked(h, d, C.byref(m), *a),
                                    lambda h, d, *a: self.L.vamd_decode_streams_marked(h, d, C.byref(m), *a), prep, pcm)
        return self._decode_run(self.L.vamd_decode_plan, self.L.vamd_decode_streams, prep, pcm)

    def _decode_run(self, plan, run, prep, pcm):
        """the plan call, the output tensor, the decode call: of the packet entry and of the Ogg entry alike"""
        t = self.torch
        ns, d = prep["nstreams"], prep["desc"]
        frames, nblocks = np.zeros(max(ns, 1), np.int64), np.zeros(2, np.int64)
        self._check(plan(self.h, C.byref(d), _vp(frames.ctypes.data), _vp(nblocks.ctypes.data)))
        out_off = np.zeros(max(ns, 1), np.int64)
        if ns > 1:
            out_off[1:ns] = np.cumsum(frames[:ns - 1] * self.channels)
        total = int((frames[:ns] * self.channels).sum())
        if pcm is None:
            pcm = t.zeros(total + 4, dtype=self._pcm_dtype, device=self._dev())
        self._need_tensor(pcm, self._pcm_dtype, "pcm")
        self._need(pcm.numel() >= total, "pcm must hold %d elements" % total)
        status = np.zeros(max(ns, 1), np.uint8)
        self._bind_stream()
        self._check(run(self.h, C.byref(d), _vp(out_off.ctypes.data), _vp(pcm.data_ptr()), _vp(status.ctypes.data)))
        return pcm, frames[:ns], out_off[:ns], status[:ns]

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

    _PCM_CODES = {"float32": PCM_F32, "int16": PCM_S16, "float16": PCM_F16, "bfloat16": PCM_BF16}

    def _set_output(self, dtype, interleaved):
        t = self.torch
        code = self._PCM_CODES.get(str(dtype).replace("torch.", "")) if isinstance(dtype, t.dtype) else None
        self._need(code is not None, "pcm_dtype must be torch.float32, int16, float16 or bfloat16 (it is %r)" % (dtype,))
        fmt = _PcmFormat(code, 1 if interleaved else 0)
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
        code = self._PCM_CODES.get(str(dtype).replace("torch.", "")) if isinstance(dtype, t.dtype) else None
        self._need(code is not None, "dtype must be torch.float32, int16, float16 or bfloat16 (it is %r)" % (dtype,))
        ch, frames = int(tensor.shape[0]), int(tensor.shape[1])
        out = t.empty((frames, ch) if interleaved else (ch, frames), dtype=dtype, device=self._dev())
        fmt = _PcmFormat(code, 1 if interleaved else 0)
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
        if not hasattr(self, "_live"):
            self._live = []
        d = LiveDecoder(self, max_streams)
        self._live.append(d)
        return d

    def live_ogg_decoder(self, max_streams, setup_header=None, max_packet_bytes=0, max_header_bytes=0):
        """vamd_decode_ogg_live_create: a LiveOggDecoder for up to max_streams continuing Ogg Vorbis streams on this context.
        setup_header: the setup header packet every stream's third packet must equal, or None; max_packet_bytes: the longest
        audio packet that may stay open between pieces (0: the larger packet capacity); max_header_bytes: what the three
        header packets may hold together (0: 1 MiB).  Closing the Analyzer closes it."""
        if not hasattr(self, "_live"):
            self._live = []
        d = LiveOggDecoder(self, max_streams, setup_header, max_packet_bytes, max_header_bytes)
        self._live.append(d)
        return d

    def decode_ogg_prepare(self, files, setup_header=None, file_offset=None):
        """The descriptor of decode_ogg()'s group (vamd_decode_ogg_desc) with the host arrays it points into."""
        for f in files:
            self._need(isinstance(f, (bytes, bytearray, memoryview)), "decode_ogg: a file must be bytes")
        ns = len(files)
        data = np.frombuffer(b"".join(bytes(f) for f in files) + b"\0" * 8, np.uint8)
        off = np.zeros(ns + 1, np.int64)
        np.cumsum(np.array([len(f) for f in files], np.int64), out=off[1:])
        if file_offset is not None:
            off = np.ascontiguousarray(file_offset, np.int64)
            self._need(off.size == ns + 1, "decode_ogg: file_offset must hold nstreams + 1 values")
        hdr = np.frombuffer(bytes(setup_header), np.uint8) if setup_header is not None else None
        d = _DecodeOggDesc(ns, _vp(data.ctypes.data), _vp(off.ctypes.data), _vp(hdr.ctypes.data) if hdr is not None and hdr.size else None,
                           hdr.size if hdr is not None else 0)
        return dict(desc=d, keep=(data, off, hdr), nstreams=ns)

    def decode_ogg_run(self, prep, pcm=None):
        """vamd_decode_ogg_plan + vamd_decode_ogg over decode_ogg_prepare()'s descriptor; pcm and the result as decode_run's"""
        return self._decode_run(self.L.vamd_decode_ogg_plan, self.L.vamd_decode_ogg, prep, pcm)

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

    def _window_run(self, plan, run, nw, pcm, stride=None):
        """a window call's plan call, output tensor and decode call: _decode_run with a window per "stream".  stride: None, or
        every window's channel stride in a pcm the caller made (window w at w * channels * stride)"""
        t = self.torch
        frames, nblocks = np.zeros(max(nw, 1), np.int64), np.zeros(2, np.int64)
        self._check(plan(_vp(frames.ctypes.data), _vp(nblocks.ctypes.data)))
        per = frames if stride is None else np.full(max(nw, 1), int(stride), np.int64)
        out_off = np.zeros(max(nw, 1), np.int64)
        if nw > 1:
            out_off[1:nw] = np.cumsum(per[:nw - 1] * self.channels)
        total = int((per[:nw] * self.channels).sum())
        if pcm is None:
            pcm = t.zeros(total + 4, dtype=self._pcm_dtype, device=self._dev())
        self._need_tensor(pcm, self._pcm_dtype, "pcm")
        self._need(pcm.numel() >= total, "pcm must hold %d elements" % total)
        status = np.zeros(max(nw, 1), np.uint8)
        self._bind_stream()
        self._check(run(_vp(out_off.ctypes.data), _vp(pcm.data_ptr()), _vp(status.ctypes.data)))
        return pcm, frames[:nw], out_off[:nw], status[:nw]

    def decode_window(self, streams, granules, stream, start, count, with_status=False, offset=None, stream_start=None):
        """vamd_decode_window_plan + vamd_decode_window: windows of packet streams.  streams / granules (or None) as
        decode_streams() takes them; window w is frames [start[w], start[w] + count[w]) of streams[stream[w]], cut to the
        stream's end.  Only the packets of the blocks a window needs go up.  -> a list of float32 tensors [ch, frames], one
        per window, bit for bit those frames of decode_streams()'s tensors; with_status, also the windows' status bytes."""
        self._need(len(stream) == len(start) == len(count), "decode_window: stream, start and count must be as long as each other")
        prep = self.decode_prepare(streams, granules, offset, stream_start)
        nw, (ws, wa, wc) = self._window_arrays(stream, start, count)
        args = (self.h, C.byref(prep["desc"]), nw, _vp(ws.ctypes.data), _vp(wa.ctypes.data), _vp(wc.ctypes.data))
        res = self._window_run(lambda *a: self.L.vamd_decode_window_plan(*args, *a), lambda *a: self.L.vamd_decode_window(*args, *a), nw, None)
        return self._decoded_tensors(nw, *res, with_status)

    def ogg_index(self, files, setup_header=None, file_offset=None):
        """vamd_ogg_index_create: one walk of whole Ogg Vorbis files, kept -> an OggIndex, whose decode() / crops() give
        windows of those files without walking or uploading them whole again.  files / setup_header / file_offset as
        decode_ogg() takes them; the index keeps the files' bytes (one joined copy).  Closing the Analyzer closes it."""
        if not hasattr(self, "_live"):
            self._live = []
        x = OggIndex(self, files, setup_header, file_offset)
        self._live.append(x)
        return x

    def analyze_block(self, pcm, lW=1, W=1, nW=1, blocktype=BLOCKTYPE_LONG, ampmax_in=-9999.0):
        """vamd_analyze_block: host numpy pcm[ch][n] in, host numpy results out (the per-block
        compatibility path that sits behind vorbis_analysis())."""
        ch, n2 = self.channels, self.blocksizes[W] // 2
        pcm, ptrs = self._host_block(pcm, W)
        o = dict(mdct=np.empty((ch, n2), np.float32), logmask=np.empty((ch, n2), np.float32),
                 posts=np.empty((ch, POSTS_STRIDE), np.int32), post_valid=np.empty(ch, np.int32),
                 iwork=np.empty((ch, n2), np.int32), nonzero=np.empty(ch, np.int32))
        amp = C.c_float(0)
        self._bind_stream()
        cap = self.residue_capacity(W)
        if cap > 0:  # the residue back-end's decisions ride along where the mode is covered
            S = self.submaps(W)
            rcls, rent, rcnt = np.zeros(S * RES_CLASS_STRIDE, np.int32), np.zeros(cap, np.uint16), np.zeros(2 * S, np.int32)
            self._check(self.L.vamd_analyze_block_res(
                self.h, ptrs, lW, W, nW, blocktype, ampmax_in, _vp(o["mdct"].ctypes.data), _vp(o["logmask"].ctypes.data),
                _vp(o["posts"].ctypes.data), _vp(o["post_valid"].ctypes.data), _vp(o["iwork"].ctypes.data),
                _vp(o["nonzero"].ctypes.data), C.cast(C.byref(amp), _vp), _vp(rcls.ctypes.data), _vp(rent.ctypes.data),
                _vp(rcnt.ctypes.data)))
            o["res_class"], o["res_entries"] = self.residue_lists(W, rcls, rent, rcnt)
        else:
            self._check(self.L.vamd_analyze_block(self.h, ptrs, lW, W, nW, blocktype, ampmax_in,
                                                  _vp(o["mdct"].ctypes.data), _vp(o["logmask"].ctypes.data),
                                                  _vp(o["posts"].ctypes.data), _vp(o["post_valid"].ctypes.data),
                                                  _vp(o["iwork"].ctypes.data), _vp(o["nonzero"].ctypes.data),
                                                  C.byref(amp)))
        o["ampmax_out"] = amp.value
        return o

    # ---- bitrate-managed blocks: fifteen candidate packets each (vamd_analyze_*_managed) ------------
    def analyze_managed(self, pcm, W=1, lW=1, nW=1, blocktype=BLOCKTYPE_LONG, ampmax_in=-9999.0, residue=False,
                        packets=False, want=()):
        """vamd_analyze_batch_managed.  pcm: cuda float32 [nblocks, ch, n].  Returns a dict: shared `mdct`,
        `logmask`, `ampmax_out`, and per candidate `m_posts` [nb,15,ch,32], `m_post_valid` / `m_nonzero`
        [nb,15,ch], `m_iwork` [nb,15,ch,n/2] (+ `m_res_class`, `m_res_entries`, `m_res_count` with residue=True;
        + `m_packets` [nb,15,packet_capacity] uint8, `m_packet_bits` [nb,15] with packets=True)."""
        self._need_batch(pcm, self.blocksizes[W])
        nb = pcm.shape[0]
        outs = self.alloc_outputs(W, nb, ("mdct", "logmask", "ampmax_out") + tuple(want))  # (want: further shared outputs, e.g. "status")
        keep = []
        d = self._desc(W, nb, lW, nW, blocktype, ampmax_in, keep)
        io = self._io(pcm, outs)
        mo, m = self._managed_outputs(W, nb, pcm.device, residue, packets)
        self._bind_stream()
        self._check(self.L.vamd_analyze_batch_managed(self.h, C.byref(d), C.byref(io), C.byref(m)))
        for k, v in mo.items():
            outs["m_" + k] = v
        return outs

    def analyze_block_managed(self, pcm, lW=1, W=1, nW=1, blocktype=BLOCKTYPE_LONG, ampmax_in=-9999.0):
        """vamd_analyze_block_managed: host numpy pcm[ch][n] in; shared mdct / ampmax_out and the fifteen
        candidates' m_posts / m_post_valid / m_iwork / m_nonzero (+ residue decisions where covered) out."""
        ch, n2 = self.channels, self.blocksizes[W] // 2
        pcm, ptrs = self._host_block(pcm, W)
        o = dict(mdct=np.empty((ch, n2), np.float32), m_posts=np.empty((PACKETBLOBS, ch, POSTS_STRIDE), np.int32),
                 m_post_valid=np.empty((PACKETBLOBS, ch), np.int32), m_iwork=np.empty((PACKETBLOBS, ch, n2), np.int32),
                 m_nonzero=np.empty((PACKETBLOBS, ch), np.int32))
        amp = C.c_float(0)
        cap = self.residue_capacity(W)
        S = self.submaps(W)
        rcls = np.zeros((PACKETBLOBS, S * RES_CLASS_STRIDE), np.int32)
        rent = np.zeros((PACKETBLOBS, max(cap, 1)), np.uint16)
        rcnt = np.zeros((PACKETBLOBS, 2 * S), np.int32)
        rp = [_vp(rcls.ctypes.data), _vp(rent.ctypes.data), _vp(rcnt.ctypes.data)] if cap > 0 else [None, None, None]
        self._bind_stream()
        self._check(self.L.vamd_analyze_block_managed(
            self.h, ptrs, lW, W, nW, blocktype, ampmax_in, _vp(o["mdct"].ctypes.data), C.cast(C.byref(amp), _vp),
            _vp(o["m_posts"].ctypes.data), _vp(o["m_post_valid"].ctypes.data), _vp(o["m_iwork"].ctypes.data),
            _vp(o["m_nonzero"].ctypes.data), *rp))
        o["ampmax_out"] = amp.value
        if cap > 0:
            lists = [self.residue_lists(W, rcls[k], rent[k], rcnt[k]) for k in range(PACKETBLOBS)]
            o["m_res_class"] = [l[0] for l in lists]
            o["m_res_entries"] = [l[1] for l in lists]
        return o

    def encode_block(self, pcm, lW=1, W=1, nW=1, blocktype=BLOCKTYPE_LONG, ampmax_in=-9999.0, managed=False):
        """vamd_encode_block: host numpy pcm[ch][n] in; (list of 1 or 15 packets as bytes, ampmax_out) out."""
        pcm, ptrs = self._host_block(pcm, W)
        nk, cap = (PACKETBLOBS if managed else 1), self.packet_capacity(W)
        pk, bits = np.zeros((nk, max(cap, 4)), np.uint8), np.zeros(nk, np.int32)
        amp = C.c_float(0)
        self._bind_stream()
        self._check(self.L.vamd_encode_block(self.h, ptrs, lW, W, nW, blocktype, C.c_float(ampmax_in), 1 if managed else 0,
                                             C.cast(C.byref(amp), _vp), _vp(pk.ctypes.data), C.c_long(pk.shape[1]),
                                             _vp(bits.ctypes.data)))
        return [packet_bytes(pk[k], bits[k]) for k in range(nk)], amp.value

    def encode_blocks(self, pcm, lW, W, nW, blocktype, ampmax_in_first=-9999.0, managed=False):
        """vamd_encode_blocks: consecutive blocks of ONE stream in one launch sequence.  pcm: list of host numpy
        [ch][blocksize[W[b]]]; lW / W / nW / blocktype: per block.  Returns (packets[b][k] as bytes -- None where the
        block's verdict is not VAMD_OK --, ampmax_in float32[nb], ampmax_out float32[nb], verdict int32[nb])."""
        ch, nb = self.channels, len(pcm)
        self._need(nb == len(lW) == len(W) == len(nW) == len(blocktype), "one lW / W / nW / blocktype per block")
        keep = [np.ascontiguousarray(x, dtype=np.float32) for x in pcm]
        for b in range(nb):
            self._need(int(W[b]) in (0, 1) and keep[b].shape == (ch, self.blocksizes[int(W[b])]),
                       "pcm[%d] must be [%d][blocksize[W]]" % (b, ch))
        ptrs = (_vp * max(1, nb * ch))(*[_vp(keep[b][c].ctypes.data) for b in range(nb) for c in range(ch)])
        arr = [np.ascontiguousarray(v, dtype=np.int32) for v in (lW, W, nW, blocktype)]
        nk, cap = (PACKETBLOBS if managed else 1), max(self.packet_capacity(0), self.packet_capacity(1), 4)
        pk, bits = np.zeros((max(nb, 1), nk, cap), np.uint8), np.zeros((max(nb, 1), nk), np.int32)
        ain, aout, verdict = np.zeros(max(nb, 1), np.float32), np.zeros(max(nb, 1), np.float32), np.zeros(max(nb, 1), np.int32)
        self._bind_stream()
        self._check(self.L.vamd_encode_blocks(self.h, C.c_long(nb), ptrs, *[_vp(a.ctypes.data) for a in arr],
                                              C.c_float(ampmax_in_first), 1 if managed else 0, _vp(ain.ctypes.data),
                                              _vp(aout.ctypes.data), _vp(pk.ctypes.data), C.c_long(cap),
                                              _vp(bits.ctypes.data), _vp(verdict.ctypes.data)))
        packets = [[packet_bytes(pk[b, k], bits[b, k]) for k in range(nk)] if verdict[b] == 0 else None for b in range(nb)]
        return packets, ain[:nb], aout[:nb], verdict[:nb]

    # ---- the block-switching detector (vamd_envelope_search*) ---------------------------------
    def envelope_geometry(self):
        w, s = C.c_int(0), C.c_int(0)
        self._check(self.L.vamd_envelope_geometry(self.h, C.byref(w), C.byref(s)))
        return w.value, s.value

    def envelope_search(self, pcm, nsteps, state=None):
        """vamd_envelope_search: host pcm[ch][>= (nsteps-1)*searchstep + winlength] -> (ret flags uint8[nsteps],
        state).  `state` is an EnvelopeState (None = start of stream) and is updated in place."""
        ch = self.channels
        win, step = self.envelope_geometry()
        pcm = np.ascontiguousarray(pcm, dtype=np.float32)
        self._need(pcm.ndim == 2 and pcm.shape[0] == ch and pcm.shape[1] >= (nsteps - 1) * step + win,
                   "pcm must be [%d][>= %d samples]" % (ch, (nsteps - 1) * step + win))
        if state is None:
            state = EnvelopeState()
        ret = np.zeros(nsteps, np.uint8)
        ptrs = self._row_pointers(pcm)
        self._bind_stream()
        self._check(self.L.vamd_envelope_search(self.h, ptrs, nsteps, C.byref(state), _vp(ret.ctypes.data)))
        return ret, state

    def envelope_search_batch(self, pcm, nsteps, states=None, ret=None):
        """vamd_envelope_search_batch: cuda float32 pcm[nstreams][ch][len]; states = cuda uint8 tensor
        [nstreams][sizeof(vamd_envelope_state)] (zeros = fresh streams), updated in place.
        Returns (ret cuda uint8 [nstreams][nsteps], states)."""
        t = self.torch
        self._need_tensor(pcm, t.float32, "pcm")
        self._need(pcm.dim() == 3, "pcm must be [streams, channels, samples]")
        ns, ch, ln = pcm.shape
        self._need(ch == self.channels, "pcm must have %d channels" % self.channels)
        win, step = self.envelope_geometry()
        self._need(ln >= (nsteps - 1) * step + win, "streams too short for %d steps" % nsteps)
        if states is None:
            states = self._fresh_states(ns)
        if ret is None:
            ret = t.empty((ns, nsteps), dtype=t.uint8, device=pcm.device)
        self._bind_stream()
        self._check(self.L.vamd_envelope_search_batch(self.h, _vp(pcm.data_ptr()), ch * ln, ln, ns, nsteps,
                                                      _vp(states.data_ptr()), _vp(ret.data_ptr())))
        return ret, states


class LiveDecoder:
    """vamd_decode_live: continuing streams decoded in pieces, a stream per slot (Analyzer.live_decoder).  A stream's
    pieces laid end to end are what Analyzer.decode_streams gives for the whole stream, at any cut of its packet list."""

    def __init__(self, analyzer, max_streams):
        self.an, self.max_streams = analyzer, int(max_streams)
        h = _vp()
        analyzer._check(analyzer.L.vamd_decode_live_create(analyzer.h, self.max_streams, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.an.L.vamd_decode_live_destroy(self.h)
            self.h = None
            if self in self.an._live:
                self.an._live.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prepare(self, slots, pieces, close=(), end_granules=None):
        """The descriptor of a call (vamd_decode_live_desc) with the host arrays it points into.  slots: the slots this call
        names; pieces[i]: the list of packets (bytes) of slot slots[i], in order -- it may be empty; close: the slots whose
        stream ends with this piece; end_granules: {slot: the granule position of the stream's last packet} for closing
        slots (a live feed's closing group carries it), a sequence with one value per slot of the call (None or -1: none),
        or None."""
        an = self.an
        an._need(self.h is not None, "live decoder: closed")
        an._need(len(slots) == len(pieces), "live decoder: one piece per slot")
        for row in pieces:
            for p in row:
                an._need(isinstance(p, (bytes, bytearray, memoryview)), "live decoder: a packet must be bytes")
        ns = len(slots)
        flat = [bytes(p) for row in pieces for p in row]
        data = np.frombuffer(b"".join(flat) + b"\0" * 8, np.uint8)
        off = np.zeros(len(flat) + 1, np.int64)
        np.cumsum([len(p) for p in flat], out=off[1:])
        start = np.zeros(ns + 1, np.int64)
        np.cumsum([len(row) for row in pieces], out=start[1:])
        slot = np.array([int(s) for s in slots] + [0], np.int64)  # (never an empty array: its pointer is read as non-null)
        closing = set(int(s) for s in close)
        an._need(closing <= set(int(s) for s in slots), "live decoder: a closing slot that this call does not name")
        cl = np.array([int(s) in closing for s in slots] + [0], np.uint8)
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
        return an._decode_run(lambda _, *a: an.L.vamd_decode_live_plan(h, *a), lambda _, *a: an.L.vamd_decode_live_wrote(h, *a), prep, pcm)

    def write(self, slots, pieces, close=(), end_granules=None, with_status=False):
        """The next piece of each named slot's stream -> a list of float32 tensors [ch, frames] on the context's device, one
        per slot of the call; a dead stream -- one that has held a flagged packet -- gives [ch, 0] until a piece closes it.
        with_status, also the status bytes (numpy uint8).  See prepare() for the arguments."""
        return self.an._decoded_tensors(len(slots), *self.run(self.prepare(slots, pieces, close, end_granules)), with_status)


class LiveOggDecoder:
    """vamd_decode_ogg_live: continuing Ogg Vorbis streams decoded in pieces of bytes, a stream per slot
    (Analyzer.live_ogg_decoder).  The pieces may be cut at any byte; for a clean stream that ends in an end-of-stream page
    their samples laid end to end are what Analyzer.decode_ogg gives for the whole file."""

    def __init__(self, analyzer, max_streams, setup_header=None, max_packet_bytes=0, max_header_bytes=0):
        self.an, self.max_streams = analyzer, int(max_streams)
        hdr = np.frombuffer(bytes(setup_header), np.uint8) if setup_header is not None else None
        opts = _DecodeOggLiveOpts(_vp(hdr.ctypes.data) if hdr is not None and hdr.size else None, hdr.size if hdr is not None else 0,
                                  int(max_packet_bytes), int(max_header_bytes))
        h = _vp()
        analyzer._check(analyzer.L.vamd_decode_ogg_live_create(analyzer.h, self.max_streams, C.byref(opts), C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.an.L.vamd_decode_ogg_live_destroy(self.h)
            self.h = None
            if self in self.an._live:
                self.an._live.remove(self)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prepare(self, slots, pieces, close=(), piece_offset=None):
        """The descriptor of a call (vamd_decode_ogg_live_desc) with the host arrays it points into.  slots: the slots this
        call names; pieces[i]: the next bytes of slot slots[i]'s stream -- any number of them, none included; close: the slots
        whose stream ends with this piece.  piece_offset: a test hook, the descriptor's array as given."""
        an = self.an
        an._need(self.h is not None, "live Ogg decoder: closed")
        an._need(len(slots) == len(pieces), "live Ogg decoder: one piece per slot")
        for p in pieces:
            an._need(isinstance(p, (bytes, bytearray, memoryview)), "live Ogg decoder: a piece must be bytes")
        ns = len(slots)
        data = np.frombuffer(b"".join(bytes(p) for p in pieces) + b"\0" * 8, np.uint8)
        off = np.zeros(ns + 1, np.int64)
        np.cumsum(np.array([len(p) for p in pieces], np.int64), out=off[1:])
        if piece_offset is not None:
            off = np.ascontiguousarray(piece_offset, np.int64)
            an._need(off.size == ns + 1, "live Ogg decoder: piece_offset must hold nstreams + 1 values")
        slot = np.array([int(s) for s in slots] + [0], np.int64)  # (never an empty array: its pointer is read as non-null)
        closing = set(int(s) for s in close)
        an._need(closing <= set(int(s) for s in slots), "live Ogg decoder: a closing slot that this call does not name")
        cl = np.array([int(s) in closing for s in slots] + [0], np.uint8)
        d = _DecodeOggLiveDesc(ns, _vp(slot.ctypes.data), _vp(data.ctypes.data), _vp(off.ctypes.data), _vp(cl.ctypes.data))
        return dict(desc=d, keep=(data, off, slot, cl), nstreams=ns)

    def run(self, prep, pcm=None):
        """vamd_decode_ogg_live_plan + vamd_decode_ogg_live_wrote over prepare()'s descriptor; pcm and the result as
        Analyzer.decode_run's: (pcm, frames, offset, status)"""
        an, h = self.an, self.h
        an._need(h is not None, "live Ogg decoder: closed")
        return an._decode_run(lambda _, *a: an.L.vamd_decode_ogg_live_plan(h, *a), lambda _, *a: an.L.vamd_decode_ogg_live_wrote(h, *a), prep, pcm)

    def write(self, slots, pieces, close=(), with_status=False):
        """The next bytes of each named slot's stream -> a list of float32 tensors [ch, frames] on the context's device, one
        per slot of the call: the samples of the audio packets those bytes complete; a dead stream -- one that has been
        flagged -- gives [ch, 0] until a piece closes it.  with_status, also the status bytes (numpy uint8)."""
        return self.an._decoded_tensors(len(slots), *self.run(self.prepare(slots, pieces, close)), with_status)


class OggIndex:
    """vamd_ogg_index: the seek index of a group of Ogg Vorbis files (Analyzer.ogg_index).  frames[s] and status[s] are what
    a whole decode_ogg() plans for file s on the host; decode() and crops() give windows of the files, bit for bit the same
    frames of the whole decode.  Damage outside a window's own pages is not seen by that window."""

    def __init__(self, analyzer, files, setup_header=None, file_offset=None, own=False):
        self.an, self._own, self.h = analyzer, own, None
        prep = analyzer.decode_ogg_prepare(files, setup_header, file_offset)
        self._data, self._off = prep["keep"][0], prep["keep"][1]
        self.nstreams = prep["nstreams"]
        h = _vp()
        analyzer._check(analyzer.L.vamd_ogg_index_create(analyzer.h, C.byref(prep["desc"]), C.byref(h)))
        self.h = h
        self.frames, self.status = np.zeros(max(self.nstreams, 1), np.int64), np.zeros(max(self.nstreams, 1), np.uint8)
        analyzer._check(analyzer.L.vamd_ogg_index_info(h, None, _vp(self.frames.ctypes.data), _vp(self.status.ctypes.data)))
        self.frames, self.status = self.frames[:self.nstreams], self.status[:self.nstreams]

    def close(self):
        if getattr(self, "h", None):
            self.an.L.vamd_ogg_index_destroy(self.h)
            self.h = None
            if self in getattr(self.an, "_live", ()):
                self.an._live.remove(self)
            if self._own:
                self.an.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _run(self, stream, start, count, pcm=None, stride=None, files=None, file_offset=None, row=None):
        """vamd_decode_ogg_window_plan + vamd_decode_ogg_window -> (pcm, frames, offset, status) per window.  files /
        file_offset: test hooks, other bytes than the index was made of."""
        an = self.an
        an._need(self.h is not None, "ogg index: closed")
        an._need(len(stream) == len(start) == len(count), "ogg index: stream, start and count must be as long as each other")
        data, off = self._data, self._off
        if files is not None:
            data = np.frombuffer(b"".join(bytes(f) for f in files) + b"\0" * 8, np.uint8)
            off = np.zeros(len(files) + 1, np.int64)
            np.cumsum(np.array([len(f) for f in files], np.int64), out=off[1:])
            an._need(len(files) == self.nstreams, "ogg index: as many files as the index has")
        if file_offset is not None:
            off = np.ascontiguousarray(file_offset, np.int64)
            an._need(off.size == self.nstreams + 1, "ogg index: file_offset must hold nstreams + 1 values")
        nw, (ws, wa, wc) = an._window_arrays(stream, start, count)
        cs = np.full(max(nw, 1), int(stride), np.int64) if stride is not None else None
        d = _OggWindowDesc(nw, _vp(ws.ctypes.data), _vp(wa.ctypes.data), _vp(wc.ctypes.data), _vp(data.ctypes.data), _vp(off.ctypes.data),
                           _vp(cs.ctypes.data) if cs is not None else None)
        args = (an.h, self.h, C.byref(d))
        return an._window_run(lambda *a: an.L.vamd_decode_ogg_window_plan(*args, *a, None), lambda *a: an.L.vamd_decode_ogg_window(*args, *a), nw, pcm, stride if row is None else row)

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
    a = Analyzer(setup_blob, device)
    try:
        a._set_output(a.pcm_dtype if dtype is None else dtype, bool(interleaved))
        x = OggIndex(a, files, setup_header, own=True)
    except Exception:
        a.close()
        raise
    return x


def decode(setup_blob, streams, granules=None, with_status=False, device=None, keep_partial=False, dtype=None, interleaved=None):
    """Analyzer(setup_blob).decode_streams(...) for a caller who holds packets and no context: the packets must come from an
    encoder of that setup.  keep_partial: Analyzer.keep_partial for the call; dtype / interleaved: Analyzer.pcm_dtype /
    pcm_interleaved for the call."""
    a = Analyzer(setup_blob, device)
    try:
        a.keep_partial = keep_partial
        return a.decode_streams(streams, granules, with_status, dtype=dtype, interleaved=interleaved)
    finally:
        a.close()


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
    a = Analyzer(default_setup_blob(), tensor.device.index if hasattr(tensor, "device") and tensor.device.index is not None else None)
    try:
        return a.pcm_convert(tensor, dtype, interleaved)
    finally:
        a.close()


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
            a = Analyzer.from_headers(ident, setup, device)
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
    a = Analyzer(setup_blob, device)
    try:
        a.keep_partial = keep_partial
        return a.decode_ogg(files, setup_header, with_status, follow_links=follow_links, dtype=dtype, interleaved=interleaved)
    finally:
        a.close()
