"""vamd_ctx in Python: the Analyzer -- batches, streams, plans, the bitrate manager's candidates, the detector.  Its decode
methods, the handles made from it and decode() / decode_ogg() / ogg_index() for a caller who holds no context are
decoder.py's, and are found here under the names they have always had."""
import ctypes as C

import numpy as np

from .abi import (ABI_VERSION, BLOCKTYPE_LONG, LEVEL_FULL, LEVEL_PSY, LEVEL_TRANSFORM, PACKETBLOBS, POSTS_STRIDE, QUANT_LIMIT_INT,
                  QUANT_LIMIT_SQUARE, RES_CLASS_STRIDE, STATUS_RANGE, VAMD_EDOMAIN, VAMD_ENONFINITE, VAMD_OK, EnvelopeState, VamdError,
                  _Desc, _IO, _MIO, _Plan, _vp, load_library)
from .decoder import (DecodeMixin, LiveDecoder, LiveOggDecoder, OggIndex, decode, decode_ogg, decode_ogg_files, ogg_index, ogg_links,  # noqa: F401
                      pcm_convert, read_ogg_headers)
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


class Analyzer(DecodeMixin):
    """One vamd_ctx: the GPU-side counterpart of a vorbis_dsp_state's lookups."""

    def __init__(self, setup_blob, device=None, _headers=None):
        import torch
        self.torch = torch
        self.L = load_library()
        self._live = []  # the handles made from this context (decoder.py, _Handle): closed with it
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
