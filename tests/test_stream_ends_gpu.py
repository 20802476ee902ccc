"""GPU suite: the two extrapolated ends of a stream as the GPU build makes them -- the lag-per-lane fp64 sums and the systolic
fp32 predictor line of k_lpc.h (#if VAMD_GPU), which no host build compiles -- against the reference's application loop on
the case table of tests/stream_edge_cases.py: the SAMPLES of every block bit for bit (floats as uint32, so signed zeros
count), because packets do not notice them (tests/test_stream_ends_cpu.py has the figures).  Then what is built on those
samples: the planned blocks through the analysis, the detector alone, the float-fed feed with its decoded signal, and
device-fed float16 / bfloat16 groups whose values are subnormal halves.  No tolerances anywhere."""
import numpy as np
import pytest

from oracle import ref
from tests import feed_source_host as fs
from tests import ref_host
from tests import stream_edge_cases as sc
from tests.feed_cases import check_state, decoded_feed_of, diff, same_bits

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not ref.available(), reason="oracle/_ref not built")]
SETUP_NAMES = tuple(sc.SETUPS)
TAPPED = ("44k_stereo_q4", "44k_stereo_qm1")
_BLOBS = {}


def u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def blob_of(setup):
    if setup not in _BLOBS:
        _BLOBS[setup] = sc.encoder(setup).pack_setup()
    return _BLOBS[setup]


def what_of(setup, i):
    return "%s, %d frames" % sc.case_list(setup)[i]


def lay_out(setup, idx):
    """the cases idx as vamd_plan_streams_whole takes them: [ns, ch, row] with every row laid out for the longest stream
    [blocksizes[1]/2 of room | samples | zeros], and the streams' lengths"""
    ch, _, _, bs = sc.SETUPS[setup]
    xs = [sc.signals(setup)[i] for i in idx]
    frames = [x.shape[1] for x in xs]
    row = (bs[1] // 2 + max(frames) + 3 * bs[1] + 3) // 4 * 4
    buf = np.zeros((len(xs), ch, row), np.float32)
    for s, x in enumerate(xs):
        buf[s, :, bs[1] // 2:bs[1] // 2 + x.shape[1]] = x
    return buf, frames


def run_plan(setup, idx, equal):
    """One plan over the cases idx (equal: the equal-length entry point) -> dict(an, plan, t = the device buffer, raw / filled
    = the buffer before / after on the host, frames, L = the plan's lists, blocks = the gathered blocks per size class)"""
    import torch
    import vorbis_amd
    an = vorbis_amd.Analyzer(blob_of(setup), 0)
    assert tuple(an.blocksizes) == sc.SETUPS[setup][3]
    raw, frames = lay_out(setup, idx)
    t = torch.from_numpy(raw).cuda()
    if equal:
        assert len(set(frames)) == 1
    plan, _ = an.plan_streams_whole(t, frames[0] if equal else np.array(frames, np.int64))
    L = an.plan_lists(plan)
    blocks = [an.gather_blocks(plan, W, t).cpu().numpy() if plan.nblocks[W] else None for W in (0, 1)]
    torch.cuda.synchronize()
    return dict(an=an, plan=plan, t=t, raw=raw, filled=t.cpu().numpy(), frames=frames, L=L, blocks=blocks, idx=idx)


def plan_mismatches(setup, w):
    """per stream the first thing in which the plan, the gathered blocks or the buffer differ from the reference's records"""
    ch, _, _, bs = sc.SETUPS[setup]
    head, pad = bs[1] // 2, 3 * bs[1]
    L, row = w["L"], w["raw"].shape[2]
    bad = []
    for s, i in enumerate(w["idx"]):
        recs, n, what = sc.records(setup)[i], w["frames"][s], what_of(setup, i)
        lo, hi = int(L["stream_start"][s]), int(L["stream_start"][s + 1])
        if not same_bits(w["filled"][s, :, head:head + n], w["raw"][s, :, head:head + n]):
            bad.append("%s: the real samples were changed" % what)
            continue
        if w["filled"][s, :, head + n + pad:].view(np.uint32).any():
            bad.append("%s: something was written behind the stream's padding" % what)
            continue
        if hi - lo != len(recs):
            bad.append("%s: %d blocks, the reference %d" % (what, hi - lo, len(recs)))
            continue
        begins = sc.begins_of(recs, bs)
        for k, o in enumerate(L["order"][lo:hi]):
            W, j = (int(o) >> 30) & 1, int(o) & 0x3fffffff
            b = recs[k]
            got = (W, int(L["lW"][W][j]), int(L["nW"][W][j]), int(L["blocktype"][W][j]))
            if got != (b["W"], b["lW"], b["nW"], b["blocktype"]):
                bad.append("%s: block %d of %d is (W, lW, nW, blocktype) = %s, the reference's %s" % (
                    what, k, len(recs), got, (b["W"], b["lW"], b["nW"], b["blocktype"])))
                break
            if int(L["src"][W][j]) != s * ch * row + begins[k]:
                bad.append("%s: block %d of %d begins at %d, the reference's at %d" % (
                    what, k, len(recs), int(L["src"][W][j]) - s * ch * row, begins[k]))
                break
            d = np.nonzero((u32(w["blocks"][W][j]) != u32(b["pcm"])).any(axis=0))[0]
            if len(d):
                c = int(np.nonzero(u32(w["blocks"][W][j])[:, d[0]] != u32(b["pcm"])[:, d[0]])[0][0])
                bad.append("%s: block %d of %d (W %d): %d samples differ, the first is sample %d of the %s, channel %d: %r, the reference %r" % (
                    (what, k, len(recs), W, len(d)) + sc.where_of(begins[k], int(d[0]), n, bs[1])[::-1] +
                    (c, float(w["blocks"][W][j][c, d[0]]), float(b["pcm"][c, d[0]]))))
                break
            if not same_bits(w["filled"][s, :, begins[k]:begins[k] + bs[W]], b["pcm"]):
                bad.append("%s: block %d: the gathered block is the reference's, the buffer at its place is not" % (what, k))
                break
    return bad


@pytest.fixture(scope="module")
def planned():
    """per setup the whole table as ONE vamd_plan_streams_whole_v call, made when first asked for and kept for the module"""
    made = {}

    def get(setup):
        if setup not in made:
            made[setup] = run_plan(setup, list(range(len(sc.case_list(setup)))), equal=False)
        return made[setup]
    yield get
    for w in made.values():
        w["an"].close()


# ---- 1. the whole-stream plan ----
@pytest.mark.parametrize("setup", SETUP_NAMES)
def test_whole_plan_of_unequal_lengths_matches_the_reference(setup, planned):
    """ALL cases of the setup in one call with an array of lengths (rows laid out for the longest stream): per stream the
    block count, every block's flags and place, every block's samples bit for bit -- the extrapolated ones are what this is
    about -- and the real samples untouched"""
    w = planned(setup)
    assert w["plan"].nstreams == len(sc.case_list(setup))
    bad = plan_mismatches(setup, w)
    assert not bad, "%d of %d streams differ:\n%s" % (len(bad), len(w["idx"]), "\n".join(bad))


@pytest.mark.parametrize("setup", SETUP_NAMES)
def test_whole_plan_of_equal_lengths_matches_the_reference(setup):
    """vamd_plan_streams_whole (one length for all) over the full-length kinds"""
    w = run_plan(setup, sc.full_cases(setup), equal=True)
    try:
        bad = plan_mismatches(setup, w)
    finally:
        w["an"].close()
    assert not bad, "%d of %d streams differ:\n%s" % (len(bad), len(w["idx"]), "\n".join(bad))


# ---- 2. the planned blocks through the analysis ----
@pytest.mark.parametrize("setup", TAPPED)
def test_planned_blocks_through_the_analysis(setup, planned):
    """analyze_plan in place over the whole table's plan: ampmax_out of EVERY block and the chain's final state against the
    reference's records; mdct, post_valid, iwork, nonzero of each stream's first two and last two blocks -- the ones made of
    extrapolated samples -- against the reference's taps.  Every case lies inside the input domain: no block is flagged."""
    import torch
    w = planned(setup)
    an, plan, L = w["an"], w["plan"], w["L"]
    want = ("mdct", "post_valid", "iwork", "nonzero", "ampmax_out", "status")
    outs = [an.alloc_outputs(W, plan.nblocks[W], want) for W in (0, 1)]
    states = torch.full((plan.nstreams,), -9999.0, device="cuda")
    an.analyze_plan(plan, None, outs, states, streams=w["t"])
    torch.cuda.synchronize()
    assert an.input_status() == (0, 0)
    host = [{k: v.cpu().numpy() for k, v in outs[W].items()} for W in (0, 1)]
    states = states.cpu().numpy()
    enc = sc.encoder(setup)
    bad = []
    for s, i in enumerate(w["idx"]):
        recs, what = sc.records(setup)[i], what_of(setup, i)
        lo, hi = int(L["stream_start"][s]), int(L["stream_start"][s + 1])
        assert hi - lo == len(recs), what
        for k, o in enumerate(L["order"][lo:hi]):
            W, j = (int(o) >> 30) & 1, int(o) & 0x3fffffff
            b = recs[k]
            assert not host[W]["status"][j].any(), (what, k)
            if np.float32(host[W]["ampmax_out"][j]) != np.float32(b["ampmax_out"]):
                bad.append("%s: block %d of %d: ampmax_out %r, the reference %r" % (what, k, len(recs), float(host[W]["ampmax_out"][j]), b["ampmax_out"]))
                break
            if k in (0, 1, len(recs) - 2, len(recs) - 1):
                r = enc.tap_block(b["pcm"], b["lW"], b["W"], b["nW"], b["blocktype"], b["ampmax_in"])
                assert not an.beyond_quant_limit(W, r["iwork"], residue=False).any(), (what, k)
                for key in ("mdct", "post_valid", "iwork", "nonzero"):
                    g, x = host[W][key][j], np.asarray(r[key])
                    if g.shape != x.shape or not np.array_equal(u32(g) if g.dtype == np.float32 else g, u32(x) if x.dtype == np.float32 else x):
                        bad.append("%s: block %d of %d: %s differs" % (what, k, len(recs), key))
        if np.float32(states[s]) != np.float32(recs[-1]["ampmax_out"]):
            bad.append("%s: the chain ends at %r, the reference's at %r" % (what, float(states[s]), recs[-1]["ampmax_out"]))
    assert not bad, "\n".join(bad)


def test_the_loudest_case_stays_inside_the_integer_bound():
    """steady noise 50 dB over full scale: the reference's quantised values of all its blocks, under every setup, stay
    within the setup's bound (vamd_quant_limit) -- the table holds no stream whose result is undefined"""
    import vorbis_amd
    for setup in SETUP_NAMES:
        an = vorbis_amd.Analyzer(blob_of(setup), 0)
        enc = sc.encoder(setup)
        i = [k for k, _ in sc.case_list(setup)].index("steady_over_50dB")
        try:
            for k, b in enumerate(sc.records(setup)[i]):
                r = enc.tap_block(b["pcm"], b["lW"], b["W"], b["nW"], b["blocktype"], b["ampmax_in"])
                assert not an.beyond_quant_limit(b["W"], r["iwork"]).any(), (setup, k)
        finally:
            an.close()


# ---- 3. the detector alone ----
@pytest.mark.parametrize("setup", SETUP_NAMES)
def test_detector_alone_on_the_edge_streams(setup):
    """the full-length kinds as the reference's detector saw them (its own buffer: no extrapolation made here) through
    envelope_search_batch, in one call and in ragged chunks with the states carried on the device: the reference's marks
    and its final filter state"""
    import torch
    import vorbis_amd
    from vorbis_amd import EnvelopeState, envelope_marks
    ch = sc.SETUPS[setup][0]
    seen = []
    for i in sc.full_cases(setup):
        seen.append(sc.encoder(setup).envelope_feed(sc.signals(setup)[i]))
    steps = seen[0]["steps"]
    assert steps > 8 and all(o["steps"] == steps for o in seen)
    ln = (steps - 1) * 64 + 128
    pcm = torch.from_numpy(np.stack([o["pcm"][:, :ln] for o in seen])).cuda()
    an = vorbis_amd.Analyzer(blob_of(setup), 0)
    try:
        assert an.envelope_geometry() == (128, 64)
        ret, states = an.envelope_search_batch(pcm, steps)
        st2, out, j, k = None, [], 0, 0
        sizes = (1, 3, 16, 17, 32, 5, 64, 250)
        while j < steps:
            n = min(sizes[k % len(sizes)], steps - j)
            r, st2 = an.envelope_search_batch(pcm[:, :, j * 64:j * 64 + (n - 1) * 64 + 128].contiguous(), n, states=st2)
            out.append(r.cpu().numpy())
            j, k = j + n, k + 1
        torch.cuda.synchronize()
        ret, states, st2 = ret.cpu().numpy(), states.cpu().numpy(), st2.cpu().numpy()
    finally:
        an.close()
    assert np.array_equal(np.concatenate(out, axis=1), ret)
    assert np.array_equal(states, st2)
    assert len(set(int(o["marks"].sum()) for o in seen)) > 2, "the streams should differ in what the detector makes of them"
    for s, i in enumerate(sc.full_cases(setup)):
        o = seen[s]
        assert np.array_equal(envelope_marks(ret[s])[:steps + 2], o["marks"]), what_of(setup, i)
        try:
            check_state(EnvelopeState.from_buffer_copy(states[s].tobytes()), o, ch)
        except AssertionError as e:
            raise AssertionError("%s: the detector's final state differs: %s" % (what_of(setup, i), e))


# ---- 4. the feed, float-fed ----
def feed_rows(setup, parts, **kw):
    """parts [frames_s, ch] float32 each, as one VAMD_FEED_F32 group -> per stream its rows"""
    import vorbis_amd
    feed = vorbis_amd.Feed(blob_of(setup), lanes_per_device=1, max_streams=len(parts), max_frames=max(len(p) for p in parts),
                           fmt=vorbis_amd.FEED_F32, **kw)
    try:
        return feed.encode(parts)
    finally:
        feed.close()


def row_mismatches(setup, idx, got):
    bad = []
    for s, i in enumerate(idx):
        bad += ["%s: %s" % (what_of(setup, i), d) for d in diff(sc.rows_of(sc.records(setup)[i]), got[s], s)]
    return bad


@pytest.mark.parametrize("setup", SETUP_NAMES)
def test_float_fed_feed_matches_the_reference(setup):
    """the setup's whole table as one VAMD_FEED_F32 group: bytes, granule position, W and e_o_s of every packet"""
    idx = list(range(len(sc.case_list(setup))))
    got = feed_rows(setup, [np.ascontiguousarray(sc.signals(setup)[i].T) for i in idx])
    bad = row_mismatches(setup, idx, got)
    assert not bad, "\n".join(bad)


def test_decoded_feed_matches_the_reference_decoder():
    """44k_stereo_q4's table through the decoded feed: the signal back is libvorbis' decoder's over the same packets"""
    setup = "44k_stereo_q4"
    idx = list(range(len(sc.case_list(setup))))
    parts = [np.ascontiguousarray(sc.signals(setup)[i].T) for i in idx]
    feed = decoded_feed_of(setup, parts)
    try:
        slot, buf = feed.buffer(parts[0].shape[1])
        flat = np.concatenate([p.reshape(-1) for p in parts])
        buf[:flat.size] = flat
        feed.wrote(slot, len(parts), np.array([len(p) for p in parts], np.int64))
        rows = feed._rows(feed.packets(slot), len(parts))
        dec, status = feed.decoded(slot, with_status=True)
        dec = [d.cpu().numpy() for d in dec]
        feed.release(slot)
    finally:
        feed.close()
    bad = row_mismatches(setup, idx, rows)
    assert not bad, "\n".join(bad)
    headers = ref_host.encoder_headers(ref_host.encoder(setup))
    for s, i in enumerate(idx):
        want = ref_host.reference_decode(headers + [r[0] for r in rows[s]], [r[1] for r in rows[s]])
        assert status[s] == 0, what_of(setup, i)
        assert want.shape == (parts[s].shape[1], len(parts[s])), (what_of(setup, i), want.shape)
        assert same_bits(dec[s], want), "%s: %d decoded samples differ" % (
            what_of(setup, i), int((u32(dec[s]) != u32(want)).sum()) if dec[s].shape == want.shape else -1)


# ---- 5. the feed, device-fed 16-bit floats ----
def f16_group(ch, frames):
    """float16 [5, ch, frames]: noise whose every value is a subnormal half, noise straddling that line, signed zeros with
    single subnormal halves, noise at 0.4, noise at amplitude 100 -- made in the 16-bit type"""
    rng = np.random.default_rng(1600 + ch)
    noise = lambda amp: ((rng.random((ch, frames)) - 0.5) * 2 * amp).astype(np.float16)  # noqa: E731
    sub = noise(6.0e-5)
    zeros = np.where(rng.random((ch, frames)) < 0.5, np.float16(-0.0), np.float16(0.0)).astype(np.float16)
    for k, (p, v) in enumerate(((5, 6e-8), (frames // 3, -3e-5), (frames - 40, 6.09e-5), (frames - 1, -6e-8))):
        zeros[k % ch, p] = np.float16(v)
    x = np.stack([sub, noise(2.0e-4), zeros, noise(0.4), noise(100.0)])
    tiny = np.float16(6.1035e-5)  # 2 ** -14, the smallest normal half
    assert sub.any() and (np.abs(sub) < tiny).all() and (np.abs(x[1]) < tiny).any() and (np.abs(x[1]) >= tiny).any()
    assert ((zeros != 0) & (np.abs(zeros) < tiny)).sum() == 4 and np.isfinite(x).all()
    return x


@pytest.mark.parametrize("setup", ["44k_stereo_q4", "8k_mono_q3"])
@pytest.mark.parametrize("dtype", ["f16", "bf16"])
def test_device_fed_16_bit_floats_match_the_reference(setup, dtype):
    """a group that lies in device memory as a strided view of a wider float16 / bfloat16 tensor: its rows are those of a
    host-fed VAMD_FEED_F32 group of the widened values, and the reference's over those values"""
    import torch
    import vorbis_amd
    ch, _, _, bs = sc.SETUPS[setup]
    if dtype == "f16":
        elems = f16_group(ch, sc.FULL_FRAMES[bs[1]])
        floats = elems.astype(np.float32)
        wide = torch.zeros((elems.shape[0], ch, 2 * elems.shape[2] + 3), dtype=torch.float16, device="cuda")
        view = wide[:, :, 3::2]                                  # every other element from an odd one on
        view.copy_(torch.from_numpy(elems).cuda())
    else:
        elems = fs.from_float(fs.SRC_BF16, np.stack([sc.signals(setup)[i] for i in sc.full_cases(setup)]))
        floats = fs.to_float(fs.SRC_BF16, elems)
        wide = torch.zeros((elems.shape[0], ch, elems.shape[2] + 5), dtype=torch.bfloat16, device="cuda")
        view = wide[:, :, 5:]                                    # rows of an odd pitch, from an odd element on
        view.copy_(torch.from_numpy(elems.view(np.int16)).cuda().view(torch.bfloat16))
    assert not view.is_contiguous() and view.shape == elems.shape
    torch.cuda.synchronize()
    feed = vorbis_amd.Feed(blob_of(setup), lanes_per_device=1, max_streams=len(elems), max_frames=elems.shape[2])
    try:
        got = feed.encode_tensors(view)
    finally:
        feed.close()
    host = feed_rows(setup, [np.ascontiguousarray(x.T) for x in floats])
    bad = []
    for s, x in enumerate(floats):
        want = sc.rows_of(sc.encoder(setup).encode_stream(x, write_frames=sc.WRITE_FRAMES))
        bad += ["against the reference: " + d for d in diff(want, got[s], s)]
        bad += ["against the host-fed group: " + d for d in diff([tuple(r) for r in host[s]], got[s], s)]
    assert not bad, "\n".join(bad)
