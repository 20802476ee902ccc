"""GPU suite: the host-fed farm on bitrate-managed setups (ABR / CBR / min-max; vamd_feed with a blob that carries the
bitrate manager's section).  Whole streams from host memory against the reference's application loop over the same
samples (x / 32768.f for 16-bit, 1024 frames per vorbis_analysis_wrote, vorbis_analysis_addblock's manager picking one
of the fifteen candidates, vorbis_bitrate_flushpacket): packets byte for byte, granulepos, W, e_o_s; the chosen
candidate (info >> 4) against the host-compiled walk over the reference's own candidates; the slices of a group; and
the two entry points underneath (vamd_analyze_streams_mixed_managed, vamd_bitrate_walk) on their own."""
import numpy as np
import pytest

from tests import bitrate_host as bh
from tests.feed_cases import planar

pytestmark = pytest.mark.gpu


def _ref():
    from oracle import ref
    if not ref.available():
        pytest.skip("needs the reference build")
    return ref


def streams(kind, ch, lengths, seed, fmt):
    """host [frames_s, ch] per stream, int16 or float32 (what the reference then reads: x / 32768.f, or x)"""
    out = []
    for s, n in enumerate(lengths):
        x = bh.signal(kind, ch, n, seed + s).T
        if fmt == "s16":
            out.append(np.clip(np.round(x * 32768.0), -32768, 32767).astype(np.int16))
        else:
            out.append(np.ascontiguousarray(x, dtype=np.float32))
    return out


def compare(ref, ch, rates, pcm, got):
    bad = []
    for s, x in enumerate(pcm):
        want = ref.RefEncoder(ch, 44100, managed=rates).encode_stream(planar(x))
        if len(want) != len(got[s]):
            bad.append("stream %d: %d packets, the reference %d" % (s, len(got[s]), len(want)))
            continue
        for k, (w, g) in enumerate(zip(want, got[s])):
            data, gp, W, eos = g
            if data != w["packet"] or gp != w["granulepos"] or W != w["W"] or eos != w["eos"]:
                bad.append("stream %d packet %d/%d: bytes %s (%s / %d) granulepos %d/%d W %d/%d eos %d/%d" % (
                    s, k, len(want), "equal" if data == w["packet"] else "DIFFER", None if data is None else len(data),
                    len(w["packet"]), gp, w["granulepos"], W, w["W"], eos, w["eos"]))
                break
    return bad


FMT = {"s16": 0, "f32": 1}


@pytest.mark.parametrize("name,ch,rates,kind", bh.CONFIGS, ids=[c[0] for c in bh.CONFIGS])
@pytest.mark.parametrize("fmt", ["s16", "f32"])
def test_feed_managed_matches_the_reference(name, ch, rates, kind, fmt):
    import vorbis_amd
    ref = _ref()
    if fmt == "f32" and name not in ("abr128_stereo", "abr64_mono", "high_min_quiet"):
        pytest.skip("float input on three of the configurations")
    blob = bh.managed_blob(ch, rates)
    frames = 66150
    feed = vorbis_amd.Feed(blob, lanes_per_device=2, max_streams=4, max_frames=frames, fmt=FMT[fmt])
    try:
        # equal lengths (vamd_feed_wrote), then unequal ones with streams shorter than one long block (vamd_feed_wrote_v)
        even = streams(kind, ch, [frames] * 3, 11, fmt)
        got = feed.encode(np.stack(even))
        bad = compare(ref, ch, rates, even, got)
        uneven = streams(kind, ch, [frames, 700, 1500, 40000], 23, fmt)
        got = feed.encode(uneven)
        bad += compare(ref, ch, rates, uneven, got)
    finally:
        feed.close()
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("name,ch,rates,kind", [bh.CONFIGS[0], bh.CONFIGS[3], bh.CONFIGS[5]], ids=["abr", "minmax", "padding"])
def test_info_carries_the_walks_choice(name, ch, rates, kind):
    """info >> 4 of every packet = the choice of the host-compiled walk over the reference's own fifteen candidates of the
    same blocks (and bits = what the manager handed out)."""
    import vorbis_amd
    ref = _ref()
    lib = bh.build()
    blob = bh.managed_blob(ch, rates)
    hw = bh.HostWalk(lib, blob)
    x = streams(kind, ch, [88200], 5, "s16")[0]
    feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=1, max_frames=x.shape[0])
    try:
        slot, buf = feed.buffer(ch)
        buf[:x.size] = x.reshape(-1)
        feed.wrote(slot, 1, x.shape[0])
        r = feed.packets(slot)
        feed.release(slot)
    finally:
        feed.close()
    recs = ref.RefEncoder(ch, 44100, managed=rates).encode_stream(planar(x))
    tap = ref.RefEncoder(ch, 44100, managed=rates)
    cands = [tap.tap_block_managed(q["pcm"], q["lW"], q["W"], q["nW"], q["blocktype"], q["ampmax_in"])["m_packets"] for q in recs]
    choice, fin, _ = hw.walk(hw.new_state(), [[len(p) for p in c] for c in cands], [q["W"] for q in recs])
    assert r["nblocks"] == len(recs)
    assert np.array_equal(r["choice"], choice), (r["choice"], choice)
    assert np.array_equal((r["bits"] + 7) // 8, fin)
    assert len(set(choice.tolist())) > 1


@pytest.mark.parametrize("arena", [None, "4096"])
def test_slices_change_nothing(arena, monkeypatch):
    """VAMD_FEED_SLICE (a test knob) forced down to 7 blocks: a group of two streams then runs in many slices, at least
    three of them inside one stream, with the ampmax chains and the managers carried across -- same bytes as one slice.
    arena: the packet arena starts at 4096 bytes (VAMD_FEED_OUT_BYTES), so it grows between slices, the earlier slices'
    packets kept."""
    import vorbis_amd
    ref = _ref()
    rates = (160000, 96000, 64000)
    blob = bh.managed_blob(2, rates)
    pcm = streams("music", 2, [88200, 30000], 3, "s16")

    def run():
        feed = vorbis_amd.Feed(blob, lanes_per_device=1, max_streams=2, max_frames=88200)
        try:
            slot, buf = feed.buffer(2)
            flat = np.concatenate([x.reshape(-1) for x in pcm])
            buf[:flat.size] = flat
            feed.wrote(slot, 2, [x.shape[0] for x in pcm])
            r = feed.packets(slot)
            feed.release(slot)
        finally:
            feed.close()
        return r
    one = run()
    monkeypatch.setenv("VAMD_TEST_KNOBS", "1")
    monkeypatch.setenv("VAMD_FEED_SLICE", "7")
    if arena:
        monkeypatch.setenv("VAMD_FEED_OUT_BYTES", arena)
    many = run()
    assert not arena or many["total_bytes"] > 4096
    first = int(one["stream_start"][1])
    assert first >= 3 * 7, "the first stream must span at least three slices"
    for k in ("stream_start", "offset", "bits", "granulepos", "info"):
        assert np.array_equal(one[k], many[k]), k
    assert one["total_bytes"] == many["total_bytes"] and np.array_equal(one["bytes"], many["bytes"])
    got = []
    for s in range(2):
        row = []
        for k in range(int(many["stream_start"][s]), int(many["stream_start"][s + 1])):
            o, b = int(many["offset"][k]), int(many["bits"][k])
            row.append((bytes(many["bytes"][o:o + (b + 7) // 8]), int(many["granulepos"][k]), int(many["info"][k]) & 1,
                        (int(many["info"][k]) >> 1) & 1))
        got.append(row)
    bad = compare(ref, 2, rates, pcm, got)
    assert not bad, "\n".join(bad)


def test_walk_on_the_device_equals_the_host_walk():
    """vamd_bitrate_walk on adversarial candidate sizes (device tensors): three streams interleaving both size classes,
    sizes from 0 to far beyond every target, blocks outside the input domain -- choice and final_bits equal the
    host-compiled walk's, and the states it leaves equal the host's."""
    import torch
    import vorbis_amd
    ref = _ref()
    lib = bh.build()
    blob = bh.managed_blob(2, (160000, 96000, 64000))
    hw = bh.HostWalk(lib, blob)
    an = vorbis_amd.Analyzer(blob, device=0)
    rng = np.random.default_rng(9)
    lens = [120, 1, 300]
    Ws, sizes, status = [], [], []
    for n in lens:
        W = (rng.random(n) < 0.8).astype(np.int32)
        base = rng.integers(0, 4000, n)[:, None] * np.where(rng.random((n, 1)) < 0.1, 8, 1)
        sz = np.sort(np.maximum(0, base + rng.integers(-50, 400, (n, 15))), axis=1).astype(np.int32)
        Ws.append(W)
        sizes.append(sz)
        status.append((rng.random(n) < 0.03).astype(np.uint8))
    W_all = np.concatenate(Ws)
    idx = np.zeros_like(W_all)
    cnt = [0, 0]
    for k, w in enumerate(W_all):
        idx[k] = cnt[w]
        cnt[w] += 1
    order = (W_all.astype(np.int64) << 30 | idx).astype(np.int32)
    start = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    sz_all, st_all = np.concatenate(sizes), np.concatenate(status)
    bits = [np.zeros((max(cnt[w], 1), 15), np.int32) for w in (0, 1)]
    stat = [np.zeros((max(cnt[w], 1), 2), np.uint8) for w in (0, 1)]
    for k, w in enumerate(W_all):
        bits[w][idx[k]] = sz_all[k] * 8 - rng.integers(0, 8, 15) * (sz_all[k] > 0)
        stat[w][idx[k], 0] = st_all[k]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    states = an.bitrate_init_states(len(lens))
    choice, final = an.bitrate_walk(dev(order), dev(start), [dev(bits[0]), dev(bits[1])], states, status=[dev(stat[0]), dev(stat[1])])
    torch.cuda.synchronize()
    choice = [c.cpu().numpy() for c in choice]
    final = [f.cpu().numpy() for f in final]
    dstates = states.cpu().numpy()
    for s, n in enumerate(lens):
        st = hw.new_state()
        for k in range(int(start[s]), int(start[s + 1])):
            w, i = W_all[k], idx[k]
            if st_all[k]:
                assert final[w][i] == -1
                continue
            b = bits[w][i]
            c, fb, _ = hw.walk(st, [(b + 7) // 8], [w])
            assert choice[w][i] == c[0], (s, k)
            assert final[w][i] == hw.final_bits(b[c[0]], max(int(fb[0]), 0)), (s, k)
        got = bh.BitrateState.from_buffer_copy(dstates[s].tobytes())
        assert (got.avgfloat, got.minmax_reservoir, got.avg_reservoir) == (st.avgfloat, st.minmax_reservoir, st.avg_reservoir)
    # a VBR context has no manager
    vbr = vorbis_amd.Analyzer(vorbis_amd.default_setup_blob("44k_stereo_q4"), device=0)
    with pytest.raises(vorbis_amd.VamdError) as e:
        vbr.bitrate_init_states(1)
    assert e.value.code == -130


def test_streams_mixed_managed_equals_encode_blocks():
    """vamd_analyze_streams_mixed_managed over a plan of two whole streams (blocks read in place, ampmax chained per
    stream) gives each block the fifteen candidate packets vamd_encode_blocks(managed) gives the same blocks."""
    import torch
    import vorbis_amd
    ref = _ref()
    ch, rates = 2, (-1, 128000, -1)
    blob = bh.managed_blob(ch, rates)
    an = vorbis_amd.Analyzer(blob, device=0)
    frames = 30000
    bs1 = an.blocksizes[1]
    row = (bs1 // 2 + frames + 3 * bs1 + 3) // 4 * 4
    x = np.zeros((2, ch, row), np.float32)
    for s in range(2):
        x[s, :, bs1 // 2:bs1 // 2 + frames] = bh.signal("music", ch, frames, 40 + s)
    t = torch.from_numpy(x).cuda()
    plan, _ = an.plan_streams_whole(t, frames)
    amp = torch.full((2,), -9999.0, dtype=torch.float32, device="cuda")
    outs = an.analyze_plan_managed(plan, t, amp)
    lists = an.plan_lists(plan)
    filled = t.cpu().numpy().reshape(-1)
    torch.cuda.synchronize()
    host = [{k: v.cpu().numpy() for k, v in o.items()} for o in outs]
    for s in range(2):
        blocks, lw, w_, nw, bt, where = [], [], [], [], [], []
        for k in range(int(lists["stream_start"][s]), int(lists["stream_start"][s + 1])):
            o = int(lists["order"][k])
            W, i = (o >> 30) & 1, o & 0x3fffffff
            n = an.blocksizes[W]
            src = int(lists["src"][W][i])
            blocks.append(np.stack([filled[src + c * row:src + c * row + n] for c in range(ch)]))
            lw.append(lists["lW"][W][i]), w_.append(W), nw.append(lists["nW"][W][i]), bt.append(lists["blocktype"][W][i])
            where.append((W, i))
        pk, _, _, verdict = an.encode_blocks(blocks, lw, w_, nw, bt, managed=True)
        assert not verdict.any()
        for b, (W, i) in enumerate(where):
            got = [vorbis_amd.packet_bytes(host[W]["m_packets"][i, j], host[W]["m_packet_bits"][i, j]) for j in range(15)]
            assert got == pk[b], (s, b)
