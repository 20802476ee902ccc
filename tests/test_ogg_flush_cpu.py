"""CPU suite: the live Ogg feed's flush per write (vamd_feed_ogg_flush) as far as it needs no GPU -- the mux in pieces of
vorbis_amd/csrc/k_ogg.h with a flush per group (compiled with the host compiler, tests/ogg_host.py), which the device
path is held against.  The size lists and cuts are tests/signals.py's; flush masks: none, all, random per group.
Held against a second implementation of the policy (a segment at a time, in Python); mask "none" is the whole mux's file;
every piece is whole pages with correct checksums; the flushed file demuxes to the same packets; nothing is held back
behind a flush; a flushed page has the shape the contract gives it; the bounds a live group is sized by hold."""
import numpy as np
import pytest

from tests import ogg_framing as fr
from tests import ogg_host as oh
from tests.signals import HB, LIVE_SIZE_LISTS as SIZE_LISTS, cuts_of

FIELDS = ("nseg", "body", "done", "flags", "granule", "seq")


@pytest.fixture(scope="module")
def hosts():
    host = oh.HostOgg()
    return host, host


def masks_of(groups, rng):
    """-> (name, flush flag per group): none, all, random (the last group closes its stream: a flag there must not matter)"""
    n = len(groups)
    return [("none", [False] * n), ("all", [True] * n), ("random", [bool(v) for v in rng.integers(0, 2, n)])]


def run_cut(live, headers, packets, granules, groups, mask, serial, cap, seen):
    """One stream through the shipped mux in pieces with the flushes of `mask`; every per-group property is asserted here.
    -> the pieces (bytes, pages, whether the group flushed), and whether the stream was closed without a packet onto an
    open page that a flush had emptied: the case a feed never meets (k_ogg.h, ogg_flush), which ends without an e_o_s page"""
    hb = [len(h) for h in headers]
    st = live.stream(headers, serial)
    model = fr.PolicyModel(hb)
    got = fr.Reassembler()
    pieces, k, seq, bare_close = [], 0, 0, False
    for g, n in enumerate(groups):
        close, flush = g == len(groups) - 1, mask[g]
        bare_close = close and n == 0 and st.begun and st.ncarry == 0
        piece = st.piece(packets[k:k + n], granules[k:k + n], close, flush)
        new = [len(p) for p in packets[k:k + n]]
        k += n
        # 1. the second implementation: the same pages
        want = model.group(new, granules[k - n:k], close, flush)
        assert [tuple(p[f] for f in FIELDS) for p in st.pages] == [tuple(p[f] for f in FIELDS) for p in want], (g, groups, mask)
        # 3. a whole number of pages, every checksum, consecutive sequence numbers
        pages = fr.pages_of(piece)
        assert len(pages) == st.npages
        for p, w in zip(pages, want):
            assert p["seq"] == seq and p["serial"] == serial
            assert tuple(p[f] for f in FIELDS) == tuple(w[f] for f in FIELDS)
            seq += 1
        got.take(pages)
        # the carry's bound
        assert 0 <= st.ncarry <= 255 and st.carried <= live.carry_body and st.carried_rounded <= live.carry_bytes - 18
        assert st.ncarry == (0 if close else st.open_page["npackets"]) and st.carried == (0 if close else st.open_page["body"])
        # 7. the bounds a group is sized by before any size is known (with and without a comment header per stream)
        assert st.npages <= live.live_slots(hb, n, cap), (g, st.npages)
        rounded = sum((v + 3) // 4 * 4 for v in new)
        assert len(piece) <= live.live_file_bound(rounded, n, 1, hb), (g, len(piece))
        assert len(piece) <= live.live_file_bound(rounded, n, 1, hb, comment_sum=hb[1]), (g, len(piece))
        if flush and not close:
            # 5. nothing is held back: no carry, no open page, and the bytes so far hold every packet given so far, whole
            assert st.ncarry == 0 and st.open_page["npackets"] == 0 and st.open_page["nseg"] == 0
            assert not got.is_open and got.packets == headers + packets[:k], (g, groups)
            # 6. the group's last page -- the flushed one, unless the open page was empty -- ends with its packet, and has a granule position
            if pages:
                assert pages[-1]["lacing"][-1] < 255 and pages[-1]["granule"] != -1 and not pages[-1]["flags"] & 4
        for p, w in zip(pages, want):
            if w["flushed"]:
                assert p["lacing"][-1] < 255 and p["granule"] != -1 and not p["flags"] & 4 and p is pages[-1]
                seen["flushed"] += 1
                seen["continued"] += bool(p["flags"] & 1)
                seen["many"] += p["done"] >= 200
        pieces.append((piece, pages, flush and not close))
    assert k == len(packets)
    return pieces, bare_close


@pytest.mark.parametrize("name", list(SIZE_LISTS))
def test_flushed_pieces(hosts, name):
    whole, live = hosts
    sizes = SIZE_LISTS[name]
    rng = np.random.default_rng(len(sizes))
    headers = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in HB]
    packets = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]
    granules = [int(v) for v in np.cumsum(rng.integers(1, 2049, len(sizes)))]
    serial = 0xf1a50000 + len(sizes)
    unflushed = whole.mux(headers, packets, granules, serial)
    n_unflushed = len(fr.demux(unflushed)[0])
    seen = {"flushed": 0, "continued": 0, "many": 0, "bare_close": 0}
    for groups in cuts_of(name, len(sizes), rng):
        for mask_name, mask in masks_of(groups, rng):
            pieces, bare_close = run_cut(live, headers, packets, granules, groups, mask, serial, max(sizes), seen)
            f = b"".join(p for p, _, _ in pieces)
            if mask_name == "none":
                assert f == unflushed, groups                       # 2. today's behaviour
                continue
            # 4. the flushed file: a well-formed stream of the same packets, longer by a header and lacing table per flushed page
            fp, got = fr.demux(f)
            assert got == headers + packets
            assert [bool(p["flags"] & 4) for p in fp] == [False] * (len(fp) - 1) + [not bare_close] and fp[0]["flags"] == 2
            seen["bare_close"] += bare_close
            assert len(f) - len(unflushed) == 27 * (len(fp) - n_unflushed)  # (the lacing values are the packets', whatever the pages)
            # 6. every audio page but the last: the fill rule, 255 segments, or the last page of a flushing group
            audio = [(p, flushing and p is pages[-1]) for _, pages, flushing in pieces for p in pages][2:]
            for p, last_of_flushing in audio[:-1]:
                assert (p["body"] > fr.FILL and p["done"] >= fr.MIN_PACKETS) or p["nseg"] == 255 or last_of_flushing, (groups, mask, p["seq"])
    # 8. the coverage guards: some flushed page carries the continued flag, some holds at least 200 packets
    assert seen["flushed"] > 0 and seen["bare_close"] > 0
    if name == "254_one_byte_then_2000":
        assert seen["continued"] > 0, seen
    if name == "70000_among_small":
        assert seen["continued"] > 0, seen
    if name == "400_one_byte":
        assert seen["many"] > 0, seen


def test_the_cut_that_leaves_byte0_255_flushed(hosts):
    """254 one-byte packets and the first 255 bytes of a 2000-byte one fill a page; cut behind that packet, the open page
    begins 255 bytes into it.  Flushed there, it leaves as a continued page of 1745 bytes, and the next page is fresh."""
    _, live = hosts
    sizes = SIZE_LISTS["254_one_byte_then_2000"]
    rng = np.random.default_rng(1)
    packets = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]
    granules = list(range(1, len(sizes) + 1))
    plain = live.stream(None, 9)
    plain.piece(packets[:255], granules[:255], False)
    assert plain.open_page["byte0"] == 255 and plain.open_page["flags"] & 1
    st = live.stream(None, 9)
    a = fr.pages_of(st.piece(packets[:255], granules[:255], False, True))
    assert [(p["nseg"], p["body"], p["flags"], p["granule"]) for p in a] == [(255, 509, 0, 254), (7, 1745, 1, 255)]
    assert st.ncarry == 0
    b = fr.pages_of(st.piece(packets[255:], granules[255:], True, True))
    assert b[0]["flags"] & 1 == 0 and b[0]["seq"] == 2 and b[-1]["flags"] == 4


def test_a_flush_of_an_empty_open_page_and_of_a_carry_alone(hosts):
    """A flushed group without packets hands out the carried packets' page; a second one nothing.  A flush before any
    packet hands out the header pages alone, and flushing twice changes nothing."""
    _, live = hosts
    rng = np.random.default_rng(2)
    headers = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in HB]
    packets = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (300, 20, 700)]
    st = live.stream(headers, 3)
    assert [p["seq"] for p in fr.pages_of(st.piece([], [], False, True))] == [0, 1]       # (30 + 4229 bytes: one page each)
    assert st.piece([], [], False, True) == b""
    assert st.piece(packets[:2], [10, 20], False, False) == b"" and st.ncarry == 2
    page = fr.pages_of(st.piece([], [], False, True))
    assert len(page) == 1 and (page[0]["seq"], page[0]["done"], page[0]["granule"], page[0]["body"]) == (2, 2, 20, 320)
    assert st.piece([], [], False, True) == b"" and st.ncarry == 0
    last = fr.pages_of(st.piece(packets[2:], [30], True, True))
    assert len(last) == 1 and (last[0]["seq"], last[0]["flags"], last[0]["granule"]) == (3, 4, 30)


def test_the_flush_bit_is_a_bit_of_its_own(hosts):
    _, live = hosts
    assert live.flush_bit == 8
