"""CPU suite: an Ogg file in pieces -- the resumed paging walk, the carry and the mux in pieces of vorbis_amd/csrc/k_ogg.h
(compiled with the host compiler, tests/ogg_host.py), which the live Ogg feed's device path is held against.  Whatever
the cut into groups, the pieces laid end to end are the file the whole-stream mux (ogg_mux) makes of the same packets;
every piece is a whole number of pages with correct checksums; the carry and the two bounds a live group is sized by
hold."""
import numpy as np
import pytest

from tests import ogg_framing as fr
from tests import ogg_host as oh
from tests.signals import HB, LIVE_SIZE_LISTS as SIZE_LISTS, cuts_of


@pytest.fixture(scope="module")
def hosts():
    host = oh.HostOgg()
    return host, host


def run_cut(live, headers, packets, granules, groups, serial, cap, seen):
    """-> the pieces, each with its number of pages; seen: the coverage guard's tally of what the open pages held"""
    st = live.stream(headers, serial)
    pieces, k = [], 0
    for g, n in enumerate(groups):
        close = g == len(groups) - 1
        piece = st.piece(packets[k:k + n], granules[k:k + n], close)
        new = [len(p) for p in packets[k:k + n]]
        k += n
        # the carry's bound, and the two bounds a group is sized by before any size is known
        assert 0 <= st.ncarry <= 255 and st.carried <= live.carry_body and st.carried_rounded <= live.carry_bytes - 18
        assert st.ncarry == (0 if close else st.open_page["npackets"])
        assert st.carried == (0 if close else st.open_page["body"])
        assert st.npages <= live.live_slots([len(h) for h in headers], n, cap), (g, st.npages)
        assert len(piece) <= live.live_file_bound(sum((v + 3) // 4 * 4 for v in new), n, 1, [len(h) for h in headers]), (g, len(piece))
        if not close:
            seen["continued"] += st.open_page["byte0"] > 0
            seen["carried"] += st.open_page["npackets"] >= 200
        pieces.append((piece, st.npages))
    assert k == len(packets)
    return pieces


@pytest.mark.parametrize("name", list(SIZE_LISTS))
def test_pieces_equal_the_whole_mux(hosts, name):
    whole, live = hosts
    sizes = SIZE_LISTS[name]
    rng = np.random.default_rng(len(sizes))
    headers = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in HB]
    packets = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]
    granules = [int(v) for v in np.cumsum(rng.integers(1, 2049, len(sizes)))]
    serial = 0xfeed0000 + len(sizes)
    want = whole.mux(headers, packets, granules, serial)
    want_pages, got = fr.demux(want)
    assert got == headers + packets
    seen = {"continued": 0, "carried": 0}
    for groups in cuts_of(name, len(sizes), rng):
        pieces = run_cut(live, headers, packets, granules, groups, serial, max(sizes), seen)
        assert b"".join(p for p, _ in pieces) == want, groups
        seq = 0
        for piece, npages in pieces:
            pages = fr.pages_of(piece)                              # a whole number of pages, every checksum
            assert len(pages) == npages
            for p in pages:
                assert p["seq"] == seq and p["serial"] == serial
                seq += 1
        assert seq == len(want_pages)
        # a page is handed out once it is closed, never before: no group but the closing one ends with the stream's last page
        assert all(not fr.pages_of(p)[-1]["flags"] & 4 for p, n in pieces[:-1] if n)
    # the coverage guard: these inputs leave, at some boundary, an open page that began inside a packet (byte0 > 0) and one
    # that carries at least 200 packets -- so neither case can go uncovered silently
    if name == "254_one_byte_then_2000":
        assert seen["continued"] > 0 and seen["carried"] > 0, seen
    if name == "400_one_byte":
        assert seen["carried"] > 0, seen
    if name == "70000_among_small":
        assert seen["continued"] > 0, seen


def test_a_bare_run_and_a_second_stream_in_the_same_state(hosts):
    """Without headers (a bare audio run); and after a close the same state begins a new file: sequence numbers from 0."""
    whole, live = hosts
    rng = np.random.default_rng(23)
    st = live.stream(None, 5)
    for trial in range(3):
        sizes = [int(v) for v in rng.integers(0, 900, 40)]
        packets = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]
        granules = list(range(100, 100 + len(sizes)))
        got = st.piece(packets[:13], granules[:13], False) + st.piece([], [], False) + st.piece(packets[13:], granules[13:], True)
        assert got == whole.mux(None, packets, granules, 5)
        assert fr.pages_of(got)[0]["seq"] == 0
