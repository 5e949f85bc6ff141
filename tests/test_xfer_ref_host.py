"""tests/xfer_ref.py without a GPU: the constants it reads from csrc/xfer.cpp and csrc/xfer_team.hpp are found, what it says about the
team's lifetime holds in the source, every cell of the grid of tests/test_gpu_host_transfers.py crosses the edge it names, and the
host arena puts guards and data where it says."""
import numpy as np

import xfer_ref as XR


def test_constants_and_team_lifetime_are_read_from_the_sources():
    c = XR.constants()
    assert c == {"NBUF": 4, "TEAM_MIN": 1 << 20, "MIN_MB": 16, "CHUNK_MB": 32, "MAX_THREADS": 16}
    facts = XR.team_lifetime_facts()
    assert all(facts.values()), facts


def test_every_cell_crosses_its_edge():
    c = XR.constants()
    cells = XR.cells(c)
    for cell in cells:
        XR.assert_edge(cell, c)
    assert max(x["bytes"] for x in cells) == XR.MAX_BYTES and max(x["threads"] for x in cells) == 16
    assert {x["threads"] for x in cells} == set(XR.THREADS) and {x["off"] for x in cells} == {0, 8}
    # the class of lengths whose tail the team once dropped, at the thread counts that have one
    assert XR.class_length(16, 8, 1 << 20) == (1 << 20) + 8 and XR.class_length(12, 8, 1 << 20) == 4096 * 12 * 22 + 8 == 1081352
    assert {(x["threads"], x["r"]) for x in cells if x["kind"] == "class"} == {
        (2, 1), (3, 1), (7, 1), (7, 4), (12, 1), (12, 4), (12, 8), (16, 1), (16, 4), (16, 8)}


def test_host_arena_and_mismatch():
    a = XR.HostArena(cap=3 * XR.PAGE)
    for off in (0, 8):
        for n in (0, 1, 4097):
            data, (front, back) = a.place(n, off)
            start = front.ctypes.data + XR.HOST_GUARD                # an empty slice has no address of its own to ask for
            assert start % XR.PAGE == off and len(data) == n and len(front) == len(back) == XR.HOST_GUARD
            assert start + n == back.ctypes.data and (n == 0 or data.ctypes.data == start)
            assert XR.guards_intact((front, back))
            back[0] ^= 1
            assert not XR.guards_intact((front, back))
    x = np.arange(10, dtype=np.uint8)
    y = x.copy()
    assert XR.mismatch(x, y) is None
    y[7:] = 0
    assert XR.mismatch(y, x) == "3 bytes wrong, first at 7 of 10"
    p = XR.pattern()
    assert len(p) >= XR.MAX_BYTES + 4099 and not p.flags.writeable and not np.array_equal(p[:4096], p[4096:8192])
