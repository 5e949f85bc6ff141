"""The host side of the entanglement kernels, against brute force over the enumerated basis: the block layout of
sd_cut_blocks, the segment tables, the flat work list replayed on the host -- every (tile pair, summation index) of every block covered
exactly once, pieces multiples of the chunk except the last, distinct workspace slots -- and every status code of the host-only entry
points.  No device compute is called here."""
import ctypes as C
import itertools
from math import comb

import numpy as np
import pytest

import entanglement_ref as ER

KC = 16                # SD_CUT_KC
TARGET = 2048          # SD_CUT_TARGET_ITEMS
SIDE = {"A": 0, "B": 1, "auto": 2}
NEW = ["sd_cut_blocks", "sd_cut_plan_info", "sd_cut_plan_items", "sd_cut_segments", "sd_cut_gram", "sd_cut_gram_dev", "sd_cut_gram_time_dev"]
# the shapes of tests/test_gpu_entanglement.py
GPU_SHAPES = [(16, 8, 8), (16, 8, 12), (22, 11, 2), (14, 3, 4), (14, 3, 10), (12, None, 3), (12, None, 6), (12, None, 9),
              (7, 0, 3), (7, 7, 3), (2, 1, 1)]


def test_new_names_are_in_the_prototype_table(pkg):
    for name in NEW:
        assert name in pkg.PROTOTYPES, name
        assert hasattr(pkg.lib(), name)
    for name in ("cut_blocks", "cut_gram", "reduced_density_matrix", "entanglement_spectrum", "entanglement_entropy",
                 "entanglement_profile", "schmidt_gap", "symmetry_resolved_entanglement"):
        assert callable(getattr(pkg, name))
    assert pkg.entanglement.CUT_BLOCK.itemsize == 40 and pkg.entanglement.CUT_ITEM.itemsize == 56        # sd_cut_block, sd_cut_item


def items_of(pkg, m, cut, side):
    n = C.c_int64(-1)
    assert pkg.lib().sd_cut_plan_items(m.h, cut, SIDE[side], None, 0, C.byref(n)) == 0
    out = np.zeros(n.value, dtype=pkg.entanglement.CUT_ITEM)
    assert pkg.lib().sd_cut_plan_items(m.h, cut, SIDE[side], out.ctypes.data, n.value, C.byref(n)) == 0
    return out


def segments_of(pkg, m, cut, side, block):
    n, ln = C.c_int64(-1), C.c_int64(-1)
    assert pkg.lib().sd_cut_segments(m.h, cut, SIDE[side], block, None, 0, C.byref(n), C.byref(ln)) == 0
    out = np.full(n.value, -1, dtype=np.int64)
    assert pkg.lib().sd_cut_segments(m.h, cut, SIDE[side], block, out.ctypes.data_as(C.POINTER(C.c_int64)), n.value, C.byref(n), C.byref(ln)) == 0
    return out, ln.value


@pytest.mark.parametrize("L,nup", [(6, 3), (9, 2), (9, 7), (7, 0), (7, 7), (6, None)])
def test_blocks_and_segments_by_brute_force(pkg, L, nup):
    m = pkg.XXZChain(L, nup=nup, ctx=None)
    states = ER.basis(L, nup)
    assert len(states) == m.N
    for cut in range(1, L):
        mask = (1 << cut) - 1
        # brute force: per m the prefixes and suffixes met, in order of first appearance
        pre, suf = {}, {}
        for s in states.tolist():
            P, S = s & mask, s >> cut
            mm = -1 if nup is None else bin(P).count("1")
            if P not in pre.setdefault(mm, []):
                pre[mm].append(P)
            if S not in suf.setdefault(mm, []):
                suf[mm].append(S)
        for side in ("A", "B", "auto"):
            blocks = pkg.cut_blocks(m, cut, side)
            assert [b.m for b in blocks] == sorted(pre)
            off = 0
            for bi, b in enumerate(blocks):
                assert (b.dA, b.dB) == (len(pre[b.m]), len(suf[b.m]))
                want_side = side if side != "auto" else ("A" if b.dA <= b.dB else "B")
                assert b.side == want_side and b.d == (b.dA if want_side == "A" else b.dB) and b.offset == off
                off += b.d * b.d
                if nup is not None:
                    assert (b.dA, b.dB) == (comb(cut, b.m), comb(L - cut, nup - b.m))
                # the segments against the enumerated basis
                starts, seg_len = segments_of(pkg, m, cut, side, bi)
                row = {s: r for r, s in enumerate(states.tolist())}
                if nup is not None:       # one segment per prefix, in vector order, holding the block's suffixes in their one order
                    assert seg_len == b.dB and len(starts) == b.dA and (np.diff(starts) > 0).all()
                    for a, P in enumerate(pre[b.m]):
                        assert [row[P | S << cut] for S in suf[b.m]] == list(range(starts[a], starts[a] + seg_len))
                else:                     # one segment per suffix value
                    assert seg_len == 1 << cut and len(starts) == 1 << (L - cut)
                    for j in range(len(starts)):
                        assert [row[a | j << cut] for a in range(1 << cut)] == list(range(starts[j], starts[j] + seg_len))


def replay(pkg, m, cut, side):
    """the work list against the blocks: returns (items, pairs, max ns)"""
    blocks = pkg.cut_blocks(m, cut, side)
    items = items_of(pkg, m, cut, side)
    full = m.nup is None
    slots, per_pair = set(), {}
    for it in items:
        b = blocks[it["block"]]
        over_segments = (b.side == "B") if full else (b.side == "A")
        K = (b.dA if b.side == "B" else b.dB)
        tile = 16 if b.d <= 16 else 64
        assert it["tile"] == tile and it["form"] == (0 if over_segments else 1)
        T = -(-b.d // tile)
        assert 0 <= it["ti"] <= it["tj"] < T
        assert 0 <= it["k0"] < it["k1"] <= K
        slots.add((int(it["slot"]), int(it["slot"]) + tile * tile))
        per_pair.setdefault((int(it["block"]), int(it["ti"]), int(it["tj"])), []).append(it)
    n_pairs = 0
    max_ns = 1
    for bi, b in enumerate(blocks):
        tile = 16 if b.d <= 16 else 64
        T = -(-b.d // tile)
        K = (b.dA if b.side == "B" else b.dB)
        for ti in range(T):
            for tj in range(ti, T):
                pieces = per_pair.pop((bi, ti, tj))
                n_pairs += 1
                max_ns = max(max_ns, len(pieces))
                # contiguous cover of [0, K) in ascending order, consecutive slots, multiples of KC except the last
                assert [int(p["piece"]) for p in pieces] == list(range(len(pieces))) and all(p["ns"] == len(pieces) for p in pieces)
                assert pieces[0]["k0"] == 0 and pieces[-1]["k1"] == K
                for p, q in zip(pieces, pieces[1:]):
                    assert p["k1"] == q["k0"] and q["slot"] == p["slot"] + tile * tile
                    assert (p["k1"] - p["k0"]) % KC == 0
                assert all(p["k1"] - p["k0"] >= min(KC, K) for p in pieces[:-1])
    assert not per_pair                                    # nothing below the diagonal, no unknown block
    spans = sorted(slots)                                  # every item owns tile x tile elements of the workspace, none shared
    assert len(spans) == len(items) and spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    ws_elems = spans[-1][1]
    for code, el in ((1, 8), (2, 16)):
        ni, ns, wb = C.c_int64(), C.c_int(), C.c_int64()
        assert pkg.lib().sd_cut_plan_info(m.h, cut, SIDE[side], code, C.byref(ni), C.byref(ns), C.byref(wb)) == 0
        assert (ni.value, ns.value, wb.value) == (len(items), max_ns, ws_elems * el)
    # the split rule: no split when the pairs alone reach the target, else about TARGET items unless K runs out
    if n_pairs >= TARGET:
        assert max_ns == 1
    else:
        assert len(items) <= 2 * TARGET + n_pairs
    return items, n_pairs, max_ns


@pytest.mark.parametrize("L,nup,cut", GPU_SHAPES)
@pytest.mark.parametrize("side", ["A", "B", "auto"])
def test_work_list_covers_every_tile_pair_once(pkg, L, nup, cut, side):
    m = pkg.XXZChain(L, nup=nup, ctx=None)
    if side == "B" and nup is not None and max(comb(L - cut, nup - mm) for mm in range(max(0, nup - (L - cut)), min(cut, nup) + 1)) > 16384:
        with pytest.raises(pkg.ArgumentError):             # a block above SD_CUT_MAX_DIM on the side asked for
            pkg.cut_blocks(m, cut, side)
        return
    items, n_pairs, max_ns = replay(pkg, m, cut, side)
    if (L, nup, cut, side) == (22, 11, 2, "auto"):
        assert max_ns > 1 and any((it["k1"] - it["k0"]) % KC for it in items)        # the last piece is not a multiple of KC
    if (L, nup, cut, side) == (16, 8, 12, "auto"):
        assert max_ns == 1 or n_pairs < TARGET


def test_work_list_on_small_sectors(pkg):
    for L, nup in ((6, 3), (9, 2), (9, 7), (6, None)):
        m = pkg.XXZChain(L, nup=nup, ctx=None)
        for cut in range(1, L):
            for side in ("A", "B", "auto"):
                replay(pkg, m, cut, side)


def test_statuses(pkg):
    E = pkg._lib
    l = pkg.lib()
    m = pkg.XXZChain(9, nup=4, ctx=None)
    nb, ne, ni, ns, wb, ln = C.c_int(), C.c_int64(), C.c_int64(), C.c_int(), C.c_int64(), C.c_int64()
    rec = np.zeros(16, dtype=pkg.entanglement.CUT_BLOCK)
    assert l.sd_cut_blocks(m.h, 4, 2, rec.ctypes.data, 16, C.byref(nb), C.byref(ne)) == 0 and nb.value == 5
    for cut in (0, 9, -1, 100):
        assert l.sd_cut_blocks(m.h, cut, 2, None, 0, C.byref(nb), C.byref(ne)) == E.SD_EARG
        assert l.sd_cut_plan_info(m.h, cut, 2, 2, C.byref(ni), C.byref(ns), C.byref(wb)) == E.SD_EARG
        assert l.sd_cut_plan_items(m.h, cut, 2, None, 0, C.byref(ni)) == E.SD_EARG
        assert l.sd_cut_segments(m.h, cut, 2, 0, None, 0, C.byref(ni), C.byref(ln)) == E.SD_EARG
    for side in (-1, 3):
        assert l.sd_cut_blocks(m.h, 4, side, None, 0, C.byref(nb), C.byref(ne)) == E.SD_EARG
        assert l.sd_cut_plan_info(m.h, 4, side, 2, C.byref(ni), C.byref(ns), C.byref(wb)) == E.SD_EARG
    # NULL pointers, a cap below the count, a block outside the list, a bad dtype
    assert l.sd_cut_blocks(None, 4, 2, None, 0, C.byref(nb), C.byref(ne)) == E.SD_EARG
    assert l.sd_cut_blocks(m.h, 4, 2, None, 0, None, C.byref(ne)) == E.SD_EARG
    assert l.sd_cut_blocks(m.h, 4, 2, None, 0, C.byref(nb), None) == E.SD_EARG
    assert l.sd_cut_blocks(m.h, 4, 2, None, 5, C.byref(nb), C.byref(ne)) == E.SD_EARG
    assert l.sd_cut_blocks(m.h, 4, 2, rec.ctypes.data, 4, C.byref(nb), C.byref(ne)) == E.SD_EARG
    assert l.sd_cut_plan_info(None, 4, 2, 2, C.byref(ni), C.byref(ns), C.byref(wb)) == E.SD_EARG
    assert l.sd_cut_plan_info(m.h, 4, 2, 2, None, C.byref(ns), C.byref(wb)) == E.SD_EARG
    assert l.sd_cut_plan_info(m.h, 4, 2, 0, C.byref(ni), C.byref(ns), C.byref(wb)) == E.SD_EARG
    assert l.sd_cut_plan_items(m.h, 4, 2, None, 1, C.byref(ni)) == E.SD_EARG
    assert l.sd_cut_plan_items(m.h, 4, 2, None, 0, None) == E.SD_EARG
    assert l.sd_cut_segments(m.h, 4, 2, 5, None, 0, C.byref(ni), C.byref(ln)) == E.SD_EARG
    assert l.sd_cut_segments(m.h, 4, 2, -1, None, 0, C.byref(ni), C.byref(ln)) == E.SD_EARG
    assert l.sd_cut_segments(m.h, 4, 2, 0, None, 0, None, C.byref(ln)) == E.SD_EARG
    # a block above SD_CUT_MAX_DIM: the full basis at L = 30, cut 15 has d = 2^15 on either side; cut 14 fits on side A only
    big = pkg.XXZChain(30, nup=None, ctx=None)
    assert l.sd_cut_blocks(big.h, 15, 2, None, 0, C.byref(nb), C.byref(ne)) == E.SD_EARG
    assert l.sd_cut_blocks(big.h, 14, 1, None, 0, C.byref(nb), C.byref(ne)) == E.SD_EARG
    assert l.sd_cut_blocks(big.h, 14, 2, rec.ctypes.data, 16, C.byref(nb), C.byref(ne)) == 0
    assert (nb.value, ne.value, int(rec[0]["m"]), int(rec[0]["side"]), int(rec[0]["d"])) == (1, 16384 ** 2, -1, 0, 16384)
    sector = pkg.XXZChain(32, nup=16, ctx=None)          # C(16, 8) = 12870 fits, the half cut of L = 36 does not
    assert l.sd_cut_blocks(sector.h, 16, 2, None, 0, C.byref(nb), C.byref(ne)) == 0 and nb.value == 17
    assert l.sd_cut_blocks(pkg.XXZChain(36, nup=18, ctx=None).h, 18, 2, None, 0, C.byref(nb), C.byref(ne)) == E.SD_EARG
    # a sharded model
    sh = pkg.XXZChain(12, nup=6, ctx=None)
    sh.set_shard(0, 2)
    assert l.sd_cut_blocks(sh.h, 6, 2, None, 0, C.byref(nb), C.byref(ne)) == E.SD_EARG
    assert l.sd_cut_plan_info(sh.h, 6, 2, 2, C.byref(ni), C.byref(ns), C.byref(wb)) == E.SD_EARG
    sh.set_shard(0, 1)
    assert l.sd_cut_blocks(sh.h, 6, 2, None, 0, C.byref(nb), C.byref(ne)) == 0
    # the Python layer refuses before anything is called
    for bad in (0, 9, 2.5, "3", True):
        with pytest.raises((pkg.ArgumentError, ValueError, TypeError)):
            pkg.cut_blocks(m, bad)
    with pytest.raises(pkg.ArgumentError):
        pkg.cut_blocks(m, 3, side="C")
