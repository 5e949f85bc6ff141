"""Dealing of orbits to the eight XCD queues (csrc/xcd_deal.hpp), on the host: tests/xcd_deal_host.cpp includes the header the
library includes, is compiled with the host compiler and prints, per orbit in sequence order, its costs and its queue.

p = 8, 10, 12 prefix sites over a 12-site suffix at half filling, 0 and 2 eligible four-site blocks at 7.8 bits, every cost
(round-robin, rows, slots, requested bytes, out-of-orbit bytes, and a mix of two), orbits dealt one by one and in runs of three:
  * the orbit list (tiles, rows, slots, both byte costs) equals the Python restatement's (profiles/orbit_key.py), so every tile
    is in exactly one orbit and an orbit goes to one queue whole; a queue holds its orbits in sequence order by construction
    (one queue index per orbit), which the rebuilt queues confirm;
  * max - min of the queues' cost is at most the largest single orbit's (run's) cost, the bound of least-loaded dealing;
  * "rows", one by one, equals the loop xcd_queues had before the header existed (restated below), entry for entry;
  * "round-robin" is o % 8 (run number % 8); the orbits of a run share a queue;
  * every cost equals the restatement's deal()."""
import importlib.util
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LS = 12
COSTS = {"rr": 0, "rows": 1, "slots": 2, "req": 3, "out": 4}
MIX = (3, "rows", 400, "slots")          # weights that make the two terms comparable: a slot is up to 256 rows


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("xcd_deal") / "xcd_deal_host")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "spindynamics.jl_amd", "csrc"),
           os.path.join(ROOT, "tests", "xcd_deal_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.fixture(scope="module")
def restatement():
    spec = importlib.util.spec_from_file_location("orbit_key_restatement", os.path.join(ROOT, "profiles", "orbit_key.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


_orbits = {}


def python_orbits(R, p, quad_blocks, cap_tenths):
    """the orbit list as the planner builds it: tiles by ascending base row, orbits by first appearance; computed once per shape"""
    key = (p, quad_blocks, cap_tenths)
    if key not in _orbits:
        nup = (p + LS) // 2
        tiles = [P for P in range(1 << p) if 0 <= nup - bin(P).count("1") <= LS]
        tiles.sort(key=lambda P: sum((1 - ((P >> (k - 1)) & 1)) << (p - k) for k in range(1, p + 1)))
        first, orbits = {}, []
        for P in tiles:
            rep = R.orbit_key(P, p, quad_blocks, cap_tenths)[0]
            if rep not in first:
                first[rep] = len(orbits)
                orbits.append([0, 0, 0, 0, 0])
            o = orbits[first[rep]]
            o[0] += 1
            for k, c in enumerate(R.tile_costs(P, p, LS, nup, quad_blocks, cap_tenths)):
                o[1 + k] += c
        _orbits[key] = (len(tiles), tuple(tuple(o) for o in orbits))
    return _orbits[key]


def dealt(exe, p, quad_blocks, cap_tenths, cost, run):
    args = [str(p), str(LS), str((p + LS) // 2), str(quad_blocks), str(cap_tenths)]
    if isinstance(cost, tuple):
        args += ["5", str(run), str(COSTS[cost[1]]), str(cost[0]), str(COSTS[cost[3]]), str(cost[2])]
    else:
        args += [str(COSTS[cost]), str(run)]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert [row[0] for row in rows] == list(range(len(rows)))
    return [row[1:6] for row in rows], [row[6] for row in rows]


def rows_loop_before_the_header(orbits):
    """xcd_queues as it was: every orbit to the queue with the fewest rows so far, ties to the lowest queue index"""
    q_rows, out = [0] * 8, []
    for orb in orbits:
        x = 0
        for y in range(1, 8):
            if q_rows[y] < q_rows[x]:
                x = y
        out.append(x)
        q_rows[x] += orb[1]
    return out


@pytest.mark.parametrize("cost", ["rr", "rows", "slots", "req", "out", MIX], ids=lambda c: c if isinstance(c, str) else "mix")
@pytest.mark.parametrize("run", [1, 3])
@pytest.mark.parametrize("quad_blocks", [0, 2])
@pytest.mark.parametrize("p", [8, 10, 12])
def test_dealing(exe, restatement, p, quad_blocks, run, cost):
    R = restatement
    n_tiles, want_orbits = python_orbits(R, p, quad_blocks, 78)
    orbits, queue = dealt(exe, p, quad_blocks, 78, cost, run)
    assert tuple(orbits) == want_orbits                                   # same orbits, same five costs
    assert sum(o[0] for o in orbits) == n_tiles                           # every tile in exactly one orbit
    assert all(0 <= x < 8 for x in queue) and len(queue) == len(orbits)   # every orbit in exactly one queue, whole
    queues = [[o for o, x in enumerate(queue) if x == y] for y in range(8)]
    assert sorted(o for q in queues for o in q) == list(range(len(orbits))) and all(q == sorted(q) for q in queues)
    assert queue == R.deal(orbits, cost, run)
    assert all(queue[o] == queue[o - o % run] for o in range(len(orbits)))          # the orbits of a run share a queue
    if cost == "rr":
        assert queue == [(o // run) % 8 for o in range(len(orbits))]
        return
    if cost == "rows" and run == 1:
        assert queue == rows_loop_before_the_header(orbits)
    load = [sum(R.cost_of(orbits[o], cost) for o in q) for q in queues]
    largest = max(sum(R.cost_of(o, cost) for o in orbits[k:k + run]) for k in range(0, len(orbits), run))
    print(f"p={p} blocks={quad_blocks} cost={cost} run={run}: queue cost max - min {max(load) - min(load)}, largest unit {largest}")
    assert max(load) - min(load) <= largest
