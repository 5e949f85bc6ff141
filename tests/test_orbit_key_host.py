"""The orbit key of the XCD-aware tile order (csrc/orbit_key.hpp), on the host: tests/orbit_key_host.cpp includes the header, is
compiled with the host compiler and prints (representative, member id) for every prefix configuration P of p sites.

p = 8 (two whole blocks), 10 (a leftover pair), 11 (a leftover pair and a single site), 12 (three blocks); all 2^p prefixes, so
every prefix filling; capacities 6.2 and 7.2 bits; 0, 2 and all leading blocks eligible for quad status.  For every P:
  * the Python restatement (profiles/orbit_key.py, which the L2 model uses) gives the same (representative, member);
  * every move of the orbit -- a generator pair flip, any same-filling configuration of a quad-active block -- leads to a
    prefix with the same representative;
  * member ids are distinct within an orbit, the orbit is exactly as large as its radices say and at most 2^capacity;
  * every prefix lies in exactly one orbit: the representative is a member of its own orbit, with member id 0.
With no eligible block and a capacity of FO bits the key equals the odd-pair rule the planner used before (restated in the
program), for every P, also at the flagship's p = 20."""
import importlib.util
import os
import subprocess
from collections import defaultdict

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("orbit_key") / "orbit_key_host")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "spindynamics.jl_amd", "csrc"),
           os.path.join(ROOT, "tests", "orbit_key_host.cpp"), "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


@pytest.fixture(scope="module")
def restatement():
    spec = importlib.util.spec_from_file_location("orbit_key_restatement", os.path.join(ROOT, "profiles", "orbit_key.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def table(exe, p, quad_blocks, cap_tenths):
    r = subprocess.run([exe, "table", str(p), str(quad_blocks), str(cap_tenths)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    rows = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert [row[0] for row in rows] == list(range(1 << p))
    return [(rep, member) for _, rep, member in rows]


@pytest.mark.parametrize("quad_blocks", [0, 2, 99])
@pytest.mark.parametrize("cap_tenths", [62, 72])
@pytest.mark.parametrize("p", [8, 10, 11, 12])
def test_orbit_key_is_consistent(exe, restatement, p, cap_tenths, quad_blocks):
    key = table(exe, p, quad_blocks, cap_tenths)
    orbits = defaultdict(list)
    for P in range(1 << p):
        rep, member, moves = restatement.orbit_key(P, p, quad_blocks, cap_tenths)
        assert key[P] == (rep, member), f"P={P:#x}: C++ {key[P]}, Python {(rep, member)}"
        assert bin(rep).count("1") == bin(P).count("1")              # same prefix filling: same tile length
        for Q in restatement.neighbours(P, moves):
            assert key[Q][0] == rep, f"P={P:#x} -> Q={Q:#x} leaves the orbit"
        size = 1
        for mv in moves:
            size *= 2 if mv[0] == "pair" else restatement.QUAD_COUNT[mv[2]]
        orbits[rep].append((member, size))
    assert sum(len(v) for v in orbits.values()) == 1 << p            # every prefix in exactly one orbit
    quad_active = 0
    for rep, members in orbits.items():
        ids = sorted(mem for mem, _ in members)
        size = members[0][1]
        assert all(s == size for _, s in members)
        assert ids == list(range(size)), f"orbit {rep:#x}: member ids {ids} for size {size}"      # distinct, dense from 0
        assert size <= 2 ** (cap_tenths / 10)
        assert key[rep] == (rep, 0)
        quad_active += size % 3 == 0
    assert (quad_active > 0) == (quad_blocks > 0)                    # a six-configuration block is what brings a factor 3


@pytest.mark.parametrize("p,FO", [(8, 6), (10, 6), (11, 6), (12, 6), (12, 5), (20, 6), (20, 5), (7, 6), (2, 6)])
def test_no_eligible_block_is_the_odd_pair_rule(exe, p, FO):
    r = subprocess.run([exe, "pairs", str(p), str(FO)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.split() == ["equal", str(1 << p)]
