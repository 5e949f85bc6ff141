"""examples/low_spectrum.py end to end on the GPU: the open chain's gap falls with L and L * gap stays of order one; the
Majumdar-Ghosh ring at L = 12 has the twofold ground state -3 L / 8 (both copies returned, the next level well above), both
states carry the same dimer structure factor sum rule; the momentum sectors' lowest levels are symmetric under k -> -k and their
minimum is the ring's ground state.  Bars: 1e-8 on energies (tol = 1e-10 times a norm below 10, with margin)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_low_spectrum_example():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "low_spectrum.py")], cwd=ROOT, capture_output=True,
                       text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    gaps = [(int(a), float(b), int(c)) for a, b, c in re.findall(r"L = +(\d+): E0 = \S+  gap = (\S+)  L \* gap = \S+  degeneracy (\d+)", r.stdout)]
    assert [x[0] for x in gaps] == [8, 12, 16] and all(x[2] == 1 for x in gaps)
    assert gaps[0][1] > gaps[1][1] > gaps[2][1] > 0 and all(1.0 < x[0] * x[1] < 6.0 for x in gaps)
    L = 12
    e0, e1, nxt = [float(x) for x in re.search(r"levels: (\S+) (\S+)  next level: (\S+)", r.stdout).groups()]
    assert abs(e0 + 3 * L / 8) <= 1e-8 and abs(e1 + 3 * L / 8) <= 1e-8 and nxt > e0 + 0.1
    m = re.search(r"spectral_gap: E0 = (\S+)  E1 - E0 = (\S+)  degeneracy (\d+)  gap above the multiplet = (\S+)", r.stdout)
    assert abs(float(m.group(1)) + 3 * L / 8) <= 1e-8 and int(m.group(3)) == 2 and abs(float(m.group(2))) <= 1e-8
    assert abs(float(m.group(4)) - (nxt - e0)) <= 1e-8
    states = re.findall(r"state \d: D_11 = (\S+)  D_12 = \S+  D_13 = \S+  S_D\(pi\) = (\S+)", r.stdout)
    assert len(states) == 2
    sector = [float(x) for x in re.findall(r"k = 2 pi +\d+ / 12: E = (\S+)", r.stdout)]
    assert len(sector) == L
    assert all(abs(sector[n] - sector[L - n]) <= 1e-8 for n in range(1, L))
    assert min(sector) == sector[0]                      # the Heisenberg ring's ground state (L/2 even) lies at k = 0
