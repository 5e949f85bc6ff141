"""examples/dimer_order.py end to end on the GPU: the open J1-J2 chain at L = 20, J2/J1 = 0 and 0.5, ground states by Lanczos, bond
energies and S_D(pi) from the dimer matrix.  At the Majumdar-Ghosh point the printed values are those of the singlet product
(bar 1e-6 on what a 150-step Lanczos state gives: its energy converges to far below that across a gap of 0.4 J1); the Heisenberg
chain's S_D(pi) stays well below it."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dimer_order_example():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dimer_order.py")], cwd=ROOT, capture_output=True,
                       text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    L, B = 20, 19
    blocks = re.findall(r"J2/J1 = (\S+): dimension \d+, E0 = (\S+) .*\n\s+bond energies: (.*)\n\s+S_D\(pi\) = (\S+)", r.stdout)
    assert [b[0] for b in blocks] == ["0.0", "0.5"], r.stdout
    heis, mg = blocks
    e = [float(x) for x in mg[2].split()]
    assert len(e) == B and abs(float(mg[1]) + 3 * L / 8) <= 1e-6
    assert max(abs(x - (-0.75 if b % 2 == 0 else 0.0)) for b, x in enumerate(e)) <= 1e-6
    exact = ((L / 2) ** 2 * 9 / 16 + (L / 2 - 1) * 3 / 16) / B
    assert abs(float(mg[3]) - exact) <= 1e-6 * B
    assert 0.0 < float(heis[3]) < 0.5 * exact and len(heis[2].split()) == B
