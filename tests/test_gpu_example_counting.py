"""examples/domain_wall_counting.py end to end on the GPU: the domain wall of the open XXZ chain at L = 16 melts under Chebyshev steps;
the printed identities hold -- the mean of the right half's counting statistics is the sum of magnetization_per_site over it (1e-12,
the script's own check), the transferred magnetisation starts at 0 and grows, P and the snapshot histogram are distributions over
0..L/2 up spins, and the number entropy printed at the end is that of the last line of the table."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_domain_wall_counting_example():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "domain_wall_counting.py")], cwd=ROOT, capture_output=True,
                       text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    L, steps, shots = 16, 20, 4096
    table = re.findall(r"^\s*(\d+\.\d\d)\s+(\d+\.\d{6})\s+(\d+\.\d{6})\s+(\d+\.\d{6})\s+(\S+e[-+]\d+)$", r.stdout, flags=re.M)
    assert len(table) == steps + 1, r.stdout
    t, moved, var, sn, gap = (np_col(table, k) for k in range(5))
    assert t[0] == 0.0 and moved[0] == 0.0 and var[0] == 0.0 and sn[0] == 0.0          # the domain wall is a basis state
    assert max(gap) <= 1e-12
    assert moved[-1] > 0.5 and all(b >= a - 1e-9 for a, b in zip(moved[:8], moved[1:9]))   # the wall melts, monotonically at first
    assert 0.0 < sn[-1] < math.log(L // 2 + 1) and var[-1] > 0.01
    rows = re.findall(r"^\s+(\d+)\s+(\d\.\d{6})\s+(\d\.\d{6})$", r.stdout, flags=re.M)
    assert [int(x[0]) for x in rows] == list(range(L // 2 + 1))
    P, H = [float(x[1]) for x in rows], [float(x[2]) for x in rows]
    assert abs(sum(P) - 1.0) <= 1e-5 and abs(sum(H) - 1.0) <= 1e-5
    assert all(round(h * shots) == pytest.approx(h * shots, abs=1e-2) for h in H)      # counts of 4096 snapshots
    final = float(re.search(r"number entropy of the right half: (\S+)", r.stdout).group(1))
    assert abs(final - sn[-1]) <= 1e-6
    worst = float(re.search(r"worst \|mean from P - sum of magnetization_per_site\|: (\S+)", r.stdout).group(1))
    assert worst <= 1e-12


def np_col(table, k):
    return [float(row[k]) for row in table]
