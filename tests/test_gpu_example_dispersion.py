"""examples/dispersion.py end to end on the GPU: the Heisenberg ring at L = 16, the ground state's labels and the lowest level of
every momentum sector by projected Lanczos.  Checked: the ground state of a ring with L = 4 m has momentum 0 and is even under R and
Z; the lowest of the sector levels is the ground-state energy (bar 1e-8: both are 150-step Lanczos values across a gap of 0.27);
E(k) = E(-k); every excitation lies above the des Cloizeaux-Pearson edge (pi/2)|sin k| of the infinite chain and within 0.35 of it
(sparse ED of the ring at L = 16 on the CPU: the lift grows from 0.018 at k = 2 pi/16 to 0.270 at k = pi)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_dispersion_example():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "dispersion.py")], cwd=ROOT, capture_output=True,
                       text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    L = 16
    gs = re.search(r"ground state: E0 = (\S+), momentum n = (\S+), parity = (\S+), spin flip = (\S+)", r.stdout)
    assert gs and (gs.group(2), gs.group(3), gs.group(4)) == ("0", "1", "1"), r.stdout
    E0 = float(gs.group(1))
    rows = re.findall(r"level\s+(\d+)\s+(\S+)\s+(\S+)\s+(\S+)\s+(\S+)", r.stdout)
    assert [int(x[0]) for x in rows] == list(range(L))
    E = np.array([float(x[2]) for x in rows])
    edge = np.array([float(x[4]) for x in rows])
    assert abs(E.min() - E0) <= 1e-8 and int(np.argmin(E)) == 0
    assert np.abs(E[1:] - E[1:][::-1]).max() <= 1e-7                       # E(k) = E(2 pi - k)
    gap = E - E0
    assert np.all(gap[1:] >= edge[1:] - 1e-9) and np.all(gap[1:] <= edge[1:] + 0.35)
