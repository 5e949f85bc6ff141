"""examples/mutual_information.py end to end on the GPU at L = 12: every printed mutual information and logarithmic negativity of the
ground state against the dense restatement of tests/subsystem_ref.py on the same vector (the recursion is deterministic) -- 12 printed
decimals and the bars of tests/test_gpu_subsystem_entanglement.py, far below them: 1e-10 covers both -- and the physics the script is
there to show: tr rho_ij = 1, I(i:j) > 0 largest for nearest neighbours and smaller at the far end, the negativity of adjacent blocks
above that of every separated pair, nothing negative."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import subsystem_ref as SR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mutual_information_example(pkg):
    L = 12
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "mutual_information.py"), str(L)], cwd=ROOT,
                       capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    i0 = L // 2 - 1
    mi = re.findall(r"^\s+(\d+)\s+(\d+)\s+(-?\d+\.\d{12})\s+(\d+\.\d{12})$", r.stdout, flags=re.M)
    assert [(int(j), int(d)) for j, d, _, _ in mi] == [(j, j - i0) for j in range(i0 + 1, L + 1)]
    en = re.findall(r"^\s+(\d+),\s*(\d+)\s+(\d+)\s+(-?\d+\.\d{12})$", r.stdout, flags=re.M)
    assert [int(g_) for _, _, g_, _ in en] == list(range(0, L - i0 - 1))
    model = pkg.XXZChain(L, Jxy=1.0, Jz=1.0, hz=0.0, nup=L // 2, boundary="open")
    E0, gs = pkg.groundstate(model, lanc_m=300)
    gs = np.asarray(gs.cpu() if hasattr(gs, "cpu") else gs)
    I = [float(x[2]) for x in mi]
    for (j, _, val, tr) in mi:
        assert abs(float(val) - SR.mutual_information(gs, L, L // 2, [i0], [int(j)])) <= 1e-10
        assert abs(float(tr) - 1.0) <= 1e-11
    assert min(I) > 0.0 and I[0] == max(I) and I[-1] < 0.2 * I[0]
    EN = [float(x[3]) for x in en]
    for (b0, b1, _, val) in en:
        assert abs(float(val) - SR.log_negativity(gs, L, L // 2, [i0 - 1, i0], [int(b0), int(b1)])) <= 1e-10
    assert EN[0] > 0.1 and all(-1e-10 <= x < EN[0] for x in EN[1:])
    S = re.search(r"one-site entropy S\(\d+\) = (\d+\.\d{12})", r.stdout)
    assert abs(float(S.group(1)) - math.log(2.0)) <= 1e-8                  # a total singlet: one site is maximally mixed
