"""examples/driven_chain.py end to end on the GPU at its small sizes (one magnon on 20 sites, a half-filled chain of 12).

The magnon's centre of mass returns after the Bloch period 2 pi / E.  Tolerance: the one of tests/test_gpu_driven_evolve.py -- 8 times
the deviation of the existing krylov_time_evolve from the dense propagator of H0 on the same model, with the example's stage
duration, kry_m = 30 and 16 calls -- scaled by L: |x(T) - x(0)| <= sum_i i |p_i(T) - p_i(0)| <= L * 2 |psi(T) - psi_exact(T)|, and the
chain's ends add about J_9(1)^2 = 3e-17.  Measured on an MI355X: floor 8.23e-15, |x(T) - x(0)| = 1.60e-14 (allowed 1.32e-12).
The second part's identities: <H0> never falls below the ground-state energy, the norm stays 1, energy is absorbed."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_driven_chain_example(pkg):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "driven_chain.py")], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    L, E, stages = 20, 1.0, 16
    # the floor: the parent's Krylov propagator against the dense one on the example's model (H0 from the apply, column by column)
    m = pkg.XXZChain(L, Jxy=1.0, Jz=0.5, hz=0.0, nup=1, boundary="open")
    H0 = np.empty((m.N, m.N))
    for k in range(m.N):
        e = np.zeros(m.N)
        e[k] = 1.0
        H0[:, k] = pkg.apply_H(np.empty(m.N), e, m)
    assert np.array_equal(H0, H0.T)
    psi0 = np.zeros(m.N, dtype=np.complex128)
    for site in (L // 2, L // 2 + 1):
        psi0[m.rank(np.array([1 << (site - 1)], dtype=np.uint64))[0]] = 1.0 / math.sqrt(2.0)
    tau = 2.0 * math.pi / E / stages
    psi = psi0
    for _ in range(stages):
        psi = pkg.krylov_time_evolve(psi, tau, pkg.apply_H, m, kry_m=30)
    w, v = np.linalg.eigh(H0)
    floor = float(np.linalg.norm(psi - v @ (np.exp(-1j * w * tau * stages) * (v.T @ psi0))))
    table = re.findall(r"^\s+(\d\.\d{4})\s+(\d+\.\d{12})$", r.stdout, flags=re.M)
    assert len(table) == stages + 1 and float(table[0][0]) == 0.0 and float(table[-1][0]) == 1.0
    x = [float(row[1]) for row in table]
    back = float(re.search(r"return after one period: \|x\(T\) - x\(0\)\| = (\S+)", r.stdout).group(1))
    print(f"floor {floor:.2e}; |x(T) - x(0)| = {back:.2e} (allowed {8 * floor * L:.2e})")
    assert abs(x[0] - (L + 1) / 2) <= 1e-12
    assert back <= 8 * floor * L
    assert abs(abs(x[stages // 2] - x[0]) - 1.0 / E) <= 1e-9           # half a period away: Jxy / E sites (the ladder's closed form)
    # the absorbed energy
    rows = re.findall(r"^\s+(\d+\.\d{3})\s+(-?\d\.\d{10}e[-+]\d+)\s+(\d\.\d\de[-+]\d+)$", r.stdout, flags=re.M)
    assert len(rows) == 9 and float(rows[0][0]) == 0.0 and float(rows[-1][0]) == 4.0
    absorbed = [float(a) for _t, a, _n in rows]
    assert abs(absorbed[0]) <= 1e-9 and min(absorbed) >= -1e-9 and absorbed[-1] > 1e-6
    assert max(float(n) for _t, _a, n in rows) <= 1e-12
