"""examples/entanglement_growth.py end to end on the GPU at a reduced step count: the Neel state of the open XXZ chain at L = 16 starts
with S_1 = 0 exactly, 0 <= S_N <= S_1 <= ln min(2^k, 2^(L-k)) holds at every step and the entropy grows; the ground state's entanglement
profile is symmetric under l <-> L - l (the chain is reflection symmetric) within the entropy bar of tests/test_gpu_entanglement.py:
each S_1(l) lies within sum over the eigenvalues of eta(eps) of the exact entropy of the same vector, eps = d (largest entry bound of the
block) / tr, so two mirror cuts differ by at most the sum of their bars (plus the 12 printed decimals)."""
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import entanglement_ref as ER

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def eta(t):
    return -t * math.log(t) if t > 0.0 else 0.0


def entropy_bar(psi, L, nup, cut):
    blocks = ER.gram_blocks(psi, L, nup, cut, "auto")
    tr = sum(float(np.trace(g).real) for g, _ in blocks.values())
    return sum(g.shape[0] * eta(g.shape[0] * float(ER.entry_bound(g, K).max()) / tr) for g, K in blocks.values())


def test_entanglement_growth_example(pkg):
    L, steps = 16, 6
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "entanglement_growth.py"), str(L), str(steps)], cwd=ROOT,
                       capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    table = re.findall(r"^\s*(\d+\.\d\d)\s+(-?\d+\.\d{8})\s+(-?\d+\.\d{8})\s+(-?\d+\.\d{8})\s+(-?\d+\.\d{8})$", r.stdout, flags=re.M)
    assert len(table) == steps + 1, r.stdout
    t, S1, SN, diff, gap = ([float(row[k]) for row in table] for k in range(5))
    assert t[0] == 0.0 and S1[0] == 0.0 and SN[0] == 0.0 and gap[0] == 1.0          # the Neel state is a product state
    cap = math.log(2.0) * (L // 2)
    for a, b in zip(SN, S1):
        assert -1e-8 <= a <= b + 1e-8 and b <= cap + 1e-8                            # 8 printed decimals
    assert S1[-1] > 0.5 and all(y > x for x, y in zip(S1[:4], S1[1:5]))               # entanglement grows after the quench
    rows = re.findall(r"^\s+(\d+)\s+(\d+\.\d{12})\s+(-?\d+\.\d{8})$", r.stdout, flags=re.M)
    assert [int(x[0]) for x in rows] == list(range(1, L))
    prof = np.array([float(x[1]) for x in rows])
    # the bars, from the same ground state (the recursion is deterministic) through the restatement
    model = pkg.XXZChain(L, Jxy=1.0, Jz=1.0, hz=0.0, nup=L // 2, boundary="open")
    E0, gs = pkg.groundstate(model, lanc_m=300)
    bars = np.array([entropy_bar(np.asarray(gs), L, L // 2, cut) for cut in range(1, L)])
    assert np.abs(prof - pkg.entanglement_profile(gs, model)).max() <= 1e-12          # the script's profile is this vector's
    asym = np.abs(prof - prof[::-1])
    print("largest asymmetry %.3e; bars %.3e .. %.3e" % (asym.max(), (bars + bars[::-1]).min(), (bars + bars[::-1]).max()))
    assert (asym <= bars + bars[::-1] + 1e-12).all(), (asym, bars)
    assert prof.min() > 0.0 and abs(prof[0] - math.log(2.0)) <= 1e-8      # a total singlet: one site is maximally mixed
