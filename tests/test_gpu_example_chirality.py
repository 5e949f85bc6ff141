"""examples/chiral_order.py end to end on the GPU: the J1-J2 ring at L = 12 with and without the chiral three-spin term, built
through operator_hamiltonian.  Without it the ground state is real and every chirality printed is zero; with J_chi = 1.5 every
triangle carries the same chirality (the ring is translation invariant), well away from zero and inside the bound 3/8 of one
triangle's spectrum (its eigenvalues are 0 and +-sqrt(3)/4), and the energy lies below the one without the term."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chiral_order_example():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "chiral_order.py")], cwd=ROOT, capture_output=True,
                       text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    L = 12
    blocks = re.findall(r"J_chi = (\S+): dimension (\d+), (\d+) string terms, E0 = (\S+) .*\n\s+chirality per triangle: (.*)\n"
                        r"\s+<chi_1 chi_b>, b = (\S+): (.*)", r.stdout)
    assert [b[0] for b in blocks] == ["0.0", "1.5"], r.stdout
    plain, chiral = blocks
    assert int(plain[1]) == 924 and int(plain[2]) == 0 and int(chiral[2]) == 6 * L
    chi0, chi1 = [float(x) for x in plain[4].split()], [float(x) for x in chiral[4].split()]
    assert len(chi0) == len(chi1) == L
    assert max(abs(x) for x in chi0) <= 1e-9
    assert max(abs(x - chi1[0]) for x in chi1) <= 1e-6 and 0.1 < abs(chi1[0]) <= 0.4331
    assert float(chiral[3]) < float(plain[3])
    far = chiral[5].split(",")
    assert far == [str(b) for b in range(4, 11)] and len(chiral[6].split()) == len(far)
    assert all(abs(float(x)) <= 0.1876 for x in chiral[6].split())
