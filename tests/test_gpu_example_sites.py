"""examples/site_correlations.py end to end on the GPU: S(q,w) of the Lanczos ground state of the periodic L = 20 chain by
method="kpm" and by method="kpm_sites", translation_invariant=True.  The Lanczos ground state is translation invariant only
to its residual, so the bar is 1e-6 max|S| here (the dense ground state meets 1e-8 in tests/test_gpu_site_moments.py)."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_site_correlations_example():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "site_correlations.py")], cwd=ROOT, capture_output=True,
                       text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "dynamical_structure_factor(:kpm_sites" in r.stdout
    mt = re.search(r"relative to max \|S\| = \S+: (\S+)", r.stdout)
    assert mt, r.stdout
    assert float(mt.group(1)) <= 1e-6, r.stdout
