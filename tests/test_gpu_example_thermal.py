"""examples/thermal_transport.py end to end on the GPU at its default L = 14: the flat line of the XXZ ring and the decaying curve
of the J1-J2 ring.  The bars are asserted in tests/test_gpu_energy_current.py; here the example's own figures are read back."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_thermal_transport_example():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "thermal_transport.py")], cwd=ROOT, capture_output=True,
                       text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "L = 14" in r.stdout and "typicality_correlation_function:" in r.stdout
    flat = float(re.search(r"XXZ ring: max \|C\(t\) - C\(0\)\| / C\(0\) = (\S+)", r.stdout).group(1))
    decay = float(re.search(r"J1-J2 ring: max \|C\(t\) - C\(0\)\| / C\(0\) = (\S+)", r.stdout).group(1))
    assert flat < 1e-9 and decay > 1e-3
