"""examples/finite_temperature.py end to end on the GPU, at its default L = 16 and at L = 12, where it prints the deviation from the
dense trace next to the standard error.  No statistical assertion: one random state of N = 924 states deviates by about its
standard error; the per-sample identities are asserted in tests/test_gpu_typicality.py."""
import math
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "finite_temperature.py"), *args], cwd=ROOT,
                       capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "typicality_correlation_function:" in r.stdout
    return r.stdout


def test_finite_temperature_example():
    out = run()
    assert "L = 16" in out and "dense deviation" not in out


def test_finite_temperature_example_prints_the_dense_deviation_at_L12():
    out = run("12", "3")
    mt = re.search(r"dense deviation: (\S+)", out)
    assert mt, out
    assert math.isfinite(float(mt.group(1)))
