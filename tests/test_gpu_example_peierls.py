"""examples/peierls_pulse.py end to end on the GPU at its default size (half-filled open chain of 8 sites, 400 steps).

The absorbed energy equals the work of the pulse, <H0>(T) - E0 = int dA/dt <dH/dA> dt with dH/dA = -sin A T_1 + cos A J_1, up to the
error of the trapezoid rule that takes the integral.  Tolerance, from halving the step on the dense oracle (recorded in the example):
the trapezoid sum is 0.223046831 at 200 steps and 0.223058128 at 400, Richardson puts its error at 400 steps at a third of the
difference, and the whole difference 1.13e-5 is allowed.  The absorbed energy itself is 0.223061893 in dense arithmetic at every step
count from 100 to 800; the device run may differ by the ground state's own error (the example allows 1e-9 there) and the print's nine
decimals: 1e-7."""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_peierls_pulse_example():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "peierls_pulse.py")], cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    absorbed = float(re.search(r"absorbed energy <H0>\(T\) - E0 = ([-0-9.e+]+)", r.stdout).group(1))
    work = float(re.search(r"work int dA/dt <dH/dA> dt   = ([-0-9.e+]+)", r.stdout).group(1))
    src = open(os.path.join(ROOT, "examples", "peierls_pulse.py")).read()
    assert float(re.search(r"^TOLERANCE = ([0-9.e-]+)", src, flags=re.M).group(1)) == 1.13e-5
    print(f"absorbed {absorbed:.9f} work {work:.9f} difference {abs(absorbed - work):.3e} (allowed 1.13e-5)")
    assert abs(absorbed - work) <= 1.13e-5
    assert abs(absorbed - 0.223061893) <= 1e-7
    assert abs(work - 0.223058128) <= 1e-7                   # the same trapezoid sum as the dense oracle's
