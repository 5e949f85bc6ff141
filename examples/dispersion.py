#!/usr/bin/env python3
"""The lowest level at every momentum of the Heisenberg ring, L = 16, nup = 8, beside the des Cloizeaux-Pearson edge
E0 + (pi/2) |sin(k - k0)| of the infinite chain (k0: the ground state's momentum) -- the lower edge S(q, w) is read against -- and
the quantum numbers of the ground state.  Each level is one Lanczos run restricted to its momentum sector: the start vector is
P_n (random) and every step applies P_n H, one pass of the projector kernel per step.  `L` may be raised
(python examples/dispersion.py 20)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g

sd = g.load_package()
L = int(sys.argv[1]) if len(sys.argv) > 1 else 16
model = sd.XXZChain(L, Jxy=1.0, Jz=1.0, nup=L // 2, boundary="periodic")
print("Heisenberg ring L = %d, nup = %d, dimension %d; T, R, Z symmetric: %s %s %s" % (
    L, L // 2, len(model), sd.is_symmetric(model, shift=1), sd.is_symmetric(model, reflect=True), sd.is_symmetric(model, flip=True)))

t0 = time.time()
E0, psi = sd.groundstate(model, lanc_m=150)
qn = sd.quantum_numbers(np.asarray(psi), model)
print("ground state: E0 = %.10f, momentum n = %s, parity = %s, spin flip = %s  (%.2f s)" % (
    E0, qn["momentum"], qn["parity"], qn["spin_flip"], time.time() - t0))
print("   momentum weights: " + " ".join("%.3f" % w for w in qn["expectation"]["weights"]))

t0 = time.time()
k = sd.momenta(model)
k0 = k[qn["momentum"]]
levels = [sd.lowest_level(model, lanc_m=150, momentum=n, seed=n) for n in range(L)]
print("lowest level per momentum (%.2f s):" % (time.time() - t0))
print("    n      k/pi       E(k)        E(k) - E0   (pi/2)|sin(k - k0)|")
for n in range(L):
    print("level %3d  %8.4f  %12.8f  %10.6f  %10.6f" % (n, k[n] / np.pi, levels[n], levels[n] - E0, 0.5 * np.pi * abs(np.sin(k[n] - k0))))
print("lowest of all sectors: %.10f at n = %d" % (min(levels), int(np.argmin(levels))))
