#!/usr/bin/env python3
"""Melting of a domain wall, read in the S^z basis: open XXZ chain, L = 16, nup = 8, Jz = 0.5, starting from domain_wall_state and
evolved with Chebyshev steps.  After every step the full counting statistics P(m) of the number of up spins in the right half give
the magnetisation that has crossed the central bond -- its mean and variance -- and the number entropy S_N = -sum p ln p, the part
of the entanglement entropy that needs no reduced density matrix.  At the last step 4096 projective snapshots are drawn from
|psi|^2, as a quantum-gas microscope would return them, and their right-half histogram is printed next to P.  The script checks
that the mean from P equals the sum of magnetization_per_site over the right half to 1e-12.
python examples/domain_wall_counting.py [L] [steps]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g

sd = g.load_package()
L = int(sys.argv[1]) if len(sys.argv) > 1 else 16
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dt, shots = 0.25, 4096
model = sd.XXZChain(L, Jxy=1.0, Jz=0.5, hz=0.0, nup=L // 2, boundary="open")
psi = np.asarray(sd.domain_wall_state(model)).astype(np.complex128)
right = list(range(L // 2 + 1, L + 1))
m = np.arange(L + 1)
P0 = sd.counting_statistics(psi, model, [right])[0]
start = float((m * P0).sum())                                  # up spins in the right half at t = 0: 0 or L/2
print("Hilbert-space dimension: %d; right half = sites %d..%d holds %d up spins at t = 0" % (len(model), right[0], right[-1], round(start)))
print("   t    transferred  variance   S_N       |mean - sum <Sz_i>|")
worst = 0.0
for n in range(steps + 1):
    if n:
        psi = sd.time_evolve(model, psi, dt, method="chebyshev", cheb_n=30, Ebounds=(-0.75 * L, 0.75 * L))
    P = sd.counting_statistics(psi, model, [right])[0]
    mean, var = sd.magnetization_cumulants(P, right, order=2)
    sz = sd.magnetization_per_site(psi, model)
    norm2 = float(np.vdot(psi, psi).real)
    gap = abs(mean - sz[L // 2:].sum() / norm2)
    worst = max(worst, gap)
    p = P[P > 0]
    print("%5.2f  %10.6f  %9.6f  %8.6f  %.2e" % (n * dt, abs(float((m * P).sum()) - start), var, float(-(p * np.log(p)).sum()) + 0.0, gap))
cfg = sd.sample_configurations(psi, model, shots, seed=2026)
hist = np.bincount((sd.snapshot_spins(cfg, L)[:, L // 2:] > 0).sum(axis=1), minlength=L + 1)
print("right-half up spins at t = %.2f:  m   P(m)      snapshots/%d" % (steps * dt, shots))
for k in range(len(right) + 1):
    print("   %2d  %.6f  %.6f" % (k, P[k], hist[k] / shots))
print("number entropy of the right half: %.10f" % sd.number_entropy(psi, model, right))
print("worst |mean from P - sum of magnetization_per_site|: %.3e" % worst)
assert worst <= 1e-12
assert hist.sum() == shots and hist[len(right) + 1:].sum() == 0
