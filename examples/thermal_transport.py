#!/usr/bin/env python3
"""Thermal transport by dynamical quantum typicality: the energy-current autocorrelation <J_E(t) J_E>_beta on a ring of L = 14
sites in the S^z = 0 sector, for the XXZ chain at Delta = 1 and for a J1-J2 ring.

J_E = (i/2) sum_{a,b} (x_b - x_a) [h_a, h_b] is a sum of three-site operators (energy_current_terms).  On the periodic XXZ chain at
zero field it commutes with H (Zotos, Naef, Prelovsek), so the correlation function does not move in time -- a flat line, to
rounding: ballistic heat transport, a finite thermal Drude weight.  A second-neighbour bond breaks the conservation law and the
curve decays.  python examples/thermal_transport.py [L] [n_samples]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g

sd = g.load_package()
L = int(sys.argv[1]) if len(sys.argv) > 1 else 14
n_samples = int(sys.argv[2]) if len(sys.argv) > 2 else 4
beta, J2 = 0.5, 0.4
times = np.linspace(0.0, 6.0, 13)
op = ("energy_current", "periodic")

xxz = sd.XXZChain(L, Jxy=1.0, Jz=1.0, nup=L // 2, boundary="periodic")
hop = [(i, i % L + 1, 0.5) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2 / 2) for i in range(1, L + 1)]
zz = [(i, i % L + 1, 1.0) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2) for i in range(1, L + 1)]
j1j2 = sd.build_model(L, nup=L // 2, hopping=hop, zz=zz)
print("rings of L = %d sites, S^z = 0: N = %d, beta = %.1f, %d samples" % (L, len(xxz), beta, n_samples))
for name, m in (("XXZ, Delta = 1", xxz), ("J1-J2, J2 = %.1f" % J2, j1j2)):
    tl = sd.energy_current_terms(m, "periodic")
    print("  %-16s J_E has %3d terms in %3d bond groups" % (name + ":", len(tl), len({(t["i"], t["j"]) for t in tl})))

t0 = time.time()
C1 = sd.typicality_correlation_function(xxz, beta, op, op, times, n_samples=n_samples, seed=1)
C2 = sd.typicality_correlation_function(j1j2, beta, op, op, times, n_samples=n_samples, seed=1)
print("typicality_correlation_function: %.3f s for two models x %d samples x %d times" % (time.time() - t0, n_samples, len(times)))

print("\n   t     XXZ Re <J_E(t)J_E>/L  +- stderr   | J1-J2 Re <J_E(t)J_E>/L  +- stderr")
for k, t in enumerate(times):
    print("%5.2f   %18.12f   %9.2e   |   %18.12f   %9.2e" % (t, C1[k].real / L, C1.stderr[k].real / L, C2[k].real / L,
                                                              C2.stderr[k].real / L))
flat = np.abs(np.asarray(C1) - C1[0]).max() / abs(C1[0])
decay = np.abs(np.asarray(C2) - C2[0]).max() / abs(C2[0])
print("\nXXZ ring: max |C(t) - C(0)| / C(0) = %.3e (conserved)" % flat)
print("J1-J2 ring: max |C(t) - C(0)| / C(0) = %.3e (decays)" % decay)
assert np.isfinite(np.asarray(C1)).all() and np.isfinite(np.asarray(C2)).all()
assert flat < 1e-9 < 1e-3 < decay
