#!/usr/bin/env python3
"""The low end of the spectrum with lowest_eigenpairs / spectral_gap / lowest_levels (thick-restart Lanczos).

1. The gap of the open Heisenberg chain (nup = L/2) against L: it closes like 1/L.
2. The Majumdar-Ghosh ring (J2 = J1/2, periodic): the ground state is twofold, E0 = -3 L J1 / 8, and a single Lanczos sequence
   holds only one combination of the two; the solver's confirmation step finds the second.  The dimer correlation matrix of
   each of the two returned states, and S_D(pi) of both.
3. The lowest level of every momentum sector of the Heisenberg ring from lowest_levels: the tower the two ground states of
   part 2 sit in at k = 0 and k = pi.

`L` of parts 2 and 3 may be raised (python examples/low_spectrum.py 16)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g

sd = g.load_package()
L = int(sys.argv[1]) if len(sys.argv) > 1 else 12

print("open Heisenberg chain: gap against L")
for Lc in (8, 12, 16):
    model = sd.XXZChain(Lc, nup=Lc // 2)
    t0 = time.time()
    E0, gap, deg = sd.spectral_gap(model)
    print("   L = %2d: E0 = %.10f  gap = %.10f  L * gap = %.6f  degeneracy %d  (%.2f s)" % (Lc, E0, gap, Lc * gap, deg, time.time() - t0))

print("Majumdar-Ghosh ring, L = %d" % L)
J1, J2 = 1.0, 0.5
site = lambda i: (i - 1) % L + 1          # noqa: E731
hop = [(i, site(i + 1), J1 / 2) for i in range(1, L + 1)] + [(i, site(i + 2), J2 / 2) for i in range(1, L + 1)]
zz = [(i, site(i + 1), J1) for i in range(1, L + 1)] + [(i, site(i + 2), J2) for i in range(1, L + 1)]
ring = sd.build_model(L, nup=L // 2, hopping=hop, zz=zz, onsite_field=np.zeros(L))
E, X, info = sd.lowest_eigenpairs(ring, k=2)
print("   levels: %.10f %.10f  next level: %.10f  exact E0 = %.4f" % (E[0], E[1], info["next_level"], -3 * L * J1 / 8))
print("   residuals: %.2e %.2e  applies: %d  restarts: %d  vectors held: %d" % (info["residuals"][0], info["residuals"][1],
                                                                              info["applies"], info["restarts"], info["workspace_vectors"]))
nn = [(i, site(i + 1)) for i in range(1, L + 1)]
for s in range(2):
    psi = np.ascontiguousarray(X[:, s])
    Dm = sd.dimer_correlation_matrix(psi, ring, bonds=nn)
    sdpi = sd.dimer_structure_factor(psi, ring, np.pi, bonds=nn)[0]
    print("   state %d: D_11 = %.6f  D_12 = %.6f  D_13 = %.6f  S_D(pi) = %.6f" % (s, Dm[0, 0].real, Dm[0, 1].real, Dm[0, 2].real, sdpi))
E0, split, deg = sd.spectral_gap(ring)
print("   spectral_gap: E0 = %.10f  E1 - E0 = %.2e  degeneracy %d  gap above the multiplet = %.10f" % (E0, split, deg, info["next_level"] - E[0]))

print("Heisenberg ring, L = %d: lowest level per momentum" % L)
heis = sd.XXZChain(L, nup=L // 2, boundary="periodic")
for n in range(L):
    En, _ = sd.lowest_levels(heis, 1, momentum=n)
    print("   k = 2 pi %2d / %d: E = %.10f" % (n, L, En[0]))
