#!/usr/bin/env python3
"""Dimer order of the open J1-J2 chain from the dimer correlation matrix D_ab = <(S_i . S_j)(S_k . S_l)> over the nearest-neighbour
bonds: L = 20, nup = 10, J2/J1 = 0 (the Heisenberg chain, critical) and 0.5 (the Majumdar-Ghosh point, a product of singlets on
(1,2), (3,4), ...).  For each it prints E0, the bond energies e_b = <S_b . S_b+1> and the dimer structure factor
S_D(pi) = (1/B) sum_ab (-1)^(a-b) D_ab, which grows with the number of bonds B in the dimerised phase: at the Majumdar-Ghosh point
S_D(pi) = [(L/2)^2 9/16 + (L/2 - 1) 3/16] / B exactly.  The two-point matrices of the two chains fall off alike; this tells them
apart.  `L` may be raised (python examples/dimer_order.py 24)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g

sd = g.load_package()
L = int(sys.argv[1]) if len(sys.argv) > 1 else 20
J1 = 1.0
nn = [(i, i + 1) for i in range(1, L)]
B = len(nn)

for ratio in (0.0, 0.5):
    J2 = ratio * J1
    hop = [(i, i + 1, J1 / 2) for i in range(1, L)] + [(i, i + 2, J2 / 2) for i in range(1, L - 1) if J2 != 0.0]
    zz = [(i, i + 1, J1) for i in range(1, L)] + [(i, i + 2, J2) for i in range(1, L - 1) if J2 != 0.0]
    model = sd.build_model(L, nup=L // 2, hopping=hop, zz=zz, onsite_field=np.zeros(L))
    t0 = time.time()
    E0, psi = sd.groundstate(model, lanc_m=150)
    t1 = time.time()
    psi = np.asarray(psi)
    e = sd.bond_energies(psi, model, nn)
    sd_pi = sd.dimer_structure_factor(psi, model, np.pi, bonds=nn)[0]
    print("J2/J1 = %.1f: dimension %d, E0 = %.10f (%.2f s), dimer matrix and S_D in %.3f s" % (ratio, len(model), E0, t1 - t0,
                                                                                             time.time() - t1))
    print("   bond energies: " + " ".join("%.6f" % x for x in e))
    print("   S_D(pi) = %.10f   S_D(pi) / B = %.6f" % (sd_pi, sd_pi / B))
    if ratio == 0.5:
        exact = ((L / 2) ** 2 * 9 / 16 + (L / 2 - 1) * 3 / 16) / B
        print("   singlet product: E0 = %.4f, S_D(pi) = %.10f, bond energies -3/4 and 0 in turn" % (-3 * L / 8, exact))
