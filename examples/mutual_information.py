#!/usr/bin/env python3
"""Entanglement between parts of a chain that no cut separates: ground state of the open XXZ chain (Jz = 1), L = 16, nup = 8.
1. The mutual information I({i}:{j}) = S(i) + S(j) - S(ij) of two single sites against their distance |i - j|, measured from a site
   near the middle of the chain: every two-site density matrix comes from the device through one site permutation and the Gram
   kernel of the chain cut.  It falls off with the distance, following the squared spin correlations.
2. The logarithmic negativity E_N = ln ||rho^{T_B}||_1 of two blocks of two sites each against the gap between them: adjacent blocks
   are strongly entangled, and E_N falls off much faster with the gap than the mutual information does -- the mutual information
   also counts classical correlations, the negativity only entanglement.
python examples/mutual_information.py [L]"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g

sd = g.load_package()
L = int(sys.argv[1]) if len(sys.argv) > 1 else 16
model = sd.XXZChain(L, Jxy=1.0, Jz=1.0, hz=0.0, nup=L // 2, boundary="open")
E0, gs = sd.groundstate(model, lanc_m=300)
print("Hilbert-space dimension: %d; ground state E0 = %.10f" % (len(model), E0))
i0 = L // 2 - 1
S_i0 = sd.subsystem_entropy(gs, model, [i0])
print("one-site entropy S(%d) = %.12f (ln 2 = %.12f)" % (i0, S_i0, np.log(2.0)))
print("mutual information of two sites, i = %d:   j  |i-j|  I(i:j)          tr rho_ij" % i0)
for j in range(i0 + 1, L + 1):
    rho = sd.two_site_density_matrix(gs, model, i0, j)
    print("   %2d  %2d  %16.12f  %.12f" % (j, j - i0, sd.mutual_information(gs, model, [i0], [j]), np.trace(rho).real))
A = [i0 - 1, i0]
print("logarithmic negativity of two-site blocks, A = sites %d,%d:   B         gap  E_N" % tuple(A))
for gap in range(0, L - i0 - 1):
    B = [i0 + 1 + gap, i0 + 2 + gap]
    print("   %2d,%2d  %2d  %16.12f" % (B[0], B[1], gap, sd.logarithmic_negativity(gs, model, A, B)))
