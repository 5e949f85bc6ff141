#!/usr/bin/env python3
"""Entanglement across the chain, both standard uses: open XXZ chain, L = 16, nup = 8, Jz = 1.
1. A quench from the Neel state, evolved with Chebyshev steps: after every step the half-chain entanglement entropy S_1(t) -- from the
   blocks of the reduced density matrix, one Gram kernel pass per cut -- with the number entropy S_N beside it, the part of S_1 that
   the counting statistics of section 20 already gave.  S_1 starts at 0 (a product state), grows linearly until the light cone reaches
   the ends, and 0 <= S_N <= S_1 <= ln 2^(L/2) throughout.
2. The ground state: the entanglement profile S_1(l), l = 1..L-1, beside the conformal form (c/6) ln[(2L/pi) sin(pi l/L)] + const with
   c = 1 (the constant is the mean difference; the open chain adds the familiar even-odd oscillation around it).
python examples/entanglement_growth.py [L] [steps]"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g

sd = g.load_package()
L = int(sys.argv[1]) if len(sys.argv) > 1 else 16
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
dt = 0.25
model = sd.XXZChain(L, Jxy=1.0, Jz=1.0, hz=0.0, nup=L // 2, boundary="open")
psi = np.asarray(sd.neel_state(model)).astype(np.complex128)
half = L // 2
cap = math.log(2.0) * min(half, L - half)
print("Hilbert-space dimension: %d; cut between sites %d and %d; blocks (m, dA, dB): %s" % (
    len(model), half, half + 1, " ".join("(%d,%d,%d)" % (b.m, b.dA, b.dB) for b in sd.cut_blocks(model, half))))
print("   t      S_1         S_N         S_1 - S_N   Schmidt gap")
for n in range(steps + 1):
    if n:
        psi = sd.time_evolve(model, psi, dt, method="chebyshev", cheb_n=30, Ebounds=(-0.75 * L, 0.75 * L))
    sr = sd.symmetry_resolved_entanglement(psi, model, half)
    S1, SN = sr["S_total"], sr["S_number"]
    print("%5.2f  %10.8f  %10.8f  %10.8f  %10.8f" % (n * dt, S1, SN, S1 - SN, sd.schmidt_gap(psi, model, half)))
    assert -1e-12 <= SN <= S1 + 1e-12 and S1 <= cap + 1e-12
E0, gs = sd.groundstate(model, lanc_m=300)          # converged well below the accuracy of the entropies
prof = sd.entanglement_profile(gs, model)
ell = np.arange(1, L)
cft = (1.0 / 6.0) * np.log((2.0 * L / math.pi) * np.sin(math.pi * ell / L))
const = float((prof - cft).mean())
print("ground state E0 = %.10f; entanglement profile:  l   S_1(l)       (1/6) ln[(2L/pi) sin(pi l/L)] + %.4f" % (E0, const))
for k in range(L - 1):
    print("   %2d  %14.12f  %10.8f" % (ell[k], prof[k], cft[k] + const))
print("largest |S_1(l) - S_1(L - l)|: %.3e" % float(np.abs(prof - prof[::-1]).max()))
