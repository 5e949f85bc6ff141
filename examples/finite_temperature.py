#!/usr/bin/env python3
"""Finite-temperature correlation functions by dynamical quantum typicality: the total spin-current autocorrelation
<J(t) J>_beta and <S^z_i(t) S^z_1>_beta of the periodic XXZ chain at beta = 1 in the S^z = 0 sector, from a few random states

    psi_beta = exp(-beta H / 2) r,    <A(t) B>_beta ~ sum_r <psi_beta(t)| A |phi(t)> / sum_r <psi_beta|psi_beta>,   phi = B psi_beta,

with the standard error over the samples.  At L <= 12 the dense trace is printed next to it: one random state of a space of
N = 924 states is NOT typical (the deviation is of the order of the standard error, ~N^(-1/2)); the method needs the large N a
GPU provides.  python examples/finite_temperature.py [L] [n_samples]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g

sd = g.load_package()
L = int(sys.argv[1]) if len(sys.argv) > 1 else 16
n_samples = int(sys.argv[2]) if len(sys.argv) > 2 else 4
beta, Jz = 1.0, 0.5
times = np.linspace(0.0, 4.0, 9)

model = sd.XXZChain(L, Jxy=1.0, Jz=Jz, nup=L // 2, boundary="periodic")
N = len(model)
print("periodic XXZ chain L = %d, Jz = %.2f, S^z = 0: N = %d, beta = %.1f, %d samples" % (L, Jz, N, beta, n_samples))
Ebounds = sd.estimate_energy_bounds(sd.apply_H, model)

t0 = time.time()
CJJ = sd.typicality_correlation_function(model, beta, ("current", None), ("current", None), times, n_samples=n_samples, seed=1,
                                         Ebounds=Ebounds)
Czz = sd.typicality_correlation_function(model, beta, "Sz_all", ("Sz", 1), times, n_samples=n_samples, seed=1, Ebounds=Ebounds)
print("typicality_correlation_function: %.3f s for two correlation functions x %d samples x %d times" % (
    time.time() - t0, n_samples, len(times)))
print("thermal energy per site <H>/L = %.6f" % (float(np.sum(CJJ.den * CJJ.energy) / np.sum(CJJ.den)) / L))

dense = None
if L <= 12:                                     # the exact trace from the dense spectrum
    eye = np.eye(N)
    col = np.empty(N)
    H = np.array([sd.apply_H(col, eye[k], model).copy() for k in range(N)]).T
    J = np.array([sd.spin_current(eye[k], model) for k in range(N)]).T
    st = model.states
    sz = np.array([np.where((st >> np.uint64(i)) & np.uint64(1), 0.5, -0.5) for i in range(L)])
    w, U = np.linalg.eigh(H)
    p = np.exp(-beta * (w - w[0]))
    Jm = U.T @ J @ U
    Sm = np.array([U.T @ (sz[i][:, None] * U) for i in range(L)])

    def trace(Am, Bm, t):                       # Tr(e^{-beta H} e^{iHt} A e^{-iHt} B) / Z in the eigenbasis
        ph = np.exp(1j * w * t)
        return np.sum(p[:, None] * ph[:, None] * Am * ph.conj()[None, :] * Bm.T) / p.sum()

    dense = (np.array([trace(Jm, Jm, t) for t in times]), np.array([[trace(Sm[i], Sm[0], t) for i in range(L)] for t in times]))

print("\n   t     Re <J(t)J>/L   +- stderr   | Re <Sz_1(t)Sz_1>  +- stderr   | Re <Sz_2(t)Sz_1>  +- stderr")
for k, t in enumerate(times):
    print("%5.2f   %12.6f   %9.2e   |   %12.6f   %9.2e   |   %12.6f   %9.2e" % (
        t, CJJ[k].real / L, CJJ.stderr[k].real / L, Czz[k, 0].real, Czz.stderr[k, 0].real, Czz[k, 1].real, Czz.stderr[k, 1].real))
if dense is not None:
    dJ = np.abs(np.asarray(CJJ) - dense[0]).max() / L
    dZ = np.abs(np.asarray(Czz) - dense[1]).max()
    print("\ndense trace (N = %d): max |C_JJ - exact|/L = %.3e (stderr %.3e), max |C_zz - exact| = %.3e (stderr %.3e)" % (
        N, dJ, np.abs(CJJ.stderr).max() / L, dZ, np.abs(Czz.stderr).max()))
    print("dense deviation: %.6e" % max(dJ, dZ))
assert np.isfinite(np.asarray(CJJ)).all() and np.isfinite(np.asarray(Czz)).all() and Czz.shape == (len(times), L)
