#!/usr/bin/env python3
"""S(q,w) at every momentum of a periodic chain from ONE Chebyshev recursion: the site-resolved KPM moments
mu_n^{ij} = <psi0| S^z_i T_n(H~) S^z_j |psi0> of a single source site j, Fourier transformed over i, against the per-momentum
recursions of method="kpm".  XXZChain(L=20, nup=10, periodic), groundstate(lanc_m=100), then both methods with the same
rescaling; prints both times, the invariance defect and the largest difference.  `L` may be raised
(python examples/site_correlations.py 24)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g

sd = g.load_package()
L = int(sys.argv[1]) if len(sys.argv) > 1 else 20
kpm_m = int(sys.argv[2]) if len(sys.argv) > 2 else 200

model = sd.XXZChain(L, Jxy=1.0, Jz=1.0, nup=L // 2, boundary="periodic")
print("Hilbert-space dimension:", len(model))
t0 = time.time()
E0, psi0 = sd.groundstate(model, lanc_m=100)
print("groundstate: %.3f s   E0 = %.12f" % (time.time() - t0, E0))

a, b = sd.get_rescaling_params(sd.apply_H, model)
q = sd.momenta(model)
omega = np.linspace(0.0, 5.0, 100)
kw = dict(a=a, b=b, kpm_m=kpm_m, kernel="jackson")
sd.dynamical_structure_factor(model, psi0, q[:2], omega, method="kpm", a=a, b=b, kpm_m=8)          # warm both paths
sd.dynamical_structure_factor(model, psi0, q, omega, method="kpm_sites", translation_invariant=True, a=a, b=b, kpm_m=8)

t0 = time.time()
S = sd.dynamical_structure_factor(model, psi0, q, omega, method="kpm", **kw)
dt = time.time() - t0
print("dynamical_structure_factor(:kpm, kpm_m=%d): %.3f s for %d momenta" % (kpm_m, dt, len(q)))
t0 = time.time()
S1 = sd.dynamical_structure_factor(model, psi0, q, omega, method="kpm_sites", translation_invariant=True, **kw)
dt1 = time.time() - t0
defect = sd.kpm_sqw_sites.last_defect
print("dynamical_structure_factor(:kpm_sites, translation_invariant): %.3f s (x%.1f faster), one source site" % (dt1, dt / dt1))
diff, scale = np.abs(S - S1).max(), np.abs(S).max()
print("invariance defect of the Lanczos ground state: %.2e" % defect)
print("max |S_kpm - S_kpm_sites| = %.3e   relative to max |S| = %.3e: %.3e" % (diff, scale, diff / scale))
C = sd.kpm_correlation_matrix(psi0, model, omega, sources=[1], **kw)
print("local spectral function C_11(w) peaks at w = %.3f; C_{1,1+L/2}(w) ranges over [%.4f, %.4f] (signed)" % (
    omega[np.argmax(C[0, 0].real)], C[L // 2, 0].real.min(), C[L // 2, 0].real.max()))
assert np.isfinite(S1).all() and S1.shape == (len(q), len(omega))
