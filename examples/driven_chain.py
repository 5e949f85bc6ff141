#!/usr/bin/env python3
"""Driven chains: H(t) = H0 + sum_k f_k(t) D_k with diagonal drives (driven_time_evolve, stage_evolve).

1. Bloch oscillation of one magnon.  Open XXZ chain (Jxy = 1, Jz = 0.5), one up spin, shared equally by the two central sites; at
   t = 0 a static tilt E sum_i (i - (L + 1)/2) S^z_i is switched on (gradient_drive with a constant coefficient: the protocol is
   piecewise constant, so piecewise_schedule is exact up to the Krylov error).  The Wannier-Stark ladder is equidistant with spacing
   E, so the centre of mass x(t) = sum_i i (<S^z_i> + 1/2) swings by Jxy / E sites and returns after the Bloch period 2 pi / E; the
   chain's ends change that by about J_n(Jxy / E)^2 with n the distance to them in sites -- 3e-17 at L = 20, E = 1.
2. Energy absorbed from an a.c. field gradient.  Half-filled XXZ chain in its ground state, f(t) = A sin(w t) on the gradient,
   fourth-order commutator-free Magnus steps; <H0>(t) - E0 is printed every few steps.  A unitary evolution cannot take <H0> below
   the ground-state energy, and the norm stays 1.
python examples/driven_chain.py [L_magnon] [L_chain]"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g

sd = g.load_package()
L1 = int(sys.argv[1]) if len(sys.argv) > 1 else 20
L2 = int(sys.argv[2]) if len(sys.argv) > 2 else 12

# ---- 1. Bloch oscillation ----
E, stages = 1.0, 16
model = sd.XXZChain(L1, Jxy=1.0, Jz=0.5, hz=0.0, nup=1, boundary="open")
tilt = sd.gradient_drive(model)
psi = np.zeros(model.N, dtype=np.complex128)
for site in (L1 // 2, L1 // 2 + 1):
    psi[model.rank(np.array([1 << (site - 1)], dtype=np.uint64))[0]] = 1.0 / math.sqrt(2.0)
sites = np.arange(1, L1 + 1)


def centre(vec):
    return float((sites * (sd.magnetization_per_site(vec, model) + 0.5)).sum())


period = 2.0 * math.pi / E
x0 = centre(psi)
print("one magnon on %d sites, tilt E = %.2f, Bloch period %.6f, %d stages" % (L1, E, period, stages))
print("   t/period   centre of mass")
print("   %8.4f   %.12f" % (0.0, x0))
far = 0.0
for n in range(1, stages + 1):
    psi = sd.stage_evolve(model, psi, [tilt], *sd.piecewise_schedule([(period / stages, [E])]), kry_m=30)
    x = centre(psi)
    far = max(far, abs(x - x0))
    print("   %8.4f   %.12f" % (n / stages, x))
print("largest excursion: %.12f sites (Jxy / E = %.6f)" % (far, 1.0 / E))
print("return after one period: |x(T) - x(0)| = %.3e" % abs(x - x0))

# ---- 2. energy absorbed from an a.c. gradient ----
A, w, dt, steps, every = 0.4, 2.0, 0.05, 80, 10
chain = sd.XXZChain(L2, Jxy=1.0, Jz=0.5, hz=0.0, nup=L2 // 2, boundary="open")
grad = sd.gradient_drive(chain)
E0, gs = sd.lanczos_groundstate(sd.apply_H, chain, lanc_m=min(120, chain.N))
print("half-filled chain of %d sites (dimension %d), E0 = %.10f; a.c. gradient %.2f sin(%.2f t), dt = %.3f, order 4" %
      (L2, chain.N, E0, A, w, dt))
print("   t       <H0> - E0       1 - norm")


def record(t, vec):
    e = sd.instantaneous_energy(vec, chain, [grad], [0.0])
    n2 = float((vec.abs() ** 2).sum())
    print("   %6.3f  %.10e  %.2e" % (t, e - E0, abs(1.0 - n2)))
    return e - E0, abs(1.0 - n2)


final, meas = sd.driven_time_evolve(chain, gs, [grad], [lambda t: A * math.sin(w * t)], 0.0, dt, steps, order=4, kry_m=30,
                                    measure=record, measure_every=every)
absorbed = [m[0] for m in meas]
print("absorbed energy at t = %.2f: %.10e" % (steps * dt, absorbed[-1]))
assert min(absorbed) >= -1e-9 and max(m[1] for m in meas) <= 1e-12
assert absorbed[-1] > 1e-6
