#!/usr/bin/env python3
"""A vector-potential pulse on a half-filled chain: the current response and the energy it leaves behind.

Open XXZ chain (Jxy = 1, Jz = 0.7) at half filling, in its ground state.  A uniform vector potential A(t) = A0 sin^2(pi t / T) puts the
Peierls phase e^{i A (j - i)} on every hop S^+_i S^-_j, which is exactly

    H(t) = H0 + (cos A(t) - 1) T_1 + sin A(t) J_1,     T_1 = sum_b t_b (S^+ S^- + h.c.),  J_1 = sum_b i t_b (S^+ S^- - S^- S^+)

(peierls_drives, peierls_functions): two hopping drives with real coefficient functions, propagated by fourth-order commutator-free
Magnus steps (driven_time_evolve).  Measured after every step on the device vector: the current <dH/dA> with

    dH/dA = -sin A T_1 + cos A J_1

(drive_expectation: 2 Re z_b <S^+_i S^-_j> from one pass of the pair kernel) and <H0>.  A(0) = A(T) = 0, so H(0) = H(T) = H0 and the
absorbed energy obeys

    <H0>(T) - E0 = int_0^T dA/dt <dH/dA> dt.

The integral is taken by the trapezoid rule over the steps.  Tolerance of the identity, from halving the step on the dense oracle
(L = 8, A0 = 0.9, T = 2; the left side is 0.223061893 at every step count): the trapezoid sum is 0.223046831 at 200 steps and
0.223058128 at 400, so Richardson puts its error at 400 steps at (I_400 - I_200) / 3 = 3.8e-6 (it is 3.77e-6); the assertion allows
the whole difference |I_400 - I_200| = 1.13e-5.  It holds for the default sizes only; other sizes print the two sides.
python examples/peierls_pulse.py [L] [steps]"""
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g

sd = g.load_package()
L = int(sys.argv[1]) if len(sys.argv) > 1 else 8
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 400
A0, T, every = 0.9, 2.0, 40
TOLERANCE = 1.13e-5          # |I_400 - I_200| of the dense oracle at L = 8: see above

A = lambda t: A0 * math.sin(math.pi * t / T) ** 2                          # noqa: E731
dA = lambda t: A0 * (math.pi / T) * math.sin(2.0 * math.pi * t / T)        # noqa: E731

model = sd.XXZChain(L, Jxy=1.0, Jz=0.7, hz=0.0, nup=L // 2, boundary="open")
drives, disp = sd.peierls_drives(model)
assert disp == [1]
E0, gs = sd.lanczos_groundstate(sd.apply_H, model, lanc_m=min(120, model.N))
print("half-filled chain of %d sites (dimension %d), E0 = %.10f; pulse A(t) = %.2f sin^2(pi t / %.1f), %d steps of order 4" %
      (L, model.N, E0, A0, T, steps))
print("   t       A(t)      <dH/dA>         <H0> - E0")


def record(t, vec):
    eT, eJ = sd.drive_expectation(vec, model, drives)
    cur = -math.sin(A(t)) * eT + math.cos(A(t)) * eJ
    e = sd.instantaneous_energy(vec, model, [], []) - E0
    n2 = float((vec.abs() ** 2).sum())
    return t, cur, e, abs(1.0 - n2)


final, meas = sd.driven_time_evolve(model, gs, drives, sd.peierls_functions(A, disp), 0.0, T / steps, steps, order=4, kry_m=20,
                                    measure=record, measure_every=1)
for (t, cur, e, _n) in meas[::every]:
    print("   %6.3f  %.6f  % .10e  %.10e" % (t, A(t), cur, e))
gvals = np.array([dA(t) * cur for (t, cur, _e, _n) in meas])
work = (T / steps) * (gvals.sum() - 0.5 * (gvals[0] + gvals[-1]))
absorbed = meas[-1][2]
print("absorbed energy <H0>(T) - E0 = %.9f" % absorbed)
print("work int dA/dt <dH/dA> dt   = %.9f (trapezoid over %d steps)" % (work, steps))
print("difference %.3e" % abs(absorbed - work))
assert max(m[3] for m in meas) <= 1e-12 and min(m[2] for m in meas) >= -1e-9
assert abs(meas[0][1]) <= 1e-12                  # no current in the ground state
if (L, steps) == (8, 400):
    assert abs(absorbed - work) <= TOLERANCE, (absorbed, work)
