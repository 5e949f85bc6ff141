#!/usr/bin/env python3
"""Dynamical quantum typicality on one MI355X, one JSON line per size.  Periodic XXZ chain, S^z = 0, beta = 1,
current-current correlation, automatic cheb_n, K uniform time steps.  Host clock around calls that end in a stream
synchronisation, warm, median of 5.
  step_ms          (T(K + 1 time points) - T(1 time point)) / K of sd_dqt_correlations: evolution of both states + measurement
  measure_ms       the same difference with all K + 1 times EQUAL (no evolution): the measurement (current bracket) alone
  evolve_ms        step_ms - measure_ms
  fixed_ms         T(1 time point at t = 0): start vector, imaginary-time step, energy, B psi, one measurement and THE read-back
                   (one copy of 16 nA nt bytes at the end of the call; not separable from the host side)
  *_unbatched      the same with sd_ctx_set_q_batch(0)
  two_evolves_ms   the comparison point: sd_chebyshev_evolve_dev called twice with the same dt, cheb_n and bounds
  bracket_ms       sd_current_bracket_dev on two device vectors (weights upload and the 16-byte read-back included);
  bracket_GBps     its two-stream algorithmic bytes (16 + 16 B/row) over that time
Usage: python profiles/typicality_bench.py [L ...]     (defaults 24 28)"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import scipy.special as ss
import torch
import __graft_entry__ as g

pkg = g.load_package()
K, DT, BETA, REPS = 4, 0.5, 1.0, 5


def med_ms(fn, reps=REPS, warm=1):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts)


def auto_terms(z):
    k = int(np.floor(z)) + 1
    while not abs(ss.jv(k, z)) < 2.0 ** -53:
        k += 1
    return k


def run(L):
    m = pkg.XXZChain(L, Jz=1.0, nup=L // 2, boundary="periodic")
    Eb = (-0.45 * L, 0.26 * L)                    # contains the spectrum: E0/L > -0.4432, Emax = L/4
    a = (Eb[1] - Eb[0]) / (2 * 0.9999)
    cheb_n = auto_terms(a * DT)
    J = ("current", None)
    moving, still = [DT * k for k in range(K + 1)], [0.0] * (K + 1)
    out = {"L": L, "N": m.N, "K": K, "dt": DT, "beta": BETA, "cheb_n_real_time": cheb_n, "path": m.device_path}

    def dqt(times):
        return lambda: pkg.dqt_sample(m, BETA, J, J, times, seed=3, Ebounds=Eb)

    for tag, on in (("", True), ("_unbatched", False)):
        m.ctx.set_q_batch(on)
        t1 = med_ms(dqt([0.0]))
        tk = med_ms(dqt(moving))
        ts = med_ms(dqt(still))
        out["fixed_ms" + tag] = round(t1, 4)
        out["step_ms" + tag] = round((tk - t1) / K, 4)
        out["measure_ms" + tag] = round((ts - t1) / K, 4)
        out["evolve_ms" + tag] = round((tk - ts) / K, 4)
    m.ctx.set_q_batch(True)
    dev = torch.device("cuda", m.ctx.device)
    rng = np.random.default_rng(1)
    psi = torch.as_tensor(rng.standard_normal(m.N) + 1j * rng.standard_normal(m.N), device=dev)
    psi /= torch.linalg.vector_norm(psi)
    phi = pkg.spin_current(psi, m)

    def two():
        pkg.chebyshev_time_evolve(psi, DT, pkg.apply_H, m, cheb_n=cheb_n, Ebounds=Eb)
        pkg.chebyshev_time_evolve(phi, DT, pkg.apply_H, m, cheb_n=cheb_n, Ebounds=Eb)

    out["two_evolves_ms"] = round(med_ms(two), 4)
    tb = med_ms(lambda: pkg.current_expectation(psi, phi, m))
    out["bracket_ms"] = round(tb, 4)
    out["bracket_GBps"] = round(32.0 * m.N / (tb * 1e-3) / 1e9, 1)
    out["apply_write_ms"] = round(med_ms(lambda: pkg.spin_current(psi, m)), 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    for L in [int(x) for x in sys.argv[1:]] or [24, 28]:
        run(L)
