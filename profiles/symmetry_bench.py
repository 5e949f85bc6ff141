"""Times the lattice symmetry operators against one plain apply of the same model.

XXZ ring at half filling, Float64 and ComplexF64.  Device events around each call, warm-up first, median of --reps runs.  Per size
and dtype one JSON line: one translate (T, T^-1, T^(L/2)), reflect, spin_flip, the fused write form, the L-element overlaps
(momentum_weights), the one-pass momentum projector P_n (n = 1: complex coefficients; n = 0: real, a Float64 psi stays Float64)
and, for ComplexF64, the Horner chain of L - 1 fused passes out = T^-1 x + c psi that gives the same P_1 psi (horner_chain),
with its distance from the one-pass result.  Each time is given in ms and in units of one apply_H at that shape on the same run.

    python profiles/symmetry_bench.py --L 28
"""
import argparse
import cmath
import ctypes as C
import json
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

from pair_correlations_bench import timed  # noqa: E402


def horner_chain(pkg, m, psi, n, bufs):
    """P_n psi = (1/L) sum_r z^r T^r psi, z = e^{i k_n}, through L - 1 fused passes: w_0 = psi, w_k = T^-1 w_{k-1} + z^k psi gives
    w_{L-1} = sum_j z^j T^-(L-1-j) psi = z^-1 sum_r z^r T^r psi (T^L = 1, z^L = 1).  Returns (w_{L-1}, z / L)."""
    L = m.L
    z = cmath.exp(2j * math.pi * n / L)
    a, b = bufs
    src = psi
    for k in range(1, L):
        dst = a if src is not a else b
        pkg.symmetry_apply(src, m, shift=-1, y=psi, c=z ** k, out=dst)
        src = dst
    return src, z ** (-(L - 1)) / L                       # P_n psi = factor * w_{L-1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="+", default=[28])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-chain", action="store_true")
    a = ap.parse_args()
    import torch
    pkg = g.load_package()
    for L in a.L:
        nup = L // 2
        m = pkg.XXZChain(L, Jxy=1.0, Jz=1.0, nup=nup, boundary="periodic")
        dev = torch.device("cuda", m.ctx.device)
        for cplx in (False, True):
            code = 2 if cplx else 1
            per = 2 if cplx else 1
            psi = torch.empty(m.N, dtype=torch.complex128 if cplx else torch.float64, device=dev)
            out = torch.empty_like(psi)
            m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, psi.data_ptr(), per * m.N, 7, 0), m.ctx.h)
            psi /= torch.linalg.vector_norm(psi)
            ms = C.c_float(0.0)
            pkg.check(pkg.lib().sd_bench_apply_dev(m.ctx.h, m.h, code, psi.data_ptr(), out.data_ptr(), m.N, 4, C.byref(ms)), m.ctx.h)
            applies = []
            for _ in range(a.reps):
                pkg.check(pkg.lib().sd_bench_apply_dev(m.ctx.h, m.h, code, psi.data_ptr(), out.data_ptr(), m.N, 4, C.byref(ms)), m.ctx.h)
                applies.append(ms.value)
            pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, psi.data_ptr(), per * m.N, 7, 0), m.ctx.h)   # the ping-pong overwrote psi
            psi /= torch.linalg.vector_norm(psi)
            apply_ms = statistics.median(applies)
            rec = {"L": L, "nup": nup, "N": m.N, "dtype": "c128" if cplx else "f64", "path": m.device_path, "apply_ms": apply_ms}

            def put(name, t):
                rec[name + "_ms"] = t[0]
                rec[name + "_min_max"] = t[1:]
                rec[name + "_applies"] = t[0] / apply_ms
            put("translate", timed(lambda: pkg.translate(psi, m, 1, out=out), a.reps))
            put("translate_back", timed(lambda: pkg.translate(psi, m, -1, out=out), a.reps))
            put("translate_half", timed(lambda: pkg.translate(psi, m, L // 2, out=out), a.reps))
            put("reflect", timed(lambda: pkg.reflect(psi, m, out=out), a.reps))
            put("spin_flip", timed(lambda: pkg.spin_flip(psi, m, out=out), a.reps))
            put("fused_translate_back", timed(lambda: pkg.symmetry_apply(psi, m, shift=-1, y=psi, c=0.5, out=out), a.reps))
            put("overlaps_L", timed(lambda: pkg.momentum_weights(psi, m), a.reps))
            pout = torch.empty(m.N, dtype=torch.complex128, device=dev)
            put("project_n1", timed(lambda: pkg.symmetry_project(psi, m, momentum=1, out=pout), a.reps))
            put("project_n0", timed(lambda: pkg.symmetry_project(psi, m, momentum=0, out=out), a.reps))
            if cplx and not a.no_chain:
                bufs = (torch.empty_like(psi), torch.empty_like(psi))
                put("chain_n1", timed(lambda: horner_chain(pkg, m, psi, 1, bufs), max(1, a.reps // 2)))
                w, f = horner_chain(pkg, m, psi, 1, bufs)
                pkg.symmetry_project(psi, m, momentum=1, out=pout)
                rec["chain_vs_one_pass_max_abs"] = float((f * w - pout).abs().max())
                del bufs, w
            print(json.dumps(rec), flush=True)
            del psi, out, pout
            torch.cuda.empty_cache()
            m.ctx.release_scratch()


if __name__ == "__main__":
    main()
