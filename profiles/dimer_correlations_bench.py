"""Times the dimer correlation matrix against one plain apply of the same model and against the route it replaces.

XXZ periodic, ComplexF64, half filling, all L nearest-neighbour bonds.  Device events around each call, warm-up first, median of
--reps runs.  Per size one JSON line: the time of dimer_correlation_matrix, the apply time and their ratio; one bond_operator
call; and, with --route-L, at that size the route without the kernel -- B bond_operator calls into B stored vectors and the
B (B + 1) / 2 sd_dot_dev calls of the upper triangle -- with the bytes of the B vectors it has to hold.

    python profiles/dimer_correlations_bench.py --L 28 --route-L 28
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

from pair_correlations_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="+", default=[28])
    ap.add_argument("--route-L", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    pkg = g.load_package()
    for L in a.L:
        nup = L // 2
        m = pkg.XXZChain(L, Jxy=1.0, Jz=1.0, nup=nup, boundary="periodic")
        bonds = pkg.model_bonds(m)
        B = len(bonds)
        dev = torch.device("cuda", m.ctx.device)
        psi = torch.empty(m.N, dtype=torch.complex128, device=dev)
        out = torch.empty_like(psi)
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, psi.data_ptr(), 2 * m.N, 7, 0), m.ctx.h)
        psi /= torch.linalg.vector_norm(psi)
        ms = C.c_float(0.0)
        pkg.check(pkg.lib().sd_bench_apply_dev(m.ctx.h, m.h, 2, psi.data_ptr(), out.data_ptr(), m.N, 4, C.byref(ms)), m.ctx.h)
        applies = []
        for _ in range(a.reps):
            pkg.check(pkg.lib().sd_bench_apply_dev(m.ctx.h, m.h, 2, psi.data_ptr(), out.data_ptr(), m.N, 4, C.byref(ms)), m.ctx.h)
            applies.append(ms.value)
        pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, psi.data_ptr(), 2 * m.N, 7, 0), m.ctx.h)   # the ping-pong overwrote psi
        apply_ms = statistics.median(applies)
        dm = timed(lambda: pkg.dimer_correlation_matrix(psi, m), a.reps)
        bo = timed(lambda: pkg.bond_operator(psi, m, L // 2, L // 2 + 1, out=out), a.reps)
        rec = {"L": L, "nup": nup, "N": m.N, "B": B, "path": m.device_path, "apply_ms": apply_ms, "dimer_ms": dm[0],
               "dimer_min_max": dm[1:], "dimer_in_applies": dm[0] / apply_ms, "bond_operator_ms": bo[0]}
        if L == a.route_L:
            vecs = [torch.empty_like(psi) for _ in range(B)]
            dot = (C.c_double * 2)()

            def route():
                for (i, j), v in zip(bonds, vecs):
                    pkg.bond_operator(psi, m, i, j, out=v)
                for x in range(B):
                    for y in range(x, B):
                        pkg.check(pkg.lib().sd_dot_dev(m.ctx.h, 2, vecs[x].data_ptr(), vecs[y].data_ptr(), m.N, dot), m.ctx.h)
            rt = timed(route, max(1, a.reps // 2))
            rec["route_ms"] = rt[0]
            rec["route_bytes"] = 16 * B * m.N
            rec["route_over_dimer"] = rt[0] / dm[0]
            del vecs
        print(json.dumps(rec), flush=True)
        del psi, out
        torch.cuda.empty_cache()
        m.ctx.release_scratch()


if __name__ == "__main__":
    main()
