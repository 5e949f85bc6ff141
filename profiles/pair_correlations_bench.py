"""Times the equal-time pair-correlation matrices against one plain apply of the same model.

XXZ periodic, ComplexF64, half filling.  Device events around each call, warm-up first, median of --reps runs.  Per size one JSON
line: the "+-" and "zz" matrix times, the apply time, and ratio = time("+-") / (nup (L - nup) / L * apply time), the matrix in
units of the gather work of one apply.  --gram-L: also the route without the kernel at that size -- L Sminus_q_vector calls and the
L x L Gram matrix of the results, with the bytes of the L adjacent-sector vectors it has to hold.

    python profiles/pair_correlations_bench.py --L 28 32 --gram-L 28
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def timed(fn, reps):
    import torch
    fn()                                                     # warm-up: code objects, scratch, pool
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="+", default=[28, 32])
    ap.add_argument("--gram-L", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    pkg = g.load_package()
    for L in a.L:
        nup = L // 2
        m = pkg.XXZChain(L, Jxy=1.0, Jz=1.0, nup=nup, boundary="periodic")
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
        pm = timed(lambda: pkg.correlation_matrix(psi, m, "+-"), a.reps)
        zz = timed(lambda: pkg.correlation_matrix(psi, m, "zz"), a.reps)
        unit = nup * (L - nup) / L * apply_ms
        rec = {"L": L, "nup": nup, "N": m.N, "path": m.device_path, "apply_ms": apply_ms, "pm_ms": pm[0], "pm_min_max": pm[1:],
               "zz_ms": zz[0], "zz_min_max": zz[1:], "apply_equivalents": nup * (L - nup) / L, "ratio": pm[0] / unit}
        if L == a.gram_L:
            qs = 2 * torch.pi * torch.arange(L) / L

            def gram():
                V = torch.stack([pkg.Sminus_q_vector(m, psi, float(q)) for q in qs])
                return V.conj() @ V.T
            gm = timed(gram, max(1, a.reps // 2))
            rec["gram_route_ms"] = gm[0]
            rec["gram_route_bytes"] = 16 * L * pkg.XXZChain(L, nup=nup - 1, boundary="periodic").N
        print(json.dumps(rec), flush=True)
        del psi, out
        torch.cuda.empty_cache()
        m.ctx.release_scratch()


if __name__ == "__main__":
    main()
