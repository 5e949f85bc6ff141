"""Times the energy current against one plain apply of the same model.

XXZ ring, ComplexF64, half filling.  Device events around each call, warm-up first, median of --reps runs.  Per size one JSON
line: the write form (energy_current into a caller's output through sd_dcurrent_apply_dev), the bracket form
(energy_current_expectation), one apply (sd_bench_apply_dev), and the ratios of the write form to one apply and to two applies.

    python profiles/energy_current_bench.py --L 28
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
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    pkg = g.load_package()
    for L in a.L:
        nup = L // 2
        m = pkg.XXZChain(L, Jxy=1.0, Jz=1.0, nup=nup, boundary="periodic")
        terms = pkg.energy_current_terms(m, "periodic")
        groups = len({(int(t["i"]), int(t["j"])) for t in terms})
        dev = torch.device("cuda", m.ctx.device)
        psi = torch.empty(m.N, dtype=torch.complex128, device=dev)
        out = torch.empty_like(psi)
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, psi.data_ptr(), 2 * m.N, 7, 0), m.ctx.h)
        ms = C.c_float(0.0)
        pkg.check(pkg.lib().sd_bench_apply_dev(m.ctx.h, m.h, 2, psi.data_ptr(), out.data_ptr(), m.N, 4, C.byref(ms)), m.ctx.h)
        applies = []
        for _ in range(a.reps):
            pkg.check(pkg.lib().sd_bench_apply_dev(m.ctx.h, m.h, 2, psi.data_ptr(), out.data_ptr(), m.N, 4, C.byref(ms)), m.ctx.h)
            applies.append(ms.value)
        pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, psi.data_ptr(), 2 * m.N, 7, 0), m.ctx.h)   # the ping-pong overwrote psi
        pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, out.data_ptr(), 2 * m.N, 8, 0), m.ctx.h)
        apply_ms = statistics.median(applies)
        bra = out.clone()

        def write():
            pkg.check(pkg.lib().sd_dcurrent_apply_dev(m.ctx.h, m.h, 2, psi.data_ptr(), m.N, terms.ctypes.data, len(terms), out.data_ptr()),
                      m.ctx.h)
        wr = timed(write, a.reps)
        br = timed(lambda: pkg.energy_current_expectation(bra, psi, m, terms), a.reps)
        ratio2 = wr[0] / (2 * apply_ms)
        rec = {"L": L, "nup": nup, "N": m.N, "terms": len(terms), "groups": groups, "path": m.device_path, "apply_ms": apply_ms,
               "write_ms": wr[0], "write_min_max": wr[1:], "bracket_ms": br[0], "bracket_min_max": br[1:],
               "write_in_applies": wr[0] / apply_ms, "write_over_two_applies": ratio2, "target_4x_two_applies": "missed" if ratio2 > 4 else "met"}
        print(json.dumps(rec), flush=True)
        del psi, out, bra
        torch.cuda.empty_cache()
        m.ctx.release_scratch()


if __name__ == "__main__":
    main()
