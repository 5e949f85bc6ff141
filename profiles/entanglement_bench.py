"""Times the block Gram kernels of the entanglement across a chain cut next to the library's own squared norm of the
same vector: the norm is one read of psi and therefore the floor where the blocks are small; where they are large the figure of merit
is the FP64 rate 8 sum_m d^2 K / 2 flop (the upper triangle of complex multiply-adds) per second.

XXZ open, half filling, ComplexF64 (Float64 with --f64), side auto.  Per (L, cut) one JSON line: the device time of the Gram kernels
and the reduction alone (sd_cut_gram_time_dev: two events around the launches; plan, table upload and the copy of the blocks to the
host are outside), warm-up first, median of --reps runs; the norm the same way around sd_nrm2sq_dev.

    python profiles/entanglement_bench.py --L 28 30 32
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402
from pair_correlations_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="+", default=[28, 30, 32])
    ap.add_argument("--cuts", type=int, nargs="*", default=None, help="default: 2, 8, L/2, L-8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--f64", action="store_true")
    a = ap.parse_args()
    import torch
    pkg = g.load_package()
    for L in a.L:
        nup = L // 2
        m = pkg.XXZChain(L, Jxy=1.0, Jz=1.0, nup=nup, boundary="open")
        dev = torch.device("cuda", m.ctx.device)
        nc = 1 if a.f64 else 2
        psi = torch.empty(m.N, dtype=torch.float64 if a.f64 else torch.complex128, device=dev)
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, psi.data_ptr(), nc * m.N, 7, 0), m.ctx.h)
        psi /= torch.linalg.vector_norm(psi)
        out = C.c_double(0.0)

        def norm():
            pkg.check(pkg.lib().sd_nrm2sq_dev(m.ctx.h, nc, psi.data_ptr(), m.N, C.byref(out)), m.ctx.h)
        norm_ms, _, _ = timed(norm, a.reps)
        for cut in (a.cuts or [2, 8, L // 2, L - 8]):
            blocks = pkg.cut_blocks(m, cut)
            items, max_ns, ws = pkg.cut_plan_info(m, cut, dtype="complex128" if nc == 2 else "float64")
            flop = sum((8 if nc == 2 else 2) * b.d * b.d * (b.dB if b.side == "A" else b.dA) / 2 for b in blocks)
            ms = C.c_double(0.0)
            runs = []
            for r in range(a.reps + 1):                                   # the first run is the warm-up
                pkg.check(pkg.lib().sd_cut_gram_time_dev(m.ctx.h, m.h, nc, psi.data_ptr(), m.N, cut, 2, C.byref(ms)), m.ctx.h)
                runs.append(ms.value)
            med = statistics.median(runs[1:])
            print(json.dumps({"L": L, "nup": nup, "N": m.N, "dtype": "f64" if a.f64 else "c128", "cut": cut,
                              "sides": "".join(sorted({b.side for b in blocks})), "d_max": max(b.d for b in blocks),
                              "K_max": max(b.dB if b.side == "A" else b.dA for b in blocks), "items": items, "max_ns": max_ns,
                              "workspace_MB": ws / 1e6, "gram_ms": med, "gram_min_max": (min(runs[1:]), max(runs[1:])),
                              "norm_ms": norm_ms, "x_norm": med / norm_ms, "GBps_psi": 8 * nc * m.N / med / 1e6,
                              "TFLOPs": flop / med / 1e9}), flush=True)
        del psi
        torch.cuda.empty_cache()
        m.ctx.release_scratch()


if __name__ == "__main__":
    main()
