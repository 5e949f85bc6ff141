"""Times the three S^z-basis statistics calls next to the library's own squared norm of the same vector: the norm is
one read of psi and therefore the floor of each of them.

XXZ periodic, half filling, ComplexF64 (and Float64 with --f64).  Device events around each call, warm-up first, median of --reps
runs.  Per size one JSON line: the norm, the moments pass (Shannon, max and q = 2, and with a pow exponent q = 2.5), the counting
statistics of one cut, of all L - 1 cuts and of 64 scattered masks, and 4096 / 65536 snapshots.  The counting and snapshot calls
include the upload of their tables and the synchronisation that returns them to the pool.

    python profiles/basis_stats_bench.py --L 28 30 32
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402
from pair_correlations_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="+", default=[28, 30, 32])
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--f64", action="store_true")
    a = ap.parse_args()
    import torch
    pkg = g.load_package()
    for L in a.L:
        nup = L // 2
        m = pkg.XXZChain(L, Jxy=1.0, Jz=1.0, nup=nup, boundary="periodic")
        dev = torch.device("cuda", m.ctx.device)
        nc = 1 if a.f64 else 2
        psi = torch.empty(m.N, dtype=torch.float64 if a.f64 else torch.complex128, device=dev)
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, psi.data_ptr(), nc * m.N, 7, 0), m.ctx.h)
        psi /= torch.linalg.vector_norm(psi)
        out = C.c_double(0.0)

        def norm():
            pkg.check(pkg.lib().sd_nrm2sq_dev(m.ctx.h, nc, psi.data_ptr(), m.N, C.byref(out)), m.ctx.h)
        cuts = [list(range(1, k + 1)) for k in range(1, L)]
        rng = np.random.default_rng(L)
        scattered = [sorted(rng.choice(np.arange(1, L + 1), size=L // 2, replace=False).tolist()) for _ in range(64)]
        rec = {"L": L, "nup": nup, "N": m.N, "path": m.device_path, "dtype": "f64" if a.f64 else "c128",
               "bytes": 8 * nc * m.N}
        for key, fn in (("norm_ms", norm),
                        ("moments_q2_ms", lambda: pkg.participation_entropy(psi, m, [1, 2, float("inf")])),
                        ("moments_q2_q2.5_ms", lambda: pkg.participation_entropy(psi, m, [1, 2, 2.5])),
                        ("counting_1_cut_ms", lambda: pkg.counting_statistics(psi, m, [cuts[L // 2 - 1]])),
                        ("counting_all_cuts_ms", lambda: pkg.cut_counting_statistics(psi, m)),
                        ("counting_64_scattered_ms", lambda: pkg.counting_statistics(psi, m, scattered)),
                        ("snapshots_4096_ms", lambda: pkg.sample_configurations(psi, m, 4096, seed=1)),
                        ("snapshots_65536_ms", lambda: pkg.sample_configurations(psi, m, 65536, seed=1))):
            med, lo, hi = timed(fn, a.reps)
            rec[key] = med
            rec[key.replace("_ms", "_min_max")] = (lo, hi)
        rec["floor_GBps"] = rec["bytes"] / rec["norm_ms"] / 1e6
        print(json.dumps(rec), flush=True)
        del psi
        torch.cuda.empty_cache()
        m.ctx.release_scratch()


if __name__ == "__main__":
    main()
