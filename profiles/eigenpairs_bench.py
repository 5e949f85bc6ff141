"""Times the thick-restart eigen-solver and its rotation kernel.

XXZ chain, Float64, half filling.  Per size one JSON line: wall time and applies of lowest_eigenpairs(k = 4), the device time
of one apply, of the Gram-Schmidt of one Lanczos step at the mean basis fill (two rounds of block dots and block subtractions
over basis_size / 2 columns) and of one rotation at (m, k) = (24, 10), each the median of --reps runs between device events;
from them the shares of the run spent in applies, Gram-Schmidt and rotations, and the rotation's GB/s against its own byte
count (m + k) N 8.  --gs-L: the same call against lanczos_groundstate(lanc_m = 100) at that size, the earlier way to one
state (orientation only).  --big-L: one lowest_eigenpairs(k = 1, basis_size = 20) run at that size.

    python profiles/eigenpairs_bench.py --L 24 28 --gs-L 28
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

from pair_correlations_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="*", default=[24, 28])
    ap.add_argument("--gs-L", type=int, default=0)
    ap.add_argument("--big-L", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    pkg = g.load_package()
    lib = pkg.lib()
    dp = C.POINTER(C.c_double)
    for L in a.L:
        m = pkg.XXZChain(L, nup=L // 2)
        N, basis, mrot, krot = m.N, 24, 24, 10
        dev = torch.device("cuda", m.ctx.device)
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        pkg.lowest_eigenpairs(m, k=1, vectors=False, max_applies=30)                       # warm-up: code objects, pool
        torch.cuda.synchronize()
        t0 = time.time()
        E, _, info = pkg.lowest_eigenpairs(m, k=4, basis_size=basis, vectors=False)
        wall = time.time() - t0
        V = torch.empty((basis, N), dtype=torch.float64, device=dev)
        w = torch.empty(N, dtype=torch.float64, device=dev)
        pkg.check(lib.sd_fill_randn_dev(m.ctx.h, V.data_ptr(), basis * N, 3, 0), m.ctx.h)
        pkg.check(lib.sd_fill_randn_dev(m.ctx.h, w.data_ptr(), N, 4, 0), m.ctx.h)
        V /= np.sqrt(N)
        ms = C.c_float(0.0)
        applies = []
        for _ in range(a.reps + 1):
            pkg.check(lib.sd_bench_apply_dev(m.ctx.h, m.h, 1, w.data_ptr(), V[0].data_ptr(), N, 4, C.byref(ms)), m.ctx.h)
            applies.append(ms.value)
        apply_ms = statistics.median(applies[1:])
        out, coef = np.zeros(16), np.full(16, 1e-3)

        def gs_step():                       # two rounds over basis / 2 columns, as one Lanczos step at the mean fill
            for _ in range(2):
                for c0 in range(0, basis // 2, 8):
                    nc = min(8, basis // 2 - c0)
                    pkg.check(lib.sd_block_dots_dev(m.ctx.h, 1, V[c0].data_ptr(), N, nc, w.data_ptr(), N, out.ctypes.data_as(dp)), m.ctx.h)
                for c0 in range(0, basis // 2, 8):
                    nc = min(8, basis // 2 - c0)
                    pkg.check(lib.sd_block_axpy_dev(m.ctx.h, 1, w.data_ptr(), V[c0].data_ptr(), N, nc, coef.ctypes.data_as(dp), N), m.ctx.h)
        gs = timed(gs_step, a.reps)
        Q = np.asfortranarray(np.linalg.qr(np.random.default_rng(0).standard_normal((mrot, mrot)))[0][:, :krot])
        rot = timed(lambda: pkg.check(lib.sd_basis_rotate_dev(m.ctx.h, V.data_ptr(), N, N, mrot, Q.ctypes.data_as(dp), krot), m.ctx.h),
                    a.reps)
        steps = info["applies"]
        t_apply, t_gs, t_rot = steps * apply_ms, steps * gs[0], info["restarts"] * rot[0]
        rec = {"L": L, "N": N, "k": 4, "basis_size": basis, "E": [float(x) for x in E], "wall_s": wall, "applies": steps,
               "restarts": info["restarts"], "apply_ms": apply_ms, "gs_step_ms": gs[0], "rotate_ms": rot[0], "rotate_min_max": rot[1:],
               "rotate_GBs": (mrot + krot) * N * 8 / (rot[0] * 1e-3) / 1e9,
               "share_apply": t_apply / (wall * 1e3), "share_gs": t_gs / (wall * 1e3), "share_rotate": t_rot / (wall * 1e3)}
        if L == a.gs_L:
            t0 = time.time()
            E0, _ = pkg.lanczos_groundstate(pkg.apply_H, m, lanc_m=100)
            rec["groundstate_lanc100_s"] = time.time() - t0
            rec["groundstate_E0"] = E0
        print(json.dumps(rec), flush=True)
        del V, w
        torch.cuda.empty_cache()
        m.ctx.release_scratch()
    if a.big_L:
        m = pkg.XXZChain(a.big_L, nup=a.big_L // 2)
        t0 = time.time()
        E, _, info = pkg.lowest_eigenpairs(m, k=1, basis_size=20, vectors=False, confirm=False)
        print(json.dumps({"L": a.big_L, "N": m.N, "k": 1, "basis_size": 20, "E": [float(x) for x in E], "wall_s": time.time() - t0,
                          "applies": info["applies"], "restarts": info["restarts"], "residuals": [float(x) for x in info["residuals"]],
                          "vectors_held": info["workspace_vectors"]}), flush=True)


if __name__ == "__main__":
    main()
