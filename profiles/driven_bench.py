"""Times a stage of the driven evolution against the Krylov propagator it is built on, and the drive pass alone.

XXZ chain (open, Jz = 0.7), half filling, ComplexF64, kry_m = 30.  Device events around each call, one warm-up, then --reps runs,
every run printed.  Per size one JSON line:
  driven_stage_ms   one stage of sd_driven_evolve_dev with a gradient and a zz drive (kry_m applies, each followed by the drive pass)
  krylov_ms         one sd_krylov_evolve_dev at the same kry_m (the fused two-launch step where the plan allows it)
  drive_pass_ms     sd_diag_apply_dev with y = out: the drive kernel alone, three streams of 16 bytes per row
  drive_pass_GBps   48 bytes per row over that time

    python profiles/driven_bench.py --L 24 28
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

from pair_correlations_bench import timed  # noqa: E402


def runs(fn, reps):
    med, lo, hi = timed(fn, reps)
    return {"median": med, "min": lo, "max": hi}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="+", default=[24, 28])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kry_m", type=int, default=30)
    a = ap.parse_args()
    import numpy as np
    import torch
    pkg = g.load_package()
    for L in a.L:
        m = pkg.XXZChain(L, Jxy=1.0, Jz=0.7, nup=L // 2, boundary="open")
        dev = torch.device("cuda", m.ctx.device)
        psi = torch.empty(m.N, dtype=torch.complex128, device=dev)
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, psi.data_ptr(), 2 * m.N, 7, 0), m.ctx.h)
        psi /= torch.linalg.vector_norm(psi)
        drives = [pkg.gradient_drive(m), pkg.zz_drive(m)]
        tau, coef = np.array([0.05]), np.array([[0.3, 0.2]])
        stage = runs(lambda: pkg.stage_evolve(m, psi, drives, tau, coef, kry_m=a.kry_m), a.reps)
        kry = runs(lambda: pkg.krylov_time_evolve(psi, 0.05, pkg.apply_H, m, kry_m=a.kry_m), a.reps)
        buf = psi.clone()
        dp = runs(lambda: pkg.diagonal_apply(psi, m, drives, coef[0], y=buf, out=buf), a.reps)
        rec = {"L": L, "nup": L // 2, "N": m.N, "path": m.device_path, "kry_m": a.kry_m, "reps": a.reps, "driven_stage_ms": stage,
               "krylov_ms": kry, "stage_over_krylov": stage["median"] / kry["median"], "drive_pass_ms": dp,
               "drive_pass_GBps": 48.0 * m.N / (dp["median"] * 1e-3) / 1e9,
               "drive_share_of_stage": a.kry_m * dp["median"] / stage["median"]}
        print(json.dumps(rec), flush=True)
        del psi, buf
        torch.cuda.empty_cache()
        m.ctx.release_scratch()


if __name__ == "__main__":
    main()
