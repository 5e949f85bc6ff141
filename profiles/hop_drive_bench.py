"""Times the hopping-drive pass beside the kernels it resembles, and a stage of the evolution built on it.

XXZ chain (open, Jz = 0.7), half filling, ComplexF64, the chain's L - 1 bonds.  Device events around each call, one warm-up each,
then --reps rounds; within a round the calls run one after the other, so the yardsticks alternate with the new pass.  Per size one
JSON line, every entry median / min / max in ms:
  hop_real_ms, hop_complex_ms   sd_hop_apply_dev with y = out, real form (the exchange drive) and complex form (the current drive)
  current_ms                    sd_current_apply_dev: the same gathers in write form (no h stream, no own-psi stream)
  apply_ms                      sd_apply_dev
  hop_stage_ms                  one stage of sd_driven_hop_evolve_dev with the two Peierls drives (kry_m applies + the pass each)
  diag_stage_ms                 one stage of sd_driven_evolve_dev with a gradient and a zz drive
  krylov_ms                     one sd_krylov_evolve_dev at the same kry_m
The hop calls upload their table (at most 2.5 KiB) and drain the stream before they return: call overhead is included.

    python profiles/hop_drive_bench.py --L 24 28
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402


def alternating(fns, reps):
    """name -> {median, min, max} in ms; one warm-up of every call, then `reps` rounds through all of them in order"""
    import torch
    for fn in fns.values():
        fn()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ms.items()}


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
        ex, cur = pkg.exchange_drive(m), pkg.current_drive(m)
        peierls, _disp = pkg.peierls_drives(m)
        diag = [pkg.gradient_drive(m), pkg.zz_drive(m)]
        tau = np.array([0.05])
        buf, out = psi.clone(), torch.empty_like(psi)
        one = np.array([1.0])
        passes = alternating({
            "hop_real_ms": lambda: pkg.hopping_apply(psi, m, [ex], one, y=buf, out=buf),
            "current_ms": lambda: pkg.spin_current(psi, m),
            "hop_complex_ms": lambda: pkg.hopping_apply(psi, m, [cur], one, y=buf, out=buf),
            "apply_ms": lambda: pkg.apply_H(out, psi, m),
        }, a.reps)
        stages = alternating({
            "hop_stage_ms": lambda: pkg.stage_evolve(m, psi, peierls, tau, np.array([[-0.1, 0.3]]), kry_m=a.kry_m),
            "diag_stage_ms": lambda: pkg.stage_evolve(m, psi, diag, tau, np.array([[0.3, 0.2]]), kry_m=a.kry_m),
            "krylov_ms": lambda: pkg.krylov_time_evolve(psi, 0.05, pkg.apply_H, m, kry_m=a.kry_m),
        }, a.reps)
        rec = {"L": L, "nup": L // 2, "N": m.N, "path": m.device_path, "bonds": L - 1, "kry_m": a.kry_m, "reps": a.reps}
        rec.update(passes)
        rec.update(stages)
        rec["hop_real_over_current"] = passes["hop_real_ms"]["median"] / passes["current_ms"]["median"]
        rec["hop_complex_over_current"] = passes["hop_complex_ms"]["median"] / passes["current_ms"]["median"]
        rec["hop_stage_over_krylov"] = stages["hop_stage_ms"]["median"] / stages["krylov_ms"]["median"]
        print(json.dumps(rec), flush=True)
        del psi, buf, out
        torch.cuda.empty_cache()
        m.ctx.release_scratch()


if __name__ == "__main__":
    main()
