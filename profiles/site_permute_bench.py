"""Times the site-permutation kernel next to a device-to-device copy of the same vector, which is one read plus one
write of psi and therefore the floor of any permutation.

XXZ open, half filling, ComplexF64.  Per L one JSON line per permutation: device events around sd_site_permute_dev, warm-up first,
median of --reps runs, and the ratio to the copy timed the same way in the same process.  The permutations:
  middle      a middle block of 8 sites to the front: the plan's suffix sites stay in place, the source rows of a tile are one run
  last        the last 8 sites to the front: every suffix bit moves, the loads are a gather
  alternate   every other site to the front: the same, with no two neighbouring sites kept together
Then the end-to-end time of subsystem_entropy for the middle block next to entanglement_entropy at cut = 8 on the same state (wall
clock around the Python call, the eigensolver on the host included in both).

    python profiles/site_permute_bench.py --L 28 30 32
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


def device_ms(fn, reps):
    """median device time of fn() between two events, after one warm-up call"""
    import torch
    fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        runs.append(e0.elapsed_time(e1))
    return statistics.median(runs), min(runs), max(runs)


def wall_ms(fn, reps):
    fn()
    runs = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        runs.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="+", default=[28, 30, 32])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import numpy as np
    import torch
    pkg = g.load_package()
    for L in a.L:
        nup = L // 2
        m = pkg.XXZChain(L, Jxy=1.0, Jz=1.0, nup=nup, boundary="open")
        dev = torch.device("cuda", m.ctx.device)
        psi = torch.empty(m.N, dtype=torch.complex128, device=dev)
        out = torch.empty_like(psi)
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, psi.data_ptr(), 2 * m.N, 7, 0), m.ctx.h)
        psi /= torch.linalg.vector_norm(psi)
        copy_ms, _, _ = device_ms(lambda: out.copy_(psi), a.reps)
        mid = list(range(5, 13))                      # interior, and below the plan's 12 suffix sites at every L >= 24
        sets = {"middle": mid, "last": list(range(L - 7, L + 1)), "alternate": list(range(1, L + 1, 2))}
        for name, sites in sets.items():
            perm = np.ascontiguousarray(pkg.subsystem_permutation(L, sites), dtype=np.intc)
            pp = perm.ctypes.data_as(C.POINTER(C.c_int))

            def run():
                pkg.check(pkg.lib().sd_site_permute_dev(m.ctx.h, m.h, 2, psi.data_ptr(), m.N, pp, out.data_ptr()), m.ctx.h)
            ms, lo, hi = device_ms(run, a.reps)
            print(json.dumps({"L": L, "nup": nup, "N": m.N, "dtype": "c128", "perm": name, "sites": sites, "permute_ms": ms,
                              "permute_min_max": (lo, hi), "copy_ms": copy_ms, "x_copy": ms / copy_ms,
                              "GBps": 32 * m.N / ms / 1e6}), flush=True)
        del out
        torch.cuda.empty_cache()
        sub = wall_ms(lambda: pkg.subsystem_entropy(psi, m, mid), a.reps)
        cut = wall_ms(lambda: pkg.entanglement_entropy(psi, m, 8), a.reps)
        print(json.dumps({"L": L, "nup": nup, "N": m.N, "dtype": "c128", "subsystem_entropy_middle8_ms": sub,
                          "entanglement_entropy_cut8_ms": cut, "x_cut": sub / cut}), flush=True)
        del psi
        torch.cuda.empty_cache()
        m.ctx.release_scratch()


if __name__ == "__main__":
    main()
