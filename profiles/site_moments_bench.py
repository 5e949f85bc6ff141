#!/usr/bin/env python3
"""Site-resolved KPM moments on one MI355X, one JSON line per item.  hipEvent-timed, warm, median of 7.
  project_c128 / project_f64   the projection pass (sd_site_project_dev: <psi0|S^z_i|v> for all i + |v|^2), ComplexF64 / Float64 bra,
                               algorithmic bytes 32 / 24 per row
  dot_c128 / dot_f64           sd_dot_dev on the same two vectors: the same bytes, 2 sums instead of 2L + 1 (the yardstick)
  nrm2sq                       sd_nrm2sq_dev of the ket (16 B/row), a second stream kernel of the library on the same box
  site_step                    one site-moment step (apply + projection): kpm_site_moments at two M, difference / steps
  kpm_step                     one SD_EPI_KPM step (sd_kpm_step_sharded_dev on the unsharded model, moment-doubling form)
  sqw                          S(q,w) at all momenta of the periodic chain, kpm_m = 1024: kpm_sqw against
                               kpm_sqw_sites(translation_invariant=True) on the Lanczos ground state
Usage: python profiles/site_moments_bench.py stream L [L ...]     (defaults 28 30 32)
       python profiles/site_moments_bench.py sqw L [L ...]        (defaults 20 24)
"""
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import __graft_entry__ as g

pkg = g.load_package()
lib, SD_F64, SD_C128 = pkg.lib(), pkg._lib.SD_F64, pkg._lib.SD_C128
_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
REPS = 7


def med_ms(dev, fn, reps=REPS, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize(dev)
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def stream(L):
    m = pkg.XXZChain(L, nup=L // 2, boundary="periodic")
    ctx = m.ctx
    dev = torch.device("cuda", ctx.device)
    ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
    N = m.N

    def line(what, ms, nbytes, **kw):
        print(json.dumps(dict(what=what, L=L, N=N, ms=round(ms, 4), alg_GBs=round(nbytes / ms / 1e6, 1), **kw)), flush=True)

    ket = torch.randn(N, dtype=torch.complex128, device=dev)
    brac = torch.randn(N, dtype=torch.complex128, device=dev)
    braf = torch.randn(N, dtype=torch.float64, device=dev)
    out = np.empty(2 * L)
    o2 = (C.c_double * 2)()
    t = {}
    for name, bra, code, per in (("c128", brac, SD_C128, 32), ("f64", braf, SD_F64, 24)):
        t["p" + name] = med_ms(dev, lambda: pkg.check(lib.sd_site_project_dev(ctx.h, m.h, code, bra.data_ptr(), ket.data_ptr(), N,
                                                                             out.ctypes.data_as(_dp)), ctx.h))
    t["dc128"] = med_ms(dev, lambda: pkg.check(lib.sd_dot_dev(ctx.h, SD_C128, brac.data_ptr(), ket.data_ptr(), N, o2), ctx.h))
    # the library has no dot of a Float64 bra with a ComplexF64 ket: the Float64 line is the real dot of the bra with itself
    t["df64"] = med_ms(dev, lambda: pkg.check(lib.sd_dot_dev(ctx.h, SD_F64, braf.data_ptr(), braf.data_ptr(), N, o2), ctx.h))
    t["n2"] = med_ms(dev, lambda: pkg.check(lib.sd_nrm2sq_dev(ctx.h, SD_C128, ket.data_ptr(), N, o2), ctx.h))
    line("project_c128", t["pc128"], 32 * N, over_dot=round(t["pc128"] / t["dc128"], 3))
    line("project_f64", t["pf64"], 24 * N, over_dot_c128=round(t["pf64"] / t["dc128"], 3))
    line("dot_c128 (sd_dot_dev, same two vectors)", t["dc128"], 32 * N)
    line("dot_f64 (sd_dot_dev, the Float64 bra with itself, 16 B/row nominal)", t["df64"], 16 * N)
    line("nrm2sq (sd_nrm2sq_dev of the ket)", t["n2"], 16 * N)
    del brac, braf

    # one SD_EPI_KPM step (moment doubling form: no phi stream), ping-pong over three vectors
    v = [ket, torch.randn(N, dtype=torch.complex128, device=dev), torch.empty(N, dtype=torch.complex128, device=dev)]
    a, b = 0.6 * L, 0.0
    state = [0]

    def kpm_step():
        k = state[0]
        state[0] = (k + 1) % 3
        pkg.check(lib.sd_kpm_step_sharded_dev(ctx.h, m.h, v[(k + 2) % 3].data_ptr(), v[(k + 1) % 3].data_ptr(), None, v[k].data_ptr(), None,
                                              N, a, b, 0, o2), ctx.h)
    t_kpm = med_ms(dev, kpm_step)
    del v
    torch.cuda.empty_cache()
    # one site-moment step: kpm_site_moments_dev at two M (v_0, promotion and read-back cancel)
    psi0 = ket
    src = np.array([1], dtype=np.int32)
    M1, M2 = 6, 22

    def moments(M):
        mu = np.empty(2 * M * L)
        pkg.check(lib.sd_kpm_site_moments_dev(ctx.h, m.h, SD_C128, psi0.data_ptr(), N, src.ctypes.data_as(_ip), 1, M, a, b,
                                              mu.ctypes.data_as(_dp)), ctx.h)
    t1 = med_ms(dev, lambda: moments(M1), reps=5, warm=1)
    t2 = med_ms(dev, lambda: moments(M2), reps=5, warm=1)
    t_site = (t2 - t1) / (M2 - M1)
    line("kpm_step (SD_EPI_KPM, 48 B/row)", t_kpm, 48 * N)
    line("site_step (SD_EPI_RECUR apply + projection, 48 + 32 B/row)", t_site, 80 * N, over_kpm_step=round(t_site / t_kpm, 3),
         apply_plus_projection_ms=round(t_kpm + t["pc128"], 4))


def sqw(L):
    m = pkg.XXZChain(L, nup=L // 2, boundary="periodic")
    dev = torch.device("cuda", m.ctx.device)
    E0, psi0 = pkg.groundstate(m, lanc_m=100)
    a, b = pkg.get_rescaling_params(pkg.apply_H, m)
    q = pkg.momenta(m)
    omega = np.linspace(0.0, 5.0, 100)
    kw = dict(a=a, b=b, kpm_m=1024)
    res = {}
    n0 = m.ctx.apply_count()
    t_kpm = med_ms(dev, lambda: res.__setitem__("kpm", pkg.kpm_sqw(psi0, m, q, omega, **kw)), reps=5, warm=1)
    n1 = m.ctx.apply_count()
    t_sites = med_ms(dev, lambda: res.__setitem__("sites", pkg.kpm_sqw_sites(psi0, m, q, omega, translation_invariant=True,
                                                                            ti_tol=float("inf"), **kw)), reps=5, warm=1)
    n2 = m.ctx.apply_count()
    ap_kpm, ap_sites = (n1 - n0) // 6, (n2 - n1) // 6
    diff = float(np.abs(res["kpm"] - res["sites"]).max() / np.abs(res["kpm"]).max())
    print(json.dumps(dict(what="sqw all momenta, kpm_m=1024", L=L, N=m.N, kpm_sqw_ms=round(t_kpm, 2), kpm_sqw_sites_ms=round(t_sites, 2),
                          speedup=round(t_kpm / t_sites, 2), applies_kpm_sqw=ap_kpm, applies_sites=ap_sites,
                          predicted_by_applies=round(ap_kpm / ap_sites, 2), defect=pkg.kpm_sqw_sites.last_defect,
                          rel_diff=diff)), flush=True)


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else "stream"
    Ls = [int(x) for x in sys.argv[2:]] or ([28, 30, 32] if mode == "stream" else [20, 24])
    for L in Ls:
        (stream if mode == "stream" else sqw)(L)
