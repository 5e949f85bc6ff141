#!/usr/bin/env python3
"""Transverse S(q,w) at full size on one MI355X, one JSON line per item (DESIGN.md "Transverse S(q,w)").
Case: XXZChain L=32, psi0 in sector nup=16 (N_src = 601,080,390), S^-_q into nup=15 (N_dst = 565,722,720), ComplexF64.
  spm_q       the S^-_q kernel (sd_spm_q_dev), algorithmic bytes 16 N_src + 16 N_dst
  apply_dst   one apply of the target sector (sd_bench_apply_dev), 32 B/row
  kpm_zz      one KPM moment pair (one fused apply) of S^zz on the source sector: kpm_sqw at two kpm_m, difference / pairs
  kpm_pm      the same for S^{+-} (kpm_sqw_transverse) on the target sector
Bars: spm_q <= 1.5 x apply_dst; kpm_pm per pair within 10 % of (N_dst / N_src) x kpm_zz per pair.
Usage: python profiles/transverse_bench.py [L]   (L even; default 32)
"""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import __graft_entry__ as g

pkg = g.load_package()
L = int(sys.argv[1]) if len(sys.argv) > 1 else 32
src = pkg.XXZChain(L, nup=L // 2, boundary="periodic")
dst = src.adjacent_sector(-1)
ctx = src.ctx
dev = torch.device("cuda", ctx.device)
q = 2 * np.pi * (L // 4) / L


def ev_time(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    fn()
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize(dev)
    return e0.elapsed_time(e1) / reps


def line(what, ms, nbytes, **kw):
    print(json.dumps(dict(what=what, L=L, N_src=src.N, N_dst=dst.N, ms=round(ms, 4), alg_GBs=round(nbytes / ms / 1e6, 1), **kw)),
          flush=True)


ctx.set_stream(torch.cuda.current_stream(dev).cuda_stream)
psi = torch.randn(src.N, dtype=torch.complex128, device=dev)
phi = torch.empty(dst.N, dtype=torch.complex128, device=dev)


def spm():
    pkg.check(pkg.lib().sd_spm_q_dev(ctx.h, src.h, dst.h, 2, pkg._lib.SD_C128, psi.data_ptr(), src.N, q, phi.data_ptr(), dst.N),
              ctx.h)


t_spm = ev_time(spm, 10)
line("spm_q (S^-_q kernel)", t_spm, 16 * src.N + 16 * dst.N)
del psi
torch.cuda.empty_cache()
b2 = torch.empty(dst.N, dtype=torch.complex128, device=dev)
ms = C.c_float()
pkg.check(pkg.lib().sd_bench_apply_dev(ctx.h, dst.h, pkg._lib.SD_C128, phi.data_ptr(), b2.data_ptr(), dst.N, 2, C.byref(ms)), ctx.h)
pkg.check(pkg.lib().sd_bench_apply_dev(ctx.h, dst.h, pkg._lib.SD_C128, phi.data_ptr(), b2.data_ptr(), dst.N, 10, C.byref(ms)), ctx.h)
t_apply = ms.value
line("apply_dst (one apply of the target sector)", t_apply, 32 * dst.N, spm_over_apply=round(t_spm / t_apply, 3))
del phi, b2
torch.cuda.empty_cache()

psi0 = np.random.default_rng(0).standard_normal(src.N)
psi0 /= np.linalg.norm(psi0)
a, b = L / 2 + 1.0, 0.0
M1, M2 = 32, 160                        # (M2 - M1) / 2 = 64 moment pairs


def per_pair(fn):
    fn(8)                                # warm-up: plans, pool, first touch
    ts = {}
    for M in (M1, M2):
        t0 = time.time()
        fn(M)
        ts[M] = time.time() - t0
    return (ts[M2] - ts[M1]) / ((M2 - M1) / 2) * 1e3


t_zz = per_pair(lambda M: pkg.kpm_sqw(psi0, src, [q], [0.0], a=a, b=b, kpm_m=M))
line("kpm_zz (one moment pair, source sector)", t_zz, 64 * src.N)
t_pm = per_pair(lambda M: pkg.kpm_sqw_transverse(psi0, src, [q], [0.0], component="+-", a=a, b=b, kpm_m=M))
want = dst.N / src.N * t_zz
line("kpm_pm (one moment pair, target sector)", t_pm, 64 * dst.N, expected_ms=round(want, 4),
     pm_over_expected=round(t_pm / want, 3))
