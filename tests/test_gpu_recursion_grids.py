"""The vector kernels of the recursions (csrc/kernels_blas1.hip) at the sizes where their capped launch grids wrap: a second and later
pass of a workgroup through its grid-stride loop, the tail blocks, the 64-bit index arithmetic.  Below these sizes -- where every
other recursion test against the oracle runs (L <= 20, N <= 184 756) -- each grid covers its vector in one pass.

Caps (the launchers' constants) and the shapes that cross them:
  16384 blocks of 256 (grid_for, RED_BLOCKS)   ComplexF64: N = C(25,12) = 5 200 300 elements > 4 194 304
                                               Float64, counted in pairs (items = n / 2): n = C(26,13) = 10 400 600 doubles
  1024 blocks (sd_k_gs_blocks, items = N / 2)  N = C(22,11) = 705 432: 1378 blocks wanted
  256 fat blocks (sd_k_lanczos_fold_blocks)    N = 705 432: 345 blocks of 2048 elements wanted
Cells (15):
  sd_dot_dev, sd_nrm2sq_dev   c128 at 5 200 300, f64 at 10 400 600: random vectors against math.fsum of the kernel's own terms,
                              unit-vector probes on both sides of the wrap (exact), same call twice (equal bits)          4
  sd_fill_randn_dev           4 206 649 doubles (> 16384 * 256), first_index 0 and 987 654 321: against the same stream filled
                              piece by piece below the cap                                                                 2
                              against sd_fill_randn_host, bit for bit                                                      2
  lanczos_tridiag             L=22 nup=11, lanc_m=6, against the oracle (k_lanczos_fold_p, one vector)                     1
  lanczos_sqw                 L=22 nup=11, three momenta in one batch against one at a time (k_lanczos_fold_p, grid.y = 3) 1
  lanczos_groundstate         L=22 nup=11, lanc_m=18, blocked and column by column; once with orthogonalize_tol=1e-18      2
                              L=23 nup=11, lanc_m=10 (k_gs_scale past its 2048 blocks)                                     1
  krylov / chebyshev / lanczos_tridiag at L=25 nup=12 (k_lanczos_fold, k_ccombine, k_cheb_init, k_ew2, k_promote)          2

The recursion cells compare whole recursions at the project's bars.  The vector kernels themselves -- every pass of the ground-state
chain (k_gs_pass, k_gs_update, k_gs_correct, k_gs_scale past its 2048 blocks), k_mdot, k_gemv_cols, k_ccombine and the elementwise
passes past their 16384 blocks -- are pinned one launcher at a time, bit for bit or under rigorous bounds, in
tests/test_gpu_blas1_kernels.py; the fold family (sd_k_lanczos_fold, sd_k_lanczos_fold_p and the two kernels that file the last
step's scalars: all twelve update kernels, every branch of the paired streaming loop, every list length and batch layout) likewise in
tests/test_gpu_fold_kernels.py.  At L=22 a single Lanczos vector takes k_lanczos_fold_p (the launch-bound form, up to 2^22 rows); the
streaming k_lanczos_fold wraps in the L=25 cells.

Run time: the oracle on the CPU is what these cells wait for (a few applies at 5.2 M rows, 18 Lanczos steps at 0.7 M), not the
GPU; the shapes are the smallest that cross the caps."""
import ctypes as C
import gc
import math
from math import comb

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
# constants of csrc/kernels_blas1.hip
BS = 256
RED_BLOCKS = 16384                 # grid_for / RED_BLOCKS: most blocks of a streaming pass
GS_BLOCKS = 1024                   # sd_k_gs_blocks, over N / 2 items
GS_SCALE_BLOCKS = 2048             # sd_k_gs_scale, over N / 2 items
FOLD_BLOCKS, FOLD_ROWS = 256, 2048  # sd_k_lanczos_fold_blocks: at most 256 blocks of >= 2048 elements
FUSED_MAX = 1 << 22                # lanczos_fused_ok (csrc/recur.cpp): the launch-bound form up to 2^22 rows
CAP = RED_BLOCKS * BS

N_C = comb(25, 12)
N_R = comb(26, 13)
XXZ = dict(Jxy=0.9, Jz=0.7, hz=0.3)


def cvec(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def fill_randn(pkg, ctx, n_doubles, seed, first=0, cplx=False):
    import torch
    x = torch.empty(n_doubles // 2 if cplx else n_doubles, dtype=torch.complex128 if cplx else torch.float64,
                    device=torch.device("cuda", ctx.device))
    ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    pkg.check(pkg.lib().sd_fill_randn_dev(ctx.h, x.data_ptr(), n_doubles, seed, first), ctx.h)
    torch.cuda.synchronize()
    return x


def dot(pkg, ctx, x, y):
    o = (C.c_double * 2)(float("nan"), float("nan"))
    pkg.check(pkg.lib().sd_dot_dev(ctx.h, pkg._lib.SD_C128 if x.is_complex() else pkg._lib.SD_F64, x.data_ptr(), y.data_ptr(), len(x), o),
              ctx.h)
    return (float(o[0]), float(o[1])) if x.is_complex() else (float(o[0]),)


def nrm2sq(pkg, ctx, x):
    o = C.c_double(float("nan"))
    pkg.check(pkg.lib().sd_nrm2sq_dev(ctx.h, pkg._lib.SD_C128 if x.is_complex() else pkg._lib.SD_F64, x.data_ptr(), len(x), C.byref(o)), ctx.h)
    return float(o.value)


def sum_check(what, got, terms):
    """|got - fsum(terms)| <= n 2^-53 sum |term_i|: the worst case of any order of n - 1 double additions of these terms"""
    exact = math.fsum(terms.tolist())
    bar = len(terms) * 2.0 ** -53 * math.fsum(np.abs(terms).tolist())
    print(f"{what}: |got - fsum| = {abs(got - exact):.2e} (bound {bar:.2e}, |sum| {abs(exact):.2e})")
    assert abs(got - exact) <= bar, (what, got, exact, bar)


@pytest.fixture(scope="module")
def big(pkg):
    """two random vectors of each element type past the 16384-block cap, on the device and on the host"""
    import torch
    ctx = pkg.default_context()
    v = {}
    for cplx, n, seed in ((True, N_C, 11), (False, N_R, 21)):
        x = fill_randn(pkg, ctx, 2 * n if cplx else n, seed, cplx=cplx)
        y = fill_randn(pkg, ctx, 2 * n if cplx else n, seed + 1, cplx=cplx)
        assert x.data_ptr() % 16 == 0 and y.data_ptr() % 16 == 0           # the Float64 kernels take their 16-byte loop
        v[cplx] = (x, y, x.cpu().numpy(), y.cpu().numpy())
    yield ctx, v
    v.clear()
    gc.collect()
    torch.cuda.empty_cache()


def items_and_rows(cplx, n):
    """the launcher's item count (ComplexF64 elements, or PAIRS of doubles) and the probe elements: item 0, the last item of the
    first pass, the first of the second, one in the last partial block, the last"""
    items = n if cplx else n // 2
    assert items > CAP and (cplx or n % 2 == 0)
    last_block = (items - 1) // BS * BS
    assert last_block > CAP and items - last_block < BS                     # a partial block, in the second pass
    picks = [0, CAP - 1, CAP, last_block + (items - last_block) // 2, items - 1]
    return items, picks if cplx else [2 * i + k for i, k in zip(picks, (0, 1, 0, 1, 1))]


@pytest.mark.parametrize("cplx", [True, False], ids=["c128", "f64"])
def test_dot_past_the_block_cap(pkg, big, cplx):
    import torch
    ctx, v = big
    x, y, xh, yh = v[cplx]
    n = len(x)
    items, rows = items_and_rows(cplx, n)
    # random vectors: the kernel's terms in the kernel's operation order, summed exactly
    got = dot(pkg, ctx, x, y)
    if cplx:
        terms = (xh.real * yh.real + xh.imag * yh.imag, xh.real * yh.imag - xh.imag * yh.real)       # conj(x) y
    else:
        terms = (xh[0::2] * yh[0::2] + xh[1::2] * yh[1::2],)                                           # one term per 16-byte pair
    for k, t in enumerate(terms):
        assert len(t) == items
        sum_check(f"dot {'c128' if cplx else 'f64'} part {k}", got[k], t)
    assert dot(pkg, ctx, x, y) == got                                       # same call twice: equal bits (no NaN: == is bits)
    # probes: x = e_r picks y[r]; every other term is an exact zero
    e = torch.zeros_like(x)
    for r in rows:
        e[r] = 1.0
        g = dot(pkg, ctx, e, y)
        want = (yh[r].real, yh[r].imag) if cplx else (yh[r],)
        assert g == tuple(float(w) for w in want), (cplx, r, g, want)
        e[r] = 0.0


@pytest.mark.parametrize("cplx", [True, False], ids=["c128", "f64"])
def test_nrm2sq_past_the_block_cap(pkg, big, cplx):
    import torch
    ctx, v = big
    x, _, xh, _ = v[cplx]
    items, rows = items_and_rows(cplx, len(x))
    got = nrm2sq(pkg, ctx, x)
    terms = xh.real * xh.real + xh.imag * xh.imag if cplx else xh[0::2] * xh[0::2] + xh[1::2] * xh[1::2]
    assert len(terms) == items
    sum_check(f"nrm2sq {'c128' if cplx else 'f64'}", got, terms)
    assert nrm2sq(pkg, ctx, x) == got
    # probes: one non-zero element, its square (sum of squares) rounded as the kernel rounds it
    e = torch.zeros_like(x)
    for r in rows:
        e[r] = x[r]
        val = xh[r]
        want = float(val.real * val.real + val.imag * val.imag) if cplx else float(val * val)
        assert nrm2sq(pkg, ctx, e) == want, (cplx, r)
        e[r] = 0.0


FILL_N, FILL_SEED = CAP + 12345, 20261019


@pytest.mark.parametrize("first", [0, 987_654_321])
def test_fill_randn_past_the_block_cap_equals_pieces_below_the_cap(pkg, first):
    """element k of a stream depends on (seed, first_index + k) alone, so one call past 16384 blocks equals, to the bit, the same
    stream filled in pieces that each stay in one pass of the grid"""
    import torch
    ctx = pkg.default_context()
    piece = 1 << 20
    assert FILL_N > CAP and piece <= CAP
    got = fill_randn(pkg, ctx, FILL_N, FILL_SEED, first)
    pieces = torch.cat([fill_randn(pkg, ctx, min(piece, FILL_N - lo), FILL_SEED, first + lo) for lo in range(0, FILL_N, piece)])
    bad = (got != pieces).nonzero().flatten()
    assert len(bad) == 0, (first, len(bad), bad[:8].tolist())
    assert bool(torch.isfinite(got).all()) and abs(float(got.mean())) < 0.01 and abs(float(got.std()) - 1.0) < 0.01


@pytest.mark.parametrize("first", [0, 987_654_321])
def test_fill_randn_past_the_block_cap_equals_the_host_stream(pkg, first):
    """sd_fill_randn_dev against sd_fill_randn_host, bit for bit: both evaluate sd_randn (csrc/randn.hpp), whose logarithm and
    cosine are written out in IEEE operations, so the host and the device round every step alike.  (With the math libraries'
    own log and cos 164 501 of these 4 206 649 elements differed by one ulp, from element 18 on.)"""
    ctx = pkg.default_context()
    assert FILL_N > CAP
    g = fill_randn(pkg, ctx, FILL_N, FILL_SEED, first).cpu().numpy()
    host = np.empty(FILL_N)
    assert pkg.lib().sd_fill_randn_host(host.ctypes.data_as(_dp), FILL_N, FILL_SEED, first) == 0
    bad = np.nonzero(g != host)[0]
    print(f"fill_randn first_index={first}: {len(bad)} of {FILL_N} elements differ from the host stream; max |diff| {np.abs(g - host).max():.2e}")
    assert len(bad) == 0, (len(bad), bad[:8].tolist(), g[bad[:4]].tolist(), host[bad[:4]].tolist())


# ---- the Lanczos update passes past 256 fat blocks ----
@pytest.fixture(scope="module")
def chain22(pkg, O):
    L, nup = 22, 11
    m = pkg.XXZChain(L, nup=nup, **XXZ)
    r = O.XXZChain(L, nup=nup, **XXZ)
    assert m.N == 705_432 and m.device_path == "tiled"
    yield m, r
    gc.collect()


def test_lanczos_tridiag_past_the_fat_block_cap_vs_oracle(pkg, O, chain22):
    m, r = chain22
    assert (m.N + FOLD_ROWS - 1) // FOLD_ROWS > FOLD_BLOCKS and m.N <= FUSED_MAX and len(m.local_tiles()[0]) <= 4096
    v = cvec(m.N, 5)
    al, be, nv = pkg.lanczos_tridiag(pkg.apply_H, m, v, lanc_m=6)
    al2, be2, nv2 = O.lanczos_tridiag(r, v, lanc_m=6)
    print(f"lanczos_tridiag L=22: alpha {np.abs(al - al2).max():.2e} beta {np.abs(be - be2).max():.2e}")
    assert len(al) == len(al2) == 6 and abs(nv - nv2) <= 1e-12 * nv2
    assert np.abs(al - al2).max() <= 1e-9 and np.abs(be - be2).max() <= 1e-9       # the bars of test_lanczos_family_vs_oracle


def test_lanczos_sqw_batch_past_the_fat_block_cap_equals_single_recursions(pkg, chain22):
    m, _ = chain22
    assert (m.N + FOLD_ROWS - 1) // FOLD_ROWS > FOLD_BLOCKS and m.N <= FUSED_MAX
    psi = cvec(m.N, 6)
    psi /= np.linalg.norm(psi)
    q = pkg.momenta(m)[1:4]
    omega = np.arange(0.0, 4.0, 0.25)
    try:
        m.ctx.set_q_batch(True)
        n0 = m.ctx.apply_count()
        S_batch = pkg.lanczos_sqw(psi, m, q, omega, lanc_m=6, eta=0.05)
        n_batch = m.ctx.apply_count() - n0
        m.ctx.set_q_batch(False)
        n0 = m.ctx.apply_count()
        S_serial = pkg.lanczos_sqw(psi, m, q, omega, lanc_m=6, eta=0.05)
        assert n_batch == m.ctx.apply_count() - n0
    finally:
        m.ctx.set_q_batch(True)
    assert np.isfinite(S_batch).all() and S_batch.shape == (3, len(omega)) and S_batch.max() > 0
    assert np.array_equal(S_batch, S_serial)


# ---- the ground-state chain past 1024 blocks ----
@pytest.mark.parametrize("otol", [1e-10, 1e-18])
def test_groundstate_chain_past_1024_blocks(pkg, O, chain22, otol):
    """lanc_m = 18: two full blocks of SD_BGS_B = 8 columns and a ragged third.  otol = 1e-18 makes the orthogonality check fire,
    so the correction path runs at this size too."""
    m, r = chain22
    assert (m.N // 2 + BS - 1) // BS > GS_BLOCKS
    x0 = np.random.default_rng(22).standard_normal(m.N)
    E2, _ = O.lanczos_groundstate(r, x0, lanc_m=18, orthogonalize_tol=otol)
    res = {}
    try:
        for blocked in ((True, False) if otol == 1e-10 else (True,)):
            m.ctx.set_gs_blocked(blocked)
            res[blocked], gs = pkg.lanczos_groundstate(pkg.apply_H, m, lanc_m=18, psi0=x0, orthogonalize_tol=otol)
            print(f"groundstate L=22 otol={otol} blocked={blocked}: E - E_oracle = {res[blocked] - E2:.2e}")
            assert abs(res[blocked] - E2) <= 1e-10 and abs(np.linalg.norm(gs) - 1) <= 1e-12
    finally:
        m.ctx.set_gs_blocked(True)
    if False in res:
        assert abs(res[True] - res[False]) <= 1e-12                       # the bars of test_blocked_gram_schmidt_chain_sizes


def test_groundstate_scale_pass_past_2048_blocks(pkg, O):
    L, nup = 23, 11
    m = pkg.XXZChain(L, nup=nup, **XXZ)
    r = O.XXZChain(L, nup=nup, **XXZ)
    assert (m.N // 2 + BS - 1) // BS > GS_SCALE_BLOCKS
    x0 = np.random.default_rng(23).standard_normal(m.N)
    E2, _ = O.lanczos_groundstate(r, x0, lanc_m=10)
    E, gs = pkg.lanczos_groundstate(pkg.apply_H, m, lanc_m=10, psi0=x0)
    print(f"groundstate L=23: E - E_oracle = {E - E2:.2e}")
    assert abs(E - E2) <= 1e-10 and abs(np.linalg.norm(gs) - 1) <= 1e-12


# ---- the streaming passes past 16384 blocks, inside whole recursions ----
@pytest.fixture(scope="module")
def chain25(pkg, O):
    L, nup = 25, 12
    m = pkg.XXZChain(L, nup=nup, **XXZ)
    r = O.XXZChain(L, nup=nup, **XXZ)
    assert m.N == N_C and m.N > CAP and m.N > FUSED_MAX                     # the streaming k_lanczos_fold, not the launch-bound form
    psi0 = cvec(m.N, 25)
    psi0 /= np.linalg.norm(psi0)
    yield m, r, psi0
    gc.collect()


def test_krylov_and_lanczos_past_the_block_cap_vs_oracle(pkg, O, chain25):
    m, r, psi0 = chain25
    got = pkg.krylov_time_evolve(psi0, 0.4, pkg.apply_H, m, kry_m=4)
    err = np.abs(got - O.krylov_time_evolve(r, psi0, 0.4, kry_m=4)).max()
    pr = np.ascontiguousarray(psi0.real) / np.linalg.norm(psi0.real)        # a Float64 state: promoted on the device (k_promote)
    err_r = np.abs(pkg.krylov_time_evolve(pr, 0.4, pkg.apply_H, m, kry_m=4) - O.krylov_time_evolve(r, pr, 0.4, kry_m=4)).max()
    print(f"krylov L=25: {err:.2e} (complex psi0), {err_r:.2e} (real psi0)")
    assert err <= 1e-11 and err_r <= 1e-11                                  # the bar of test_recursions_on_the_per_row_path_vs_oracle
    al, be, nv = pkg.lanczos_tridiag(pkg.apply_H, m, psi0, lanc_m=4)
    al2, be2, nv2 = O.lanczos_tridiag(r, psi0, lanc_m=4)
    print(f"lanczos_tridiag L=25: alpha {np.abs(al - al2).max():.2e} beta {np.abs(be - be2).max():.2e}")
    assert len(al) == 4 and abs(nv - nv2) <= 1e-12 * nv2 and np.abs(al - al2).max() <= 1e-9 and np.abs(be - be2).max() <= 1e-9


def test_chebyshev_past_the_block_cap_vs_oracle(pkg, O, chain25):
    m, r, psi0 = chain25
    Eb = (-m.L / 2, m.L / 2)
    got = pkg.chebyshev_time_evolve(psi0, 0.4, pkg.apply_H, m, cheb_n=3, Ebounds=Eb)
    want = O.chebyshev_time_evolve(r, psi0, 0.4, cheb_n=3, Ebounds=Eb)
    bad = np.nonzero(np.abs(got - want) > 1e-14)[0]
    print(f"chebyshev L=25: {np.abs(got - want).max():.2e}")
    assert len(bad) == 0, (len(bad), bad[:8].tolist())                      # the bar of test_recursions_on_the_per_row_path_vs_oracle
