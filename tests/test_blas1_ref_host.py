"""The yardstick of tests/test_gpu_blas1_kernels.py, proven without a GPU: every function of tests/blas1_ref.py against exact
rational arithmetic rounded once per operation (fractions.Fraction is exact, float(Fraction) is correctly rounded), the two
longdouble chains against Fraction to 2^-60, the chain bound against the double-precision chain it bounds; and the build of
tests/blas1_shim.cpp against the library, with the two pure host functions it reaches checked against their constants."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import blas1_ref as R

N = 300


def mul(x, y):
    return float(Fr(x) * Fr(y))


def add(x, y):
    return float(Fr(x) + Fr(y))


def sub(x, y):
    return float(Fr(x) - Fr(y))


def div(x, y):
    return float(Fr(x) / Fr(y))


def vec(rng, n=N):
    v = rng.standard_normal(n) * 10.0 ** rng.integers(-3, 4, n)          # a spread of exponents: roundings of every size
    v[:4] = [0.0, 1.0, -2.5, 3.0][:min(4, n)]                             # ... and a few exact cases
    return v


def cvec(rng, n=N):
    return vec(rng, n) + 1j * vec(rng, n)[::-1]


@pytest.mark.parametrize("stride", [8, 16])
@pytest.mark.parametrize("nb", [1, 2, 63, 64, 65, 127, 128, 129, 300, 1024])
def test_sum_cols_is_the_lane_strided_sum_then_the_shuffle_tree(nb, stride):
    rng = np.random.default_rng(nb)
    lst = rng.standard_normal((nb, stride)) * 10.0 ** rng.integers(-3, 4, (nb, stride))
    for col in (0, 1, stride - 1):
        lanes = [0.0] * 64
        for b in range(nb):                                               # lane b % 64 meets its entries in ascending order
            lanes[b % 64] = add(lanes[b % 64], float(lst[b, col]))
        off = 32
        while off:
            for lane in range(off):
                lanes[lane] = add(lanes[lane], lanes[lane + off])
            off >>= 1
        assert R.sum_cols(lst, nb, stride, col) == lanes[0], (nb, stride, col)
        assert R.sum_cols(lst.reshape(-1), nb, stride, col) == lanes[0]    # a flat list is read alike
    # a NaN in another column, or past row nb, is never read
    poisoned = np.vstack([lst, np.full((3, stride), np.nan)])
    poisoned[:, 2] = np.nan
    assert R.sum_cols(poisoned, nb, stride, 1) == R.sum_cols(lst, nb, stride, 1)


def test_projection_update_correction_and_scale_round_once_per_operation():
    rng = np.random.default_rng(1)
    w, cols = vec(rng), [vec(rng) for _ in range(8)]
    cf = [float(c) for c in vec(rng, 8) + 0.37]
    a, b, d = 1.7, -0.31, 0.0123
    got_p = {k: R.proj(w, cf[:k], cols[:k]) for k in (0, 1, 7, 8)}
    got_u2, got_u1 = R.update(w, a, cols[0], b, cols[1]), R.update(w, a, cols[0])
    got_c, got_s = R.correct(w, d, cols[1]), R.scale(w, b)
    for i in range(N):
        x = float(w[i])
        for k in range(9):
            if k in got_p:
                assert float(got_p[k][i]) == x, (k, i)
            if k < 8:
                x = sub(x, mul(cf[k], float(cols[k][i])))                   # x - c*v, column order
        u1 = sub(float(w[i]), mul(a, float(cols[0][i])))
        assert float(got_u1[i]) == u1
        assert float(got_u2[i]) == sub(u1, mul(b, float(cols[1][i])))       # (w - a*vj) - b*vjm1
        assert float(got_c[i]) == sub(float(w[i]), mul(d, float(cols[1][i])))
        assert float(got_s[i]) == div(float(w[i]), b)
    assert not np.array_equal(got_u2, w - (a * cols[0] + b * cols[1]))      # the other association differs somewhere: order is pinned


@pytest.mark.parametrize("ncols", [0, 1, 2, 255, 256, 257, 513])
def test_gemv_cols_accumulates_in_column_order_from_zero(ncols):
    rng = np.random.default_rng(ncols)
    n = 7
    V = np.stack([vec(rng, n) for _ in range(ncols)]) if ncols else np.zeros((0, n))
    coef = rng.standard_normal(ncols)
    got = R.gemv_cols(V, coef, np.full(n, np.nan))
    if ncols == 0:
        assert np.isnan(got).all()                                          # nothing is launched: y stays
        return
    for i in range(n):
        s = 0.0
        for k in range(ncols):
            s = add(s, mul(float(V[k, i]), float(coef[k])))
        assert float(got[i]) == s, (ncols, i)


@pytest.mark.parametrize("ncols", [0, 1, 15, 16, 17, 33])
def test_ccombine_accumulates_component_wise_in_column_order(ncols):
    rng = np.random.default_rng(100 + ncols)
    n = 40
    cols = [cvec(rng, n) for _ in range(ncols)]
    cr, ci = rng.standard_normal(ncols), rng.standard_normal(ncols)
    y = cvec(rng, n)
    for init in (True, False):
        got = R.ccombine(cols, cr, ci, y, init)
        for i in range(n):
            ar, ai = (0.0, 0.0) if init else (float(y[i].real), float(y[i].imag))
            for x, r, m in zip(cols, cr, ci):
                xr, xi, r, m = float(x[i].real), float(x[i].imag), float(r), float(m)
                ar = add(ar, sub(mul(r, xr), mul(m, xi)))
                ai = add(ai, add(mul(r, xi), mul(m, xr)))
            assert (float(got[i].real), float(got[i].imag)) == (ar, ai), (ncols, init, i)
    # groups of 16 with init on the first alone are one accumulation from zero
    if ncols > 16:
        g = R.ccombine(cols[:16], cr[:16], ci[:16])
        for k0 in range(16, ncols, 16):
            g = R.ccombine(cols[k0:k0 + 16], cr[k0:k0 + 16], ci[k0:k0 + 16], g, init=False)
        assert np.array_equal(g, R.ccombine(cols, cr, ci))


def test_cheb_init_promote_sub2_and_scale_div():
    rng = np.random.default_rng(5)
    x0, x1 = cvec(rng), cvec(rng)
    c0, c1 = 0.3 - 0.2j, -0.11 + 0.23j
    for have1 in (0, 1):
        got = R.cheb_init(x0, x1, c0, c1, have1)
        for i in range(N):
            tr = add(0.0, sub(mul(c0.real, float(x0[i].real)), mul(c0.imag, float(x0[i].imag))))
            ti = add(0.0, add(mul(c0.real, float(x0[i].imag)), mul(c0.imag, float(x0[i].real))))
            if have1:
                tr = add(tr, sub(mul(c1.real, float(x1[i].real)), mul(c1.imag, float(x1[i].imag))))
                ti = add(ti, add(mul(c1.real, float(x1[i].imag)), mul(c1.imag, float(x1[i].real))))
            assert (float(got[i].real), float(got[i].imag)) == (tr, ti), (have1, i)
    x = vec(rng)
    p1, p2 = R.promote(x, 1), R.promote(x, 2)
    assert p1.dtype == p2.dtype == np.complex128 and len(p1) == N and len(p2) == N // 2
    assert np.array_equal(p1.real, x) and not p1.imag.any() and np.array_equal(p2.real, x[0::2]) and np.array_equal(p2.imag, x[1::2])
    # sd_k_sub2 and sd_k_scale_div are update() and scale(): proven above


@pytest.mark.parametrize("ncols", [1, 2, 3, 9, 10, 11])
def test_longdouble_chains_against_exact_rational_arithmetic(ncols):
    rng = np.random.default_rng(ncols)
    n = 12
    Q = np.linalg.qr(rng.standard_normal((n, ncols)))[0].T.copy()
    w = Q.T @ rng.uniform(0.5, 2.0, ncols) + rng.standard_normal(n) / np.sqrt(n)

    def exact(block):
        x = [Fr(float(t)) for t in w]
        for c0 in range(0, ncols - 1, block):
            cs = range(c0, min(c0 + block, ncols - 1))
            cf = [sum(Fr(float(Q[c, i])) * x[i] for i in range(n)) for c in cs]
            for c, f in zip(cs, cf):
                x = [x[i] - f * Fr(float(Q[c, i])) for i in range(n)]
        return x, sum(Fr(float(Q[ncols - 1, i])) * x[i] for i in range(n))

    def to_ld(fr):
        hi = float(fr)
        return R.LD(hi) + R.LD(float(fr - Fr(hi)))

    for fn, block in ((R.bgs_longdouble, 8), (R.mgs_longdouble, 1)):
        x, last = exact(block)
        got, coefs, got_last = fn(w, Q, ncols)
        assert got.dtype == R.LD and len(coefs) == ncols - 1
        scale = max(abs(float(t)) for t in w)
        err = max(abs(float(g - to_ld(t))) for g, t in zip(got, x)) / scale
        err_last = abs(float(got_last - to_ld(last))) / scale
        print(f"{fn.__name__} ncols={ncols}: {err:.2e} (vector), {err_last:.2e} (last dot), bar {2.0 ** -60:.2e}")
        assert err <= 2.0 ** -60 and err_last <= 2.0 ** -60
    if ncols > 2:                                                           # blocked and sequential are different chains
        assert not np.array_equal(R.bgs_longdouble(w, Q, ncols)[0], R.mgs_longdouble(w, Q, ncols)[0])


@pytest.mark.parametrize("block", [8, 1])
def test_chain_bound_holds_for_the_double_chain_and_sees_a_skipped_column(block):
    rng = np.random.default_rng(8 + block)
    n, ncols = 2001, 26
    Q = np.linalg.qr(rng.standard_normal((n, ncols)))[0].T.copy()
    a = rng.uniform(0.5, 2.0, ncols) * rng.choice([-1.0, 1.0], ncols)
    r = rng.standard_normal(n)
    w = Q.T @ a + r / np.linalg.norm(r)
    ref = (R.bgs_longdouble if block == 8 else R.mgs_longdouble)(w, Q, ncols)[0]
    bound = R.chain_bound(w, Q, ncols, block)
    x = w.copy()                                                            # the chain in doubles, dots by numpy
    for c0 in range(0, ncols - 1, block):
        cs = range(c0, min(c0 + block, ncols - 1))
        cf = [float(Q[c] @ x) for c in cs]
        x = R.proj(x, cf, [Q[c] for c in cs])
    err = np.abs((x.astype(R.LD) - ref).astype(np.float64))
    top = float(np.abs(ref).max())
    print(f"block {block}: max error {err.max():.2e}, max bound {bound.max():.2e}, 1e-8 max|w| {1e-8 * top:.2e}")
    assert (err <= bound).all() and bound.max() <= 1e-8 * top
    skipped = x + a[ncols - 2] * Q[ncols - 2]                               # the last projected column left in
    assert (np.abs((skipped.astype(R.LD) - ref).astype(np.float64)) > bound).any()


@pytest.fixture(scope="module")
def shim(pkg, tmp_path_factory):
    return R.build_shim(pkg, tmp_path_factory.mktemp("blas1_shim"))


def test_shim_links_and_the_pure_host_functions_match_their_constants(shim):
    for n in (1, 2, 511, 512, 513, 524_288, 524_289, 10 ** 9):
        assert shim.b1_gs_blocks(n) == min(1024, max(1, -(-(n // 2) // 256))), n
        assert shim.b1_lanczos_fold_blocks(n) == min(256, max(1, -(-n // 2048))), n
    assert shim.b1_gs_blocks(524_288) == 1024 and shim.b1_gs_blocks(513) == 1 and shim.b1_gs_blocks(514) == 2
