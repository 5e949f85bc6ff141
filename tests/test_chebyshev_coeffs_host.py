"""The scalars of real-time Chebyshev evolution, pinned without a GPU at every a*dt the library admits:
c_k = (2 - delta_k0) (-i)^k J_k(a dt) exp(-i b dt) from sd_chebyshev_coeffs and the automatic term count from sd_chebyshev_terms,
against tests/golden/chebyshev/real_coeffs_exact.npz -- J_k(z) from a 70-digit backward recurrence, rounded once to Float64, and
the exact count (tests/golden/make_chebyshev_golden.py; the tests read only the file).  u = 2^-53 throughout."""
import ctypes as C
import math
import os
import time

import numpy as np
import pytest

_dp = C.POINTER(C.c_double)
U = 2.0 ** -53
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chebyshev", "real_coeffs_exact.npz"))
ZS = [float(z) for z in GOLD["z"]]
UNIT = np.array([1, -1j, -1, 1j])                 # (-i)^k, exact


def golden(z):
    """(k, J_k(z) at those k, n_used) -- every k up to n_used + 8 for z <= 1100, a sample above"""
    i = ZS.index(z)
    return GOLD[f"k{i}"].astype(np.int64), GOLD[f"J{i}"], int(GOLD["n_used"][i])


def raw_coeffs(pkg, n, a, b, dt):
    c = np.full(n, np.nan + 1j * np.nan)
    rc = pkg.lib().sd_chebyshev_coeffs(n, a, b, dt, c.ctypes.data_as(_dp))
    return rc, c


def lib_terms(pkg, z):
    n = C.c_int(-1)
    rc = pkg.lib().sd_chebyshev_terms(z, C.byref(n))
    return rc, n.value


def exact_coeffs(k, J):
    return np.where(k == 0, 1.0, 2.0) * J * UNIT[k & 3]


def test_golden_file_is_what_the_tests_assume():
    assert ZS == [0.5, 2.16, 30.0, 100.0, 400.0, 999.0, 1000.0, 1000.5, 1100.0, 5000.0, 2e4, 1e5, 1e6]
    for z in ZS:
        k, J, nu = golden(z)
        assert len(k) == len(J) and k[-1] == nu + 8 and (np.diff(k) > 0).all()
        assert nu > z and abs(J[k == nu][0]) < U and (np.abs(J[(k > z) & (k < nu)]) >= U).all()
        if z <= 1100:
            assert np.array_equal(k, np.arange(nu + 9))
        else:
            assert len(k) <= 1200 and np.array_equal(k[k >= int(z) - 64], np.arange(int(z) - 64, nu + 9))


@pytest.mark.parametrize("z", ZS)
def test_coefficients_match_the_exact_values_to_4u(pkg, z):
    """sd_chebyshev_coeffs(n, a = z, b = 0, dt = 1): the phase is exactly 1 and (-i)^k an exact unit, so c_k is 2 J_k (J_0 for
    k = 0) on one axis and zero on the other.  Bar 4u ABSOLUTE: |2 J_k| < 2, so two ulps of a value below 2 that was rounded once
    from extended precision (the golden value is itself rounded once: u/2 of J, u of 2J)."""
    k, J, nu = golden(z)
    rc, c = raw_coeffs(pkg, int(k[-1]) + 1, z, 0.0, 1.0)
    assert rc == 0
    dev = np.abs(c[k] - exact_coeffs(k, J)).max()
    print(f"z={z:g}: {len(k)} orders up to {k[-1]}, worst |c_k - exact| = {dev / U:.3f} u")
    assert dev <= 4 * U
    # the axis that must be empty is empty
    assert not c.real[1::2].any() and not c.imag[0::2].any()
    assert np.isfinite(c.view(np.float64)).all() and np.abs(c).max() <= 2.0


@pytest.mark.parametrize("z", [2.16, 400.0, 1000.5, 5000.0, 1e5])
@pytest.mark.parametrize("b,dt", [(-0.3, 0.5), (1.7, -2.0), (9973.3, 1.0), (-40013.7, 0.25)])
def test_phase_factor_to_8u(pkg, z, b, dt):
    """b != 0, |b dt| up to 1e4, both signs of dt: against (golden 2 J_k (-i)^k) * (cos p - i sin p), p = the Float64 product
    b*dt, cos and sin from this test's own libm calls.  (dt is a power of two so that a = z/|dt| gives |a*dt| = z exactly: the
    golden values are for that z and no neighbour.)  Bar 8u = the 4u of the b = 0 test plus three more roundings, each of a
    value of modulus <= 2: cos p and sin p are each good to an ulp of a value <= 1, i.e. <= 2u absolute, of which ONE enters
    each component ((-i)^k is axis-aligned, the other factor is exactly zero), scaled by |2 J_k| < 1 for z >= 2: 2u; the
    complex multiply is then one product per component, u/2 relative of a value below 2: u.  Sum 4u + 2u + u = 7u <= 8u."""
    k, J, nu = golden(z)
    a = z / abs(dt)
    assert a * dt == math.copysign(z, dt)
    sgn = np.where((k & 1) == 1, np.sign(dt), 1.0)                   # J_k(-z) = (-1)^k J_k(z)
    p = b * dt
    want = exact_coeffs(k, J * sgn) * complex(math.cos(p), -math.sin(p))
    rc, c = raw_coeffs(pkg, int(k[-1]) + 1, a, b, dt)
    assert rc == 0
    dev = max(np.abs(c[k].real - want.real).max(), np.abs(c[k].imag - want.imag).max())
    print(f"z={z:g} b={b} dt={dt}: worst component deviation {dev / U:.3f} u")
    assert dev <= 8 * U


@pytest.mark.parametrize("z", [1e5, 1e6, 31415.9])
def test_sum_rules_where_the_golden_values_are_sampled(pkg, z):
    """Every order at once where the file holds only a sample (and at one z it does not hold): J_0 + 2 sum_k J_2k = 1 and
    J_0^2 + 2 sum_k J_k^2 = 1, summed exactly (math.fsum) over the library's Float64 values up to n_used + 8.
    Bar u * fsum|terms| + 2^-52 for both.  First rule: a Float64 J_k rounded once from a value good to far below its ulp is off
    by at most u RELATIVE (half an ulp), so the sum is off by at most u times the sum of the terms' moduli, reached only if
    every rounding falls the same way; the 2^-52 covers the truncated tail (|J_k| < 2^-53 from n_used on, falling by more than
    a third per order there: under 2^-52 in all) and what the recurrence itself leaves.  Second rule: a square carries twice
    the relative error, 2u * sum(terms) = 2^-52 at worst since the terms sum to 1, which is the second summand; the first, u,
    is then what remains for the tail and the recurrence.  The first rule is sharp for signs and parity (the terms alternate
    in blocks and sum to 1 out of ~ sqrt(z) of moduli), the second for amplitudes; the first is also the normalisation the
    library uses, the second is independent of it."""
    rc, nu = lib_terms(pkg, z)
    assert rc == 0
    n = nu + 9
    rc, c = raw_coeffs(pkg, n, z, 0.0, 1.0)
    assert rc == 0
    k = np.arange(n)
    sign = np.where(((k & 3) == 0) | ((k & 3) == 3), 1.0, -1.0)      # the sign the unit (-i)^k leaves on its axis
    J = (c.real + c.imag) * sign                                     # one of the two is zero
    J[1:] /= 2.0                                                     # exact
    t1 = [J[0]] + [2.0 * x for x in J[2::2]]
    t2 = [J[0] * J[0]] + [2.0 * x * x for x in J[1:]]
    d1 = abs(math.fsum(t1) - 1.0)
    d2 = abs(math.fsum(t2) - 1.0)
    bar1 = U * math.fsum(abs(x) for x in t1) + 2.0 ** -52
    bar2 = U * math.fsum(t2) + 2.0 ** -52
    print(f"z={z:g}: n_used={nu}; |J_0 + 2 sum J_2k - 1| = {d1:.3e} (bar {bar1:.3e}); |J_0^2 + 2 sum J_k^2 - 1| = {d2:.3e} (bar {bar2:.3e})")
    assert d1 <= bar1 and d2 <= bar2


@pytest.mark.parametrize("z", ZS)
@pytest.mark.parametrize("b", [0.0, -0.3])
def test_negative_time_is_the_conjugate_bit_for_bit(pkg, z, b):
    _, _, nu = golden(z)
    n = min(nu + 9, 6000)
    a, dt = z / 0.8, 0.8
    rc1, fwd = raw_coeffs(pkg, n, a, b, dt)
    rc2, bwd = raw_coeffs(pkg, n, a, b, -dt)
    assert rc1 == 0 and rc2 == 0
    assert np.array_equal(bwd, np.conj(fwd))
    rc3, neg_a = raw_coeffs(pkg, n, -a, 0.0, dt)                     # the sign of a*dt is what counts
    rc4, pos_a = raw_coeffs(pkg, n, a, 0.0, dt)
    assert rc3 == 0 and rc4 == 0 and np.array_equal(neg_a, np.conj(pos_a))


@pytest.mark.parametrize("z", [z for z in ZS if z <= 5000])
@pytest.mark.parametrize("sign", [1.0, -1.0])
def test_oracle_parity(pkg, O, z, sign):
    """the project's bar for the coefficients (tests/test_cabi_host.py): 1e-15 against the oracle's libm jn, both time directions"""
    _, _, nu = golden(z)
    got = pkg.chebyshev_coeffs(nu + 9, z, -0.3, sign)
    want = O.chebyshev_coeffs(nu + 9, z, -0.3, sign)
    dev = np.abs(got - want).max()
    print(f"z={sign * z:g}: |lib - oracle| = {dev:.3e}")
    assert dev <= 1e-15


@pytest.mark.parametrize("a,dt", [(0.0, 0.7), (3.0, 0.0), (0.0, 0.0)])
def test_zero_step_is_the_bare_phase(pkg, a, dt):
    b = -1.25
    rc, c = raw_coeffs(pkg, 40, a, b, dt)
    assert rc == 0
    assert c[0].real == math.cos(b * dt) and c[0].imag == -math.sin(b * dt)
    assert not c[1:].real.any() and not c[1:].imag.any()


def test_bad_arguments_come_back_as_status(pkg):
    """SD_EARG (1), never an exception across the C ABI (which would end the process), and the Python mirror raises"""
    inf, nan = float("inf"), float("nan")
    for a, b, dt in [(nan, 0.0, 1.0), (inf, 0.0, 1.0), (-inf, 0.0, 1.0), (1.0, 0.0, nan), (1.0, 0.0, inf), (1.0, 0.0, -inf),
                     (0.0, 0.0, inf), (inf, 0.0, 0.0), (1.0, nan, 1.0), (1.0, inf, 1.0),
                     (1e6, 0.0, 1.0000001), (1e3, 0.0, -1000.001), (1e200, 0.0, 1e200), (-1e200, 0.0, 1e200)]:
        assert raw_coeffs(pkg, 8, a, b, dt)[0] == 1, (a, b, dt)
    assert raw_coeffs(pkg, 8, 1e6, 0.0, 1.0)[0] == 0 and raw_coeffs(pkg, 8, -1e3, 0.0, 1e3)[0] == 0      # the cap itself is admitted
    assert pkg.lib().sd_chebyshev_coeffs(0, 1.0, 0.0, 1.0, np.empty(2).ctypes.data_as(_dp)) == 1
    assert pkg.lib().sd_chebyshev_coeffs(4, 1.0, 0.0, 1.0, None) == 1
    for z in [nan, inf, -inf, 1000000.5, -1000000.5]:
        assert lib_terms(pkg, z)[0] == 1, z
    assert pkg.lib().sd_chebyshev_terms(1.0, None) == 1
    with pytest.raises(pkg.ArgumentError):
        pkg.chebyshev_coeffs(10, 1.0, 0.0, -2e6)
    with pytest.raises(pkg.ArgumentError):
        pkg.chebyshev_terms(2e6)
    assert pkg.chebyshev_terms(2.16) == golden(2.16)[2]


@pytest.mark.parametrize("z", ZS)
def test_term_count_is_the_exact_one(pkg, z):
    """the first k with k > |z| and |J_k(z)| < 2^-53, for either sign of z.  (The generator refuses a z at which some |J_k|
    lies within 1e-6 relative of 2^-53, so the count does not hang on the last digits of either side.)"""
    nu = golden(z)[2]
    assert lib_terms(pkg, z) == (0, nu)
    assert lib_terms(pkg, -z) == (0, nu)


def test_term_count_is_monotone_up_to_the_cap(pkg):
    zs = np.concatenate([[0.0, 1e-300, 1e-9, 0.5, 1.0], np.geomspace(1.5, 1e6, 195)])
    assert len(zs) == 200 and zs[-1] == 1e6
    ns = [lib_terms(pkg, float(z)) for z in zs]
    assert all(rc == 0 for rc, _ in ns)
    ns = np.array([n for _, n in ns])
    assert (np.diff(ns) >= 0).all(), ns
    assert (ns > zs).all() and ns[0] == 1 and ns[-1] == golden(1e6)[2]


def test_a_million_terms_take_well_under_a_second(pkg):
    """all orders come from one recurrence: O(z + n).  One Bessel evaluation per order would be O(n^2) -- minutes here."""
    n = golden(1e6)[2]
    c = np.empty(n, dtype=np.complex128)
    t0 = time.perf_counter()
    rc = pkg.lib().sd_chebyshev_coeffs(n, 1e6, 0.25, 1.0, c.ctypes.data_as(_dp))
    dt = time.perf_counter() - t0
    print(f"{n} coefficients at z = 1e6: {dt * 1e3:.1f} ms")
    assert rc == 0 and dt < 0.5
