"""The yardstick of the finite-temperature typicality functions, proven without a GPU: the numpy restatement
(tests/typicality_ref.py) against Kronecker-product matrices and dense propagators, plus the host-only coefficient export of
the library.  The residuals printed here are the reference's own error: the bars of tests/test_gpu_typicality.py."""
import ctypes as C

import numpy as np
import pytest
import scipy.special as ss

import typicality_ref as R

_dp = C.POINTER(C.c_double)


def chain(L, boundary="open", Jxy=1.0, Jz=1.0, hz=0.0):
    hop = [(i, i + 1, Jxy / 2) for i in range(1, L)]
    zz = [(i, i + 1, Jz) for i in range(1, L)]
    if boundary == "periodic":
        hop.append((L, 1, Jxy / 2))
        zz.append((L, 1, Jz))
    return hop, zz, np.full(L, hz)


def j1j2(L, J1=1.0, J2=0.4):
    hop = [(i, i % L + 1, J1 / 2) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2 / 2) for i in range(1, L + 1)]
    zz = [(i, i % L + 1, J1) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2) for i in range(1, L + 1)]
    return hop, zz, np.full(L, 0.1)


def rand_vec(N, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(N) + 1j * rng.standard_normal(N)


LISTS = {"open": lambda L: chain(L, "open", Jz=0.7, hz=0.2), "periodic": lambda L: chain(L, "periodic", Jz=0.7), "j1j2": j1j2}


# ---- the library's host-only export ----
def lib_coeffs(pkg, z, n_max=4096):
    c = np.empty(n_max)
    nu = C.c_int(-1)
    rc = pkg.lib().sd_chebyshev_imag_coeffs(n_max, 2.0, z / 2.0, c.ctypes.data_as(_dp), C.byref(nu))
    return rc, c[: max(nu.value, 0)].copy(), nu.value


@pytest.mark.parametrize("z", [0.0, 0.3, 5.0, 60.0, 600.0])
def test_imag_coefficients_match_scipy_to_4_ulp(pkg, z):
    """sd_chebyshev_imag_coeffs against scipy.special.ive, and n_used against the stated rule.  The unit is the ulp of the largest
    coefficient (c_0 <= 1): a coefficient multiplies a Chebyshev vector of norm <= |psi|, so its absolute error is what reaches
    the state.  An ulp of each element cannot be the unit with this reference: measured against 50-digit mpmath values, scipy's
    ive is itself off by 20 / 24 / 178 / 1202 ulp of the element at z = 0.3 / 5 / 60 / 600 (in the tails, where the values are
    below 1e-10 c_0), the library by <= 0.51 ulp.  Measured here: 1.0 / 0.5 / 2.0 / 2.0 ulp of c_0.  The next test holds the
    library to one ulp of EVERY element against the exact values."""
    rc, c, nu = lib_coeffs(pkg, z)
    assert rc == 0
    want = R.imag_coeffs(z)
    assert nu == len(want), (nu, len(want))                 # the stated truncation rule
    e0 = ss.ive(0, z)
    assert nu > z and ss.ive(nu, z) < 2.0 ** -53 * e0
    assert all(not (k > z and ss.ive(k, z) < 2.0 ** -53 * e0) for k in range(nu))
    ulps = np.abs(c - want) / np.spacing(np.abs(want).max())
    print(f"z={z}: n_used={nu}, max deviation {ulps.max():.2f} ulp of c_0")
    assert ulps.max() <= 4.0
    assert abs(np.sum(c * np.where(np.arange(nu) % 2, -1.0, 1.0)) - 1.0) <= 1e-14       # the series at x = -1: exp(z) exp(-z)


@pytest.mark.parametrize("z", [0.3, 5.0, 60.0, 600.0])
def test_imag_coefficients_are_the_rounded_exact_values(pkg, z):
    """every coefficient within one ulp OF ITSELF of (2 - delta_k0) (-1)^k exp(-z) I_k(z).  tests/golden/typicality/imag_coeffs_exact.npz holds
    those values evaluated with 50 digits (mpmath: exp(-z) * besseli(k, z), mp.dps = 50) and rounded once to Float64, array
    "z<z>", a few entries longer than n_used -- so the check needs no multiprecision package and always runs."""
    import os
    exact = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "typicality", "imag_coeffs_exact.npz"))["z%g" % z]
    rc, c, nu = lib_coeffs(pkg, z)
    assert rc == 0 and 0 < nu <= len(exact)
    ulps = np.abs(c - exact[:nu]) / np.spacing(np.abs(exact[:nu]))
    print(f"z={z}: max deviation from the exact values {ulps.max():.3f} ulp")
    assert ulps.max() <= 1.0


def test_imag_coefficients_refuse_bad_arguments(pkg):
    assert lib_coeffs(pkg, 600.5)[0] == 1                   # SD_EARG: z > 600
    assert lib_coeffs(pkg, -0.1)[0] == 1
    assert lib_coeffs(pkg, 60.0, n_max=20)[0] == 1          # n_used would exceed n_max
    assert pkg.lib().sd_chebyshev_imag_coeffs(10, 1.0, 1.0, None, None) == 1
    with pytest.raises(pkg.ArgumentError):
        pkg.chebyshev_imag_coeffs(1.0, 700.0)
    assert np.array_equal(pkg.chebyshev_imag_coeffs(2.0, 2.5), lib_coeffs(pkg, 5.0)[1])


def test_python_mirror_refuses_unknown_methods_and_operators(pkg):
    """argument checks that run before any device call"""
    class Fake:
        L, N, hopping_list = 4, 6, [(1, 2, 0.5)]
    for bad in [dict(method="rk4"), dict(operator_i=("Sx", 1)), dict(operator_j="Sz_all"), dict(operator_i=("Sz", 9)),
                dict(operator_j=("current", [1.0, 2.0])), dict(n_samples=0), dict(dt=0.1)]:
        kw = dict(operator_i=("Sz", 1), operator_j=("Sz", 1), method="chebyshev")
        kw.update(bad)
        oi, oj = kw.pop("operator_i"), kw.pop("operator_j")
        with pytest.raises(pkg.ArgumentError):
            pkg.typicality_correlation_function(Fake, 1.0, oi, oj, [0.0, 0.1], **kw)


# ---- the restatement against Kronecker products ----
@pytest.mark.parametrize("name,L,nup", [("open", 8, 4), ("open", 10, 3), ("periodic", 8, 4), ("periodic", 9, 4), ("periodic", 10, 5),
                                        ("j1j2", 8, 3), ("j1j2", 10, 5), ("periodic", 7, None)])
def test_current_matrix_equals_the_kronecker_form(name, L, nup):
    hop, zz, field = LISTS[name](L)
    states, index = R.basis(L, nup)
    plan = R.CurrentPlan(L, nup, hop, states, index)
    rng = np.random.default_rng(L)
    for w in (None, np.eye(len(hop))[2], rng.standard_normal(len(hop))):
        got = plan.matrix(w)
        want = R.project(R.kron_current(L, hop, w), states)
        err = np.abs(got - want).max()
        print(f"{name} L={L} nup={nup}: row loop vs Kronecker {err:.2e}")
        assert err <= 1e-14
        assert np.abs(got - got.conj().T).max() <= 1e-14     # Hermitian
    Hk = R.project(R.kron_hamiltonian(L, hop, zz, field), states)
    assert np.abs(R.hamiltonian(L, nup, hop, zz, field, states, index).toarray() - Hk).max() <= 1e-14


@pytest.mark.parametrize("name,L,nup", [("open", 8, 4), ("periodic", 8, 3), ("j1j2", 8, 4), ("periodic", 6, None)])
def test_continuity_equation(name, L, nup):
    """i [H, S^z_k] = sum_{b: j_b = k} j_b - sum_{b: i_b = k} j_b"""
    hop, zz, field = LISTS[name](L)
    states, index = R.basis(L, nup)
    H = R.hamiltonian(L, nup, hop, zz, field, states, index).toarray()
    plan = R.CurrentPlan(L, nup, hop, states, index)
    worst = 0.0
    for k in range(1, L + 1):
        Sz = np.diag(R.sz_site(states, k))
        lhs = 1j * (H @ Sz - Sz @ H)
        w = np.array([(1.0 if j == k else 0.0) - (1.0 if i == k else 0.0) for i, j, _ in hop])
        worst = max(worst, np.abs(lhs - plan.matrix(w)).max())
    print(f"{name} L={L} nup={nup}: continuity residual {worst:.2e}")
    assert worst <= 1e-14


# ---- the per-sample loop against dense propagators ----
def sample_setup(name, L, nup):
    hop, zz, field = LISTS[name](L)
    states, index = R.basis(L, nup)
    H = R.hamiltonian(L, nup, hop, zz, field, states, index)
    Hd = H.toarray()
    w = np.linalg.eigvalsh(Hd)
    plan = R.CurrentPlan(L, nup, hop, states, index)
    return hop, states, H, Hd, (w[0] - 0.05, w[-1] + 0.05), plan


@pytest.mark.parametrize("L,nup", [(8, 4), (10, 5)])
@pytest.mark.parametrize("beta", [0.0, 0.5, 4.0])
@pytest.mark.parametrize("method", ["chebyshev", "krylov"])
def test_sample_identity_against_dense_propagators(L, nup, beta, method):
    hop, states, H, Hd, Eb, plan = sample_setup("periodic", L, nup)
    r = rand_vec(len(states), 5 + L)
    times = [0.0, 0.4, 0.8, 1.2, 2.0]
    worst = 0.0
    for A, B in [(("Sz", 3), ("Sz", 1)), (("Sz_all", None), ("Sz", 2)), (("Szq", 2 * np.pi / L), ("Szq", 2 * np.pi / L)),
                 (("current", None), ("current", None))]:
        Ao, Bo = R.Operator(*A, L, states, plan), R.Operator(*B, L, states, plan)
        num, ln, en = R.dqt_sample(H, Ao, Bo, beta, r, times, method=method, Ebounds=Eb, kry_m=30)
        num_d, ln_d, en_d = R.dqt_dense(Hd, Ao, Bo, beta, r, times)
        err = max(np.abs(num - num_d).max(), abs(ln - ln_d), abs(en - en_d))
        worst = max(worst, err)
    print(f"L={L} beta={beta} {method}: reference vs dense {worst:.2e}")
    # measured: <= 4.4e-15 for both methods in all twelve cases (the truncated series is summed to rounding; the one Krylov
    # projection on 30 vectors is exact to rounding while beta/2 * bandwidth, here <= 12, is small against 30); the bar is ten
    # times that, for other BLAS builds
    assert worst <= 5e-14


def test_current_is_conserved_at_jz_zero_and_the_sum_rule_holds():
    """[J, H] = 0 for the periodic chain at Jz = 0: C_JJ(t) is constant; sum_i <psi(t)|S^z_i S^z_j ... > = (nup - L/2) <S^z_j>."""
    L, nup, beta = 10, 5, 1.0
    hop, zz, field = chain(L, "periodic", Jz=0.0)
    states, index = R.basis(L, nup)
    H = R.hamiltonian(L, nup, hop, zz, field, states, index)
    plan = R.CurrentPlan(L, nup, hop, states, index)
    w = np.linalg.eigvalsh(H.toarray())
    Eb = (w[0] - 0.05, w[-1] + 0.05)
    r = rand_vec(len(states), 3)
    times = np.linspace(0.0, 4.0, 9)
    Jop = R.Operator("current", None, L, states, plan)
    num, _, _ = R.dqt_sample(H, Jop, Jop, beta, r, times, Ebounds=Eb)
    drift = np.abs(num - num[0]).max()
    print(f"C_JJ(t) drift at Jz = 0: {drift:.2e} on |C_JJ| = {abs(num[0, 0]):.3f}")
    assert drift <= 1.5e-14                                  # measured 1.3e-15, times ten
    # sum rule at Jz = 0.7, sector nup = 4
    hop, zz, field = chain(L, "periodic", Jz=0.7)
    states, index = R.basis(L, 4)
    H = R.hamiltonian(L, 4, hop, zz, field, states, index)
    w = np.linalg.eigvalsh(H.toarray())
    Eb = (w[0] - 0.05, w[-1] + 0.05)
    r = rand_vec(len(states), 4)
    num, _, _ = R.dqt_sample(H, R.Operator("Sz_all", None, L, states), R.Operator("Sz", 2, L, states), beta, r, times, Ebounds=Eb)
    psi, _ = R.imag_chebyshev(H, r / np.linalg.norm(r), beta / 2, Eb)
    want = (4 - L / 2) * np.vdot(psi, R.sz_site(states, 2) * psi)
    res = np.abs(num.sum(axis=1) - want).max()
    print(f"sum rule residual: {res:.2e}")
    assert res <= 2e-15                                      # measured 2.0e-16, times ten


def test_substepped_imaginary_time_matches_dense():
    """The upper bound widened until z = a beta/2 > 600: the step is split and renormalised.  (Only the upper one: the series is
    scaled to 1 at the LOWER bound, so a lower bound far below the spectrum leaves a sum of size exp(-tau (E_0 - Emin)) formed
    from terms of size 1 -- the relative error grows by that factor.  DESIGN.md 14.)"""
    L, nup = 8, 4
    hop, states, H, Hd, Eb, plan = sample_setup("periodic", L, nup)
    wide = (Eb[0], Eb[1] + 300.0)
    beta = 10.0
    a, _ = R.rescaling(*wide)
    assert a * beta / 2 > 600
    r = rand_vec(len(states), 1)
    psi, ln = R.imag_chebyshev(H, r, beta / 2, wide)
    w, U = np.linalg.eigh(Hd)
    v = U @ (np.exp(-0.5 * beta * (w - w[0])) * (U.T @ r))
    err = np.abs(psi - v / np.linalg.norm(v)).max()
    eln = abs(ln - (np.log(np.linalg.norm(v)) - 0.5 * beta * w[0]))
    print(f"sub-stepped: state {err:.2e}, log_norm {eln:.2e}")
    assert err <= 1.5e-14 and eln <= 4e-13                   # measured 1.2e-15 and 3.6e-14, times ten
