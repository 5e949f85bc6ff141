"""The yardstick of the site-resolved KPM correlations, proven without a GPU: the numpy restatement (tests/site_moments_ref.py)
against the dense spectral sum, against the oracle's per-momentum moments, and the one-source shortcut for a
translation-invariant state.  Plus the host pieces of the library that need no device."""
import types

import numpy as np
import pytest

import site_moments_ref as R


def ground_state(D, L, nup, boundary, O=None, need_gap=False):
    """Dense sector H (Kronecker products for L <= 10; above, the columns of the oracle's apply_H, which the existing tests pin
    against the Kronecker form), its ground state and spectrum."""
    if L <= 10:
        hop, zz, field = D.xxz_lists(L, boundary=boundary)
        H = D.dense_H(L, nup, hop, zz, field)
    else:
        model = O.XXZChain(L, nup=nup, boundary=boundary)
        eye = np.eye(model.N)
        H = np.array([O.apply_H(model, eye[k]) for k in range(model.N)]).T
        assert np.array_equal(H, H.T)
    w, V = np.linalg.eigh(H)
    if need_gap:
        assert w[1] - w[0] > 1e-6      # non-degenerate: the ground state is translation invariant on the periodic chain
    return H, V[:, 0].copy(), w


def random_state(N, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    return x / np.linalg.norm(x)


def bounds(w):
    return (w[-1] - w[0]) / (2 * 0.99), (w[-1] + w[0]) / 2


@pytest.mark.parametrize("L,nup", [(9, 4), (10, 5)])
@pytest.mark.parametrize("boundary", ["open", "periodic"])
@pytest.mark.parametrize("state", ["ground", "random"])
def test_recursion_matches_the_dense_spectral_sum(O, D, L, nup, boundary, state):
    H, gs, w = ground_state(D, L, nup, boundary)
    model = O.XXZChain(L, nup=nup, boundary=boundary)
    psi0 = gs if state == "ground" else random_state(model.N, L)
    a, b = bounds(w)
    sources, M = [1, L // 2 + 1, L], 512
    got = R.site_moments(O, model, psi0, sources, M, a, b)
    want = R.dense_spectral_moments(H, model.states, L, psi0, sources, M, a, b)
    err = np.abs(got - want).max()
    print(f"L={L} {boundary} {state}: recursion vs spectral sum {err:.2e}")
    assert err <= 1e-12
    if state == "ground":
        assert np.abs(got.imag).max() <= 1e-15      # real psi0: real moments


@pytest.mark.parametrize("L,nup,boundary,state", [(10, 5, "open", "ground"), (10, 5, "periodic", "random"), (12, 6, "periodic", "ground")])
def test_fourier_identity_against_the_oracle_moments(O, D, L, nup, boundary, state):
    """(1/L) sum_ij e^{-iq(r_i - r_j)} mu_n^{ij} = |phi_q|^2 x compute_chebyshev_moments(phi_q / |phi_q|) at every momentum."""
    H, gs, w = ground_state(D, L, nup, boundary, O)
    model = O.XXZChain(L, nup=nup, boundary=boundary)
    psi0 = gs if state == "ground" else random_state(model.N, 3)
    a, b = bounds(w)
    M = 256
    sources = list(range(1, L + 1))
    mu = R.site_moments(O, model, psi0, sources, M, a, b)
    worst = 0.0
    for q in O.momenta(model):
        phi = O.Sz_q_vector(model, psi0, q)
        nphi = np.linalg.norm(phi)
        mq = R.moments_q_all(mu, sources, q)
        if nphi < 1e-13:
            want = np.zeros(M)
        else:
            want = nphi ** 2 * O.compute_chebyshev_moments(model, phi / nphi, M, a, b)
        worst = max(worst, np.abs(mq.real - want).max(), np.abs(mq.imag).max())
    print(f"L={L} {boundary} {state}: Fourier identity {worst:.2e}")
    assert worst <= 1e-12


@pytest.mark.parametrize("L", [10, 12])
def test_one_source_identity_for_the_periodic_ground_state(O, D, L):
    nup = L // 2
    H, gs, w = ground_state(D, L, nup, "periodic", O, need_gap=True)
    model = O.XXZChain(L, nup=nup, boundary="periodic")
    a, b = bounds(w)
    M = 256
    sources = list(range(1, L + 1))
    mu = R.site_moments(O, model, gs, sources, M, a, b)
    worst = defect = 0.0
    for q in O.momenta(model):
        full = R.moments_q_all(mu, sources, q).real
        for s in (0, L // 2):
            one = R.moments_q_one(mu[s], sources[s], q)
            worst = max(worst, np.abs(one.real - full).max())
            defect = max(defect, np.abs(one.imag).max() / 0.25)
    print(f"L={L}: one source vs all sources {worst:.2e}, defect {defect:.2e}")
    assert worst <= 1e-12 and defect <= 1e-12


@pytest.mark.parametrize("boundary,state", [("periodic", "random"), ("open", "ground")])
def test_one_source_shortcut_fails_without_translation_invariance(O, D, boundary, state):
    """What the invariance guard is for: the shortcut is off by O(0.1) for a random state or an open chain."""
    L, nup = 10, 5
    H, gs, w = ground_state(D, L, nup, boundary)
    model = O.XXZChain(L, nup=nup, boundary=boundary)
    psi0 = gs if state == "ground" else random_state(model.N, 5)
    a, b = bounds(w)
    sources = list(range(1, L + 1))
    mu = R.site_moments(O, model, psi0, sources, 64, a, b)
    off = max(np.abs(R.moments_q_one(mu[0], 1, q).real - R.moments_q_all(mu, sources, q).real).max() for q in O.momenta(model))
    print(f"{boundary} {state}: one source off by {off:.2e}")
    assert off >= 0.05 * 0.25


def test_signed_reconstruction_matches_the_restatement(pkg, O):
    """sd_kpm_reconstruct_signed (host code of the library): the restatement's formula, and kpm_reconstruct wherever that is
    positive."""
    rng = np.random.default_rng(0)
    M, a, b, E0 = 300, 3.3, -0.4, -2.9
    mu = rng.standard_normal(M) * pkg.get_kernel(M, "jackson") / (1.0 + np.arange(M))
    omega = np.linspace(-0.5, 7.5, 160)
    got = pkg.kpm_reconstruct_signed(mu, omega, a, b, E0)
    want = R.reconstruct_signed(mu, omega, a, b, E0)
    scale = np.abs(want).max()
    assert np.abs(got - want).max() <= 1e-11 * scale
    assert (got < 0).any() and (got == 0).any()            # signed, and zero outside the band
    clamped = O.kpm_reconstruct(mu, omega, a, b, E0)
    assert np.abs(np.maximum(got, 0.0) - clamped).max() <= 1e-12 * scale
    z = mu + 1j * mu[::-1]
    gz = pkg.kpm_reconstruct_signed(z, omega, a, b, E0)
    assert np.array_equal(gz.real, got) and np.array_equal(gz.imag, pkg.kpm_reconstruct_signed(mu[::-1].copy(), omega, a, b, E0))


def test_shift_invariance_of_the_lists(pkg, D):
    """The list check in front of translation_invariant=True (needs no device: any object with the model's list fields)."""
    from importlib import import_module
    solvers = import_module(pkg.__name__ + ".solvers")

    def fake(L, boundary, field=None, extra=()):
        hop, zz, f = D.xxz_lists(L, boundary=boundary)
        return types.SimpleNamespace(L=L, hopping_list=list(hop) + list(extra), zz_list=list(zz),
                                     onsite_field=np.asarray(f if field is None else field, dtype=float))
    assert solvers._shift_invariant(fake(8, "periodic"))
    assert not solvers._shift_invariant(fake(8, "open"))
    assert not solvers._shift_invariant(fake(8, "periodic", field=[0.1] + [0.0] * 7))
    assert solvers._shift_invariant(fake(8, "periodic", field=[0.1] * 8))
    assert not solvers._shift_invariant(fake(8, "periodic", extra=[(1, 3, 0.2)]))
    assert solvers._shift_invariant(fake(8, "periodic", extra=[(i, (i + 1) % 8 + 1, 0.2) for i in range(1, 9)]))
