"""Real-time Chebyshev evolution at long steps, z = a*dt from 400 to 2e4, forwards and backwards, on the GPU: every driver that
feeds sd_chebyshev_coeffs into the term loop, against the exact propagator exp(-iHt) from the dense matrix's eigensystem.
Wide energy bounds make a*dt large at t = 1 while the spectrum stays inside them, so the cases stay small and quick.

The bars are the CPU oracle's own: its chebyshev_time_evolve (libm jn coefficients, good to 4e-16 at every z here; one
accumulation per term) was measured against the same dense propagator at each shape and z (ORACLE_DEV below, max over both term
counts of max_k |psi_k - exact_k|).  The library gets FOUR times that -- it adds the terms in pairs, in another order, and its
apply sums a row's bonds in another order than the oracle's -- and never less than the project's Chebyshev bar of 1e-12.
The coefficients and term counts themselves are pinned on the CPU by tests/test_chebyshev_coeffs_host.py against
tests/golden/chebyshev/real_coeffs_exact.npz, which also gives the term counts used here."""
import os

import numpy as np
import pytest

import typicality_ref as R

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "chebyshev", "real_coeffs_exact.npz"))
N_USED = {float(z): int(n) for z, n in zip(GOLD["z"], GOLD["n_used"])}

SHAPES = {"per10": (10, 5, "periodic"),           # 252 rows
          "open13": (13, 6, "open")}              # 1716 rows, tiled plan
ZS = [400.0, 999.0, 1000.5, 1100.0, 5000.0]
CENTER = -1.0                                     # b of the rescaling: both spectra lie in (-6, 4)

# max |oracle chebyshev_time_evolve - exact propagator| at t = 1 (cheb_n = n_used and n_used - 1), measured on the CPU
ORACLE_DEV = {
    ("per10", 400.0): 4.2e-16, ("per10", 999.0): 4.6e-16, ("per10", 1000.5): 5.3e-16, ("per10", 1100.0): 5.2e-16,
    ("per10", 5000.0): 1.1e-15, ("per10", 2e4): 1.6e-15,
    ("open13", 400.0): 3.0e-16, ("open13", 999.0): 3.2e-16, ("open13", 1000.5): 3.0e-16, ("open13", 1100.0): 3.1e-16,
    ("open13", 5000.0): 5.5e-16,
}
# |num(T) in one step - num(T) in ten| of the numpy restatement of the typicality loop (tests/typicality_ref.py, oracle
# coefficients) at a*T = 1100, measured on the CPU
TYPICALITY_DEV = {"per10": 3.1e-16, "open13": 4.2e-16}


def bar(dev):
    return max(4.0 * dev, 1e-12)


def bounds(z, dt=1.0):
    """(Emin, Emax) with (Emax - Emin) / (2 * 0.9999) * |dt| = z (to a rounding) around CENTER"""
    half = 0.9999 * z / abs(dt)
    return CENTER - half, CENTER + half


_systems = {}


def system(D, name):
    """the dense side of a shape, computed once and left unchanged: (lists, H eigenvalues, eigenvectors, psi0)"""
    if name not in _systems:
        L, nup, bc = SHAPES[name]
        hop, zz, field = D.xxz_lists(L, boundary=bc)
        if L <= 10:
            Hd = D.dense_H(L, nup, hop, zz, field)
        else:
            # the Kronecker products of oracle/dense.py take minutes at 2^13: the sector matrix of the numpy restatement,
            # held to dense.py's at the small shape right here
            small = D.xxz_lists(10, boundary=bc)
            assert np.abs(R.hamiltonian(10, 5, *small).toarray() - D.dense_H(10, 5, *small)).max() <= 1e-15
            Hd = R.hamiltonian(L, nup, hop, zz, np.asarray(field)).toarray()
        w, V = np.linalg.eigh(Hd)
        assert -6.0 < w[0] and w[-1] < 4.0
        rng = np.random.default_rng(11 + L)
        psi0 = rng.standard_normal(len(w)) + 1j * rng.standard_normal(len(w))
        psi0 /= np.linalg.norm(psi0)
        for a in (w, V, psi0):
            a.setflags(write=False)
        _systems[name] = (L, nup, bc, w, V, psi0)
    return _systems[name]


def exact(w, V, psi, t):
    return V @ (np.exp(-1j * w * t) * (V.T @ psi))


def model_of(pkg, name):
    L, nup, bc = SHAPES[name]
    m = pkg.XXZChain(L, nup=nup, boundary=bc)
    assert np.array_equal(m.states_range(0, m.N), R.basis(L, nup)[0])
    return m


def evolve(pkg, m, psi, dt, n, Eb):
    return pkg.chebyshev_time_evolve(psi, dt, pkg.apply_H, m, cheb_n=n, Ebounds=Eb)


@pytest.mark.parametrize("z", ZS)
@pytest.mark.parametrize("name", list(SHAPES))
def test_long_steps_against_the_exact_propagator(pkg, D, name, z):
    """chebyshev_time_evolve at z = a*dt in {400, 999, 1000.5, 1100, 5000} with cheb_n = n_used(z) (the first k > z with
    |J_k(z)| < 2^-53) and n_used - 1: an even and an odd count, so both tails of the paired-term loop run.
    Oracle against the dense propagator, measured on the CPU (bar = 4 x, at least 1e-12):
        per10  (252 rows):  z=400 4.2e-16, 999 4.6e-16, 1000.5 5.3e-16, 1100 5.2e-16, 5000 1.1e-15
        open13 (1716 rows): z=400 3.0e-16, 999 3.2e-16, 1000.5 3.0e-16, 1100 3.1e-16, 5000 5.5e-16
    (its norm off by up to 5.0e-15 at z = 5000), the same backwards: four times that stays under 1e-12, so 1e-12 is the bar
    of every case.  The norm of psi(t) is held to 1 within the same bar."""
    L, nup, bc, w, V, psi0 = system(D, name)
    m = model_of(pkg, name)
    if name == "open13":
        assert m.device_path == "tiled"
    Eb = bounds(z)
    assert Eb[0] < w[0] and w[-1] < Eb[1]
    want = exact(w, V, psi0, 1.0)
    tol = bar(ORACLE_DEV[(name, z)])
    for n in (N_USED[z], N_USED[z] - 1):
        got = evolve(pkg, m, psi0, 1.0, n, Eb)
        dev = np.abs(got - want).max()
        dn = abs(np.linalg.norm(got) - 1.0)
        print(f"{name} z={z:g} cheb_n={n}: |psi - exact| = {dev:.2e}, | |psi| - 1 | = {dn:.2e} (bar {tol:.2e})")
        assert dev <= tol and dn <= tol


def test_twenty_thousand_terms(pkg, O, D):
    """z = 2e4 once, at 252 rows: about 20 300 applies in one step.  Oracle against the dense propagator on the CPU: 1.6e-15
    (norm 4.9e-15).
    Norm, the exact propagator and the oracle within 4 x that (at least 1e-12)."""
    name, z = "per10", 2e4
    L, nup, bc, w, V, psi0 = system(D, name)
    m = model_of(pkg, name)
    Eb = bounds(z)
    n = N_USED[z]
    got = evolve(pkg, m, psi0, 1.0, n, Eb)
    want = O.chebyshev_time_evolve(O.XXZChain(L, nup=nup, boundary=bc), psi0, 1.0, cheb_n=n, Ebounds=Eb)
    tol = bar(ORACLE_DEV[(name, z)])
    d_or, d_ex, dn = np.abs(got - want).max(), np.abs(got - exact(w, V, psi0, 1.0)).max(), abs(np.linalg.norm(got) - 1.0)
    print(f"z=2e4 cheb_n={n}: |psi - oracle| = {d_or:.2e}, |psi - exact| = {d_ex:.2e}, | |psi| - 1 | = {dn:.2e} (bar {tol:.2e})")
    assert d_or <= tol and d_ex <= tol and dn <= tol


@pytest.mark.parametrize("z", [2.16, 1100.0])
@pytest.mark.parametrize("name", list(SHAPES))
def test_backward_evolution_is_the_conjugate_bit_for_bit(pkg, D, name, z):
    """H is real: exp(+iHt) psi = conj(exp(-iHt) conj(psi)).  The library keeps that exactly -- c(-dt) = conj(c(dt)) bit for
    bit, and conjugating both factors of every complex product only flips the sign of its imaginary part."""
    L, nup, bc, w, V, psi0 = system(D, name)
    m = model_of(pkg, name)
    dt = 1.0 if z > 100 else 0.4                                  # a = 5.4 at the short step: the spectrum stays inside the bounds
    Eb = bounds(z, dt)
    assert Eb[0] < w[0] and w[-1] < Eb[1]
    for n in (N_USED[z], N_USED[z] - 1):
        back = evolve(pkg, m, psi0, -dt, n, Eb)
        fwd = evolve(pkg, m, np.conj(psi0), dt, n, Eb)
        assert np.array_equal(back, np.conj(fwd)), np.abs(back - np.conj(fwd)).max()
    dev = np.abs(back - exact(w, V, psi0, -dt)).max()             # and it IS the backward propagator (with n_used - 1 terms)
    print(f"{name} z={-z:g}: |psi - exact| = {dev:.2e}")
    assert dev <= 1e-12


@pytest.mark.parametrize("z", [1100.0, 5000.0])
@pytest.mark.parametrize("name", list(SHAPES))
def test_round_trip(pkg, D, name, z):
    """forwards, then backwards: psi0 again within the bar of one step (two steps of a quarter of it each at most)"""
    L, nup, bc, w, V, psi0 = system(D, name)
    m = model_of(pkg, name)
    Eb, n = bounds(z), N_USED[z]
    there = evolve(pkg, m, psi0, 1.0, n, Eb)
    back = evolve(pkg, m, there, -1.0, n, Eb)
    dev = np.abs(back - psi0).max()
    tol = bar(ORACLE_DEV[(name, z)])
    print(f"{name} z={z:g}: |back - psi0| = {dev:.2e} (bar {tol:.2e})")
    assert dev <= tol


@pytest.mark.parametrize("name", list(SHAPES))
def test_typicality_one_long_step_against_ten_short(pkg, D, name):
    """typicality_correlation_function with cheb_n = 0 (automatic count): times [0, T] with a*T = 1100 against the same T
    reached in ten equal steps of a*dt = 110, infinite temperature, <S^z_2(T) S^z_1>.  The numpy restatement of the same loop
    with the oracle's coefficients, one step against ten, on the CPU: per10 3.1e-16, open13 4.2e-16; the bar is 4 x that, at
    least 1e-12, so 1e-12.  The apply counter shows the exact term count of the long step for both states: the first term takes no
    apply, so 2 (n_used - 1) applies beyond what the call needs at t = 0."""
    L, nup, bc, w, V, psi0 = system(D, name)
    m = model_of(pkg, name)
    Eb = bounds(1100.0)
    T = 1.0
    kw = dict(r=psi0, Ebounds=Eb, cheb_n=0)
    c0 = m.ctx.apply_count()
    pkg.typicality_correlation_function(m, 0.0, ("Sz", 2), ("Sz", 1), [0.0], **kw)
    c1 = m.ctx.apply_count()
    one = pkg.typicality_correlation_function(m, 0.0, ("Sz", 2), ("Sz", 1), [0.0, T], **kw)
    c2 = m.ctx.apply_count()
    ten = pkg.typicality_correlation_function(m, 0.0, ("Sz", 2), ("Sz", 1), np.linspace(0.0, T, 11), **kw)
    assert (c2 - c1) - (c1 - c0) == 2 * (N_USED[1100.0] - 1), (c0, c1, c2)
    states = R.basis(L, nup)[0]
    A, B = R.sz_site(states, 2), R.sz_site(states, 1)
    want = np.vdot(A * exact(w, V, psi0, T), exact(w, V, B * psi0, T))
    dev = abs(one[-1] - ten[-1])
    tol = bar(TYPICALITY_DEV[name])
    print(f"{name}: |one step - ten steps| = {dev:.2e}, |one step - exact| = {abs(one[-1] - want):.2e} (bar {tol:.2e})")
    assert one[0] == ten[0]
    assert dev <= tol and abs(one[-1] - want) <= tol


@pytest.mark.parametrize("name", list(SHAPES))
def test_device_resident_and_sharded_give_the_host_call_bits(pkg, D, name):
    """z = 1100, forwards and backwards: sd_chebyshev_evolve_dev and a one-rank ShardedOperator against the host-pointer call"""
    import torch
    L, nup, bc, w, V, psi0 = system(D, name)
    m = model_of(pkg, name)
    z = 1100.0
    Eb, n = bounds(z), N_USED[z]
    dev = torch.device("cuda", m.ctx.device)
    x = torch.from_numpy(psi0.copy()).to(dev)
    op = pkg.ShardedOperator(model_of(pkg, name), 0, 1)
    for dt in (1.0, -1.0):
        host = evolve(pkg, m, psi0, dt, n, Eb)
        on_dev = evolve(pkg, m, x, dt, n, Eb)
        assert np.array_equal(on_dev.cpu().numpy(), host)
        sharded = op.chebyshev_time_evolve(x.clone(), dt, cheb_n=n, Ebounds=Eb)
        assert np.array_equal(sharded.cpu().numpy(), host)
