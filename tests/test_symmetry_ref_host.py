"""tests/symmetry_ref.py against dense operators built independently with oracle/dense.py: T, R and Z as products of Kronecker-product
exchange / flip operators on the full 2^L space, restricted to the sector order of sector_states.  CPU only.

  SWAP_ij = 1/2 + 2 S_i . S_j (entries exactly 0 and 1),  T = SWAP_12 SWAP_23 ... SWAP_{L-1,L} (the rightmost acts first: the spin of
  site L walks down to site 1, every other spin moves up by one),  R = prod_{i < L+1-i} SWAP_{i,L+1-i},  Z = prod_i (S^+_i + S^-_i).

Couplings are dyadic (0.5, 0.75, 0.25, 0.125), so every matrix element of H is an exact sum and [H, U_g] = 0 holds to the bit."""
import numpy as np
import pytest

import symmetry_ref as SR

# (L, nup); None: the full basis
CASES = [(2, 1), (3, 1), (4, 2), (5, 2), (6, 3), (6, 1), (7, 3), (8, 4), (8, 3), (10, 5), (6, None), (8, None)]


def swap(D, i, j, L):
    sp = D.site_op(D.SP, i, L) @ D.site_op(D.SM, j, L)
    return 0.5 * np.eye(1 << L) + 2.0 * (D.site_op(D.SZ, i, L) @ D.site_op(D.SZ, j, L)) + sp + sp.T


_dense = {}


def dense_ops(D, L):
    """(T, R, Z) on the full space"""
    if L not in _dense:
        dim = 1 << L
        Tm = np.eye(dim)
        for i in range(L - 1, 0, -1):                     # SWAP_{L-1,L} acts first
            Tm = swap(D, i, i + 1, L) @ Tm
        Rm = np.eye(dim)
        for i in range(1, L // 2 + 1):
            Rm = swap(D, i, L + 1 - i, L) @ Rm
        Zm = np.eye(dim)
        for i in range(1, L + 1):
            Zm = (D.site_op(D.SP, i, L) + D.site_op(D.SM, i, L)) @ Zm
        for M in (Tm, Rm, Zm):
            assert np.all((M == 0.0) | (M == 1.0)) and np.all(M.sum(0) == 1.0) and np.all(M.sum(1) == 1.0)
        _dense[L] = (Tm, Rm, Zm)
    return _dense[L]


def dense_U(D, L, nup, g):
    """U_g = T^r R^refl Z^flip restricted to the sector"""
    Tm, Rm, Zm = dense_ops(D, L)
    r, refl, flip = g
    U = np.linalg.matrix_power(Tm, r) @ (Rm if refl else np.eye(1 << L)) @ (Zm if flip else np.eye(1 << L))
    if nup is None:
        return U
    st = D.sector_states(L, nup).astype(np.int64)
    return U[np.ix_(st, st)]


def elements(L, nup):
    fl = (0, 1) if SR.flip_defined(L, nup) else (0,)
    return [(r, refl, f) for r in sorted({0, 1, 2 % L, L // 2, L - 1}) for refl in (0, 1) for f in fl]


def vec(L, nup, cplx, seed):
    N = len(SR.configurations(L, nup))
    rng = np.random.default_rng(seed)
    return rng.standard_normal(N) + 1j * rng.standard_normal(N) if cplx else rng.standard_normal(N)


def test_the_definitions_on_basis_states(D):
    """T moves the spin of site i to site i + 1, R exchanges i and L + 1 - i, Z flips: one up spin on L = 5"""
    L = 5
    Tm, Rm, Zm = dense_ops(D, L)
    for i in range(1, L + 1):
        e = np.zeros(1 << L)
        e[1 << (i - 1)] = 1.0
        assert (Tm @ e)[1 << (i % L)] == 1.0
        assert (Rm @ e)[1 << (L - i)] == 1.0
        assert (Zm @ e)[((1 << L) - 1) ^ (1 << (i - 1))] == 1.0
    s = np.array([0b00101], dtype=np.uint64)
    assert SR.T(s, L)[0] == 0b01010 and SR.T(s, L, 3)[0] == 0b01001 and SR.R(s, L)[0] == 0b10100 and SR.Z(s, L)[0] == 0b11010
    assert SR.transform(s, L, (1, 1, 1))[0] == SR.T(SR.R(SR.Z(s, L), L), L)[0]


@pytest.mark.parametrize("L,nup", CASES)
def test_apply_and_overlaps_match_the_dense_operators(D, L, nup):
    s = SR.configurations(L, nup)
    if nup is not None:
        assert np.array_equal(s, D.sector_states(L, nup))
    psi, bra = vec(L, nup, True, 10 * L + 1), vec(L, nup, True, 10 * L + 2)
    el = elements(L, nup)
    for g in el:
        U = dense_U(D, L, nup, g)
        assert np.array_equal(SR.apply(psi, L, nup, g), U @ psi), g                    # a permutation: exact
        assert np.array_equal(SR.rows_of(SR.transform(s, L, g), L, nup)[SR.source_rows(L, nup, g)], np.arange(len(s)))
    ov = SR.overlaps(bra, psi, L, nup, el)
    want = np.array([np.vdot(bra, dense_U(D, L, nup, g) @ psi) for g in el])
    assert np.abs(ov - want).max() <= 1e-13 * np.linalg.norm(bra) * np.linalg.norm(psi)
    assert ov[0] == np.vdot(bra, psi)


@pytest.mark.parametrize("L,nup", [(2, 1), (3, 1), (5, 2), (6, 3), (8, 4), (7, None)])
def test_group_laws(L, nup):
    psi = vec(L, nup, True, 77 + L)
    A = lambda v, g: SR.apply(v, L, nup, g)             # noqa: E731
    x = psi
    for _ in range(L):
        x = A(x, (1, 0, 0))
    assert np.array_equal(x, psi)                                                      # T^L = 1
    assert np.array_equal(A(A(psi, (0, 1, 0)), (0, 1, 0)), psi)                        # R^2 = 1
    assert np.array_equal(A(A(A(psi, (0, 1, 0)), (1, 0, 0)), (0, 1, 0)), A(psi, (L - 1, 0, 0)))     # R T R = T^-1
    for a in range(L):
        for b in range(L):
            assert np.array_equal(A(A(psi, (b, 0, 0)), (a, 0, 0)), A(psi, ((a + b) % L, 0, 0)))
    assert np.array_equal(A(psi, (1, 1, 0)), A(A(psi, (0, 1, 0)), (1, 0, 0)))          # U_(r, refl) = T^r R^refl
    if SR.flip_defined(L, nup):
        assert np.array_equal(A(A(psi, (0, 0, 1)), (0, 0, 1)), psi)                    # Z^2 = 1
        assert np.array_equal(A(psi, (2 % L, 1, 1)), A(A(A(psi, (0, 0, 1)), (0, 1, 0)), (2 % L, 0, 0)))


@pytest.mark.parametrize("L", [2, 4, 6, 8, 10, 12, 14, 16])
def test_spin_flip_at_half_filling_is_the_row_reversal(L):
    rows = SR.source_rows(L, L // 2, (0, 0, 1))
    assert np.array_equal(rows, len(rows) - 1 - np.arange(len(rows)))


def models(L):
    """name -> (hop, zz, field) with dyadic couplings"""
    ring = lambda J: [(i, i % L + 1, J) for i in range(1, L + 1)]          # noqa: E731
    chain = lambda J: [(i, i + 1, J) for i in range(1, L)]                 # noqa: E731
    nnn = lambda J: [(i, (i + 1) % L + 1, J) for i in range(1, L + 1)]     # noqa: E731
    rng = np.random.default_rng(5)
    return {
        "ring": (ring(0.5), ring(0.75), np.zeros(L)),
        "ring-field": (ring(0.5), ring(0.75), np.full(L, 0.125)),
        "open": (chain(0.5), chain(0.75), np.zeros(L)),
        "j1j2-field": (ring(0.5) + nnn(0.25), ring(1.0) + nnn(0.5), np.full(L, 0.125)),
        "random-field": (ring(0.5), ring(0.75), rng.integers(1, 64, L) / 64.0),
    }


@pytest.mark.parametrize("name", ["ring", "ring-field", "open", "j1j2-field", "random-field"])
@pytest.mark.parametrize("L,nup", [(6, 3), (7, 3), (8, 4), (6, None)])
def test_commutators_vanish_exactly_where_the_model_is_symmetric(pkg, D, L, nup, name):
    hop, zz, field = models(L)[name]
    m = pkg.build_model(L, nup=nup, hopping=hop, zz=zz, onsite_field=field, ctx=None)
    H = D.dense_H(L, nup, hop, zz, list(field))
    seen = set()
    for g in elements(L, nup):
        if g == (0, 0, 0):
            continue
        U = dense_U(D, L, nup, g)
        sym = pkg.is_symmetric(m, *g)
        seen.add(sym)
        comm = H @ U - U @ H
        if sym:
            assert np.all(comm == 0.0), (name, g)
        elif g[2] and nup is not None and name in ("ring-field", "j1j2-field") and pkg.is_symmetric(m, g[0], g[1]):
            # is_symmetric speaks about the lists: a uniform field is refused for Z, although inside a half-filled SECTOR it is the
            # constant h (nup - L/2) = 0 and drops out; the full-basis case below shows that the field does break Z
            assert np.all(comm == 0.0), (name, g)
        else:
            assert np.abs(comm).max() > 1e-3, (name, g)
    if name in ("ring-field", "j1j2-field"):              # T and R hold; Z, where it is defined, is broken by the field
        assert seen == ({True, False} if SR.flip_defined(L, nup) else {True})
    else:
        assert seen == {"ring": {True}, "open": {True, False}, "random-field": {False}}[name]


@pytest.mark.parametrize("L,nup", [(2, 1), (3, 1), (4, 2), (6, 3), (7, 3), (8, 4), (5, None)])
def test_momentum_projectors(L, nup):
    N = len(SR.configurations(L, nup))
    eye = np.eye(N)
    P = [np.stack([SR.project(eye[:, j], L, nup, momentum=n) for j in range(N)], axis=1) for n in range(L)]
    Tm = np.stack([SR.apply(eye[:, j], L, nup, (1, 0, 0)) for j in range(N)], axis=1)
    for n in range(L):
        assert np.abs(P[n] - P[n].conj().T).max() <= 1e-14                             # Hermitian
        assert np.abs(P[n] @ P[n] - P[n]).max() <= 1e-14                               # idempotent
        for k in range(n):
            assert np.abs(P[n] @ P[k]).max() <= 1e-14
        assert np.abs(Tm @ P[n] - np.exp(-2j * np.pi * n / L) * P[n]).max() <= 1e-14   # T P_n = e^{-i k_n} P_n
    assert np.abs(sum(P) - eye).max() <= 1e-14
    psi = vec(L, nup, True, 5 * L)
    w = SR.momentum_weights(psi, L, nup)
    n2 = np.vdot(psi, psi).real
    assert np.all(w >= -1e-13 * n2) and abs(w.sum() - n2) <= 1e-13 * n2
    assert np.abs(w - np.array([np.vdot(psi, P[n] @ psi).real for n in range(L)])).max() <= 1e-13 * n2
    # parity and spin flip combine with k = 0 (and k = pi): the product is again a projector that commutes with T
    for kw in ([dict(momentum=0, parity=1), dict(momentum=0, parity=-1)] + ([dict(momentum=L // 2, parity=-1)] if L % 2 == 0 else [])
               + ([dict(momentum=0, parity=1, spin_flip=-1), dict(spin_flip=1)] if SR.flip_defined(L, nup) else [])):
        Q = np.stack([SR.project(eye[:, j], L, nup, **kw) for j in range(N)], axis=1)
        assert np.abs(Q @ Q - Q).max() <= 1e-14 and np.abs(Q - Q.conj().T).max() <= 1e-14, kw
        if all(c.imag == 0.0 for c in SR.projector_list(L, **kw)[1]):
            assert np.all(Q.imag == 0.0)


def test_labels_of_dense_eigenvectors(D):
    """the Heisenberg ring L = 8: the ground state is a singlet with k = 0, even parity, even under Z (L = 4 m)"""
    L, nup = 8, 4
    hop, zz, field = D.xxz_lists(L, boundary="periodic")
    w, v = np.linalg.eigh(D.dense_H(L, nup, hop, zz, field))
    assert w[1] - w[0] > 0.1
    assert SR.labels(v[:, 0], L, nup) == (0, 1, 1)
    assert SR.labels(vec(L, nup, True, 3), L, nup) == (None, None, None)


@pytest.mark.parametrize("L,nup", [(6, 3), (9, 4), (7, None)])
def test_torch_ports_equal_the_numpy_functions(L, nup):
    import torch
    s = SR.configurations(L, nup)
    st = torch.from_numpy(s.astype(np.int64))
    psi = vec(L, nup, True, 9)
    pt = torch.from_numpy(psi)
    el = elements(L, nup)
    for g in el:
        assert np.array_equal(SR.source_rows_t(st, L, nup, g).numpy(), SR.source_rows(L, nup, g)), g
        assert np.array_equal(SR.apply_t(pt, st, L, nup, g).numpy(), SR.apply(psi, L, nup, g))
    co = np.random.default_rng(1).standard_normal(len(el)) + 1j * np.random.default_rng(2).standard_normal(len(el))
    assert np.array_equal(SR.combine_t(pt, st, L, nup, el, co).numpy(), SR.combine(psi, L, nup, el, co))
    assert np.array_equal(SR.combine_t(pt.real.contiguous(), st, L, nup, el, co).numpy(), SR.combine(psi.real.copy(), L, nup, el, co))
    ov = SR.overlaps_t(pt, pt, st, L, nup, el)
    assert np.abs(ov - SR.overlaps(psi, psi, L, nup, el)).max() <= 1e-13 * np.vdot(psi, psi).real
