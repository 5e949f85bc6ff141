"""tests/opstring_ref.py (the numpy restatement the GPU tests of the operator strings compare with) against Kronecker products of
oracle/dense.py's one-site matrices, restricted to the sector order: no bit tricks, no ranking on that side.  CPU only."""
import numpy as np
import pytest

import dimer_ref as DR
import ecurrent_ref as ER
import opstring_ref as OR


def mats(D):
    return {"+": D.SP, "-": D.SM, "z": D.SZ, "x": 0.5 * (D.SP + D.SM), "y": (D.SP - D.SM) / 2j}


def kron_string(D, L, factors):
    """prod of one-site operators on distinct sites as ONE Kronecker chain (site 1 is the rightmost factor)"""
    chain = [D.I2.astype(np.complex128)] * L
    for kind, site in factors:
        chain[L - site] = mats(D)[kind].astype(np.complex128)
    out = chain[0]
    for m in chain[1:]:
        out = np.kron(out, m)
    return out


def dense_terms(D, L, terms, op=0):
    O = np.zeros((1 << L, 1 << L), dtype=np.complex128)
    for P, M, Z, c, o in terms:
        if o != op:
            continue
        f = [("+", i) for i in range(1, L + 1) if P >> (i - 1) & 1] + [("-", i) for i in range(1, L + 1) if M >> (i - 1) & 1] + \
            [("z", i) for i in range(1, L + 1) if Z >> (i - 1) & 1]
        O += complex(c) * kron_string(D, L, f)
    return O


def restrict(D, O, L, nup):
    if nup is None:
        return O
    st = D.sector_states(L, nup).astype(np.int64)
    return O[np.ix_(st, st)]


def rand_vec(rng, n, cplx):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n) if cplx else rng.standard_normal(n)


def random_strings(rng, L, n_strings, kinds):
    """[(coeff, factors)]: up to 6 distinct sites each, factor kinds drawn from `kinds`"""
    out = []
    for _ in range(n_strings):
        k = int(rng.integers(1, min(6, L) + 1))
        sites = rng.choice(np.arange(1, L + 1), size=k, replace=False)
        c = complex(rng.standard_normal(), rng.standard_normal() if rng.random() < 0.5 else 0.0)
        out.append((c, [(str(rng.choice(kinds)), int(s)) for s in sites]))
    return out


def random_conserving_strings(rng, L, n_strings):
    """the same with as many S^+ as S^- factors (at least one pair where two sites are to be had), the other sites S^z"""
    out = []
    for _ in range(n_strings):
        k = int(rng.integers(1, min(6, L) + 1))
        sites = [int(s) for s in rng.choice(np.arange(1, L + 1), size=k, replace=False)]
        npairs = int(rng.integers(min(1, k // 2), k // 2 + 1))
        kinds = ["+"] * npairs + ["-"] * npairs + ["z"] * (k - 2 * npairs)
        c = complex(rng.standard_normal(), rng.standard_normal() if rng.random() < 0.5 else 0.0)
        out.append((c, list(zip(kinds, sites))))
    return out


CASES = [(4, 2), (6, 3), (7, 2), (8, 4), (8, None), (5, None), (10, 5), (9, 1), (6, 0), (6, 6)]


@pytest.mark.parametrize("L,nup", CASES)
@pytest.mark.parametrize("cplx", [False, True])
def test_random_strings_match_kronecker_products(D, L, nup, cplx):
    """sum of random strings with x / y factors; on the full basis (L <= 8) the sector-changing terms stay, in a sector the dense
    operator is restricted and the list keeps its S^z-conserving terms"""
    rng = np.random.default_rng(1000 * L + (0 if nup is None else nup + 1) + (50 if cplx else 0))
    strings = random_strings(rng, L, 5 if L >= 9 else 8, ["+", "-", "z", "x", "y"]) + random_conserving_strings(rng, L, 3)
    terms, dense = [], np.zeros((1 << L, 1 << L), dtype=np.complex128)
    for c, f in strings:
        terms += OR.expand(c, f)
        dense += c * kron_string(D, L, f)
    if nup is not None:
        terms = OR.sector_terms(terms)
    O = restrict(D, dense, L, nup)
    psi = rand_vec(rng, O.shape[0], cplx)
    got = OR.apply_rows(terms, psi, L, nup)
    bar = 1e-13 * max(np.linalg.norm(O, 2), 1e-300) * np.linalg.norm(psi)
    assert np.abs(got - O @ psi).max() <= bar
    # the same operator with equal (P, M, Z) merged and regrouped
    got2 = OR.apply_rows(OR.simplify(terms), psi, L, nup)
    assert np.abs(got2 - O @ psi).max() <= bar


@pytest.mark.parametrize("L,nup", [(6, 3), (7, None), (8, 4)])
def test_several_operators_and_expectations(D, L, nup):
    rng = np.random.default_rng(77 + L)
    terms, dense = [], []
    for k in range(5):
        O = np.zeros((1 << L, 1 << L), dtype=np.complex128)
        for c, f in (random_conserving_strings(rng, L, 3) if nup is not None else random_strings(rng, L, 3, ["+", "-", "z", "x"])):
            tl = OR.expand(c, f, op=k)
            terms += tl
            O += dense_terms(D, L, tl, op=k)
        dense.append(restrict(D, O, L, nup))
    rng.shuffle(terms)                                   # operators interleaved in the list
    n = dense[0].shape[0]
    bra, ket = rand_vec(rng, n, True), rand_vec(rng, n, True)
    assert OR.n_ops(terms) == 5
    for k, (val, scale) in enumerate(OR.expectations(terms, bra, ket, L, nup)):
        want = np.vdot(bra, dense[k] @ ket)
        assert abs(val - want) <= 1e-13 * max(scale, np.linalg.norm(dense[k], 2) * np.linalg.norm(bra) * np.linalg.norm(ket))


@pytest.mark.parametrize("L", [5, 7])
def test_adjoint_is_the_conjugate_transpose(D, L):
    rng = np.random.default_rng(L)
    terms = []
    for c, f in random_strings(rng, L, 6, ["+", "-", "z", "y"]):
        terms += OR.expand(c, f)
    O = dense_terms(D, L, terms)
    assert np.abs(dense_terms(D, L, OR.adjoint(terms)) - O.conj().T).max() <= 1e-14 * max(np.abs(O).max(), 1.0)
    assert not OR.is_hermitian(terms)
    assert OR.is_hermitian(terms + OR.adjoint(terms))


@pytest.mark.parametrize("L,nup,boundary,hz", [(6, 3, "open", 0.0), (7, 3, "periodic", 0.3), (8, None, "periodic", -0.7), (2, 1, "open", 0.0),
                                               (3, None, "periodic", 0.2)])
def test_hamiltonian_terms_are_dense_H(D, L, nup, boundary, hz):
    hop, zz, field = D.xxz_lists(L, Jxy=0.9, Jz=1.3, hz=hz, boundary=boundary)
    hop = hop + [(1, 3, 0.25)] if L >= 3 else hop                # a second-neighbour hop as well
    terms = OR.hamiltonian_terms(hop, zz, field)
    assert OR.is_hermitian(terms)
    H = D.dense_H(L, nup, hop, zz, field)
    rng = np.random.default_rng(L)
    psi = rand_vec(rng, H.shape[0], False)
    got = OR.apply_rows(terms, psi, L, nup)
    assert np.abs(got.imag).max() == 0.0
    assert np.abs(got.real - H @ psi).max() <= 1e-13 * np.linalg.norm(H, 2) * np.linalg.norm(psi)


@pytest.mark.parametrize("L,nup,periodic", [(6, 3, False), (7, 3, True), (6, None, False)])
def test_energy_current_as_strings(L, nup, periodic):
    rng = np.random.default_rng(5 + L)
    hop = [(i, i + 1, float(rng.standard_normal())) for i in range(1, L)] + ([(L, 1, 0.7)] if periodic else [])
    zz = [(i, i + 1, float(rng.standard_normal())) for i in range(1, L)] + ([(L, 1, -0.4)] if periodic else [])
    field = list(rng.standard_normal(L))
    dterms = ER.energy_current_terms(L, hop, zz, field, periodic)
    assert len(dterms) > 0
    n = len(OR.configurations(L, nup))
    for cplx in (False, True):
        psi = rand_vec(rng, n, cplx)
        want = ER.apply_rows(dterms, psi, L, nup)
        got = OR.apply_rows(OR.from_ecurrent(dterms), psi, L, nup)
        assert np.abs(got - want).max() <= 1e-13 * 2 * ER.row_sum_bound(dterms) * np.abs(psi).max()
    assert OR.is_hermitian(OR.from_ecurrent(dterms))


@pytest.mark.parametrize("L,nup", [(6, 3), (7, None)])
def test_bond_operator_as_strings(L, nup):
    import torch
    rng = np.random.default_rng(9 + L)
    s = OR.configurations(L, nup)
    st = torch.as_tensor(s.astype(np.int64))
    for (i, j, xy, zz) in [(1, 2, 1.0, 1.0), (L, 2, 0.7, -1.1), (3, 5, 0.0, 2.0)]:
        for cplx in (False, True):
            psi = rand_vec(rng, len(s), cplx)
            want = DR.bond_rows(torch.as_tensor(psi), st, L, nup, i, j, xy, zz).numpy()
            got = OR.apply_rows(OR.from_bond(i, j, xy, zz), psi, L, nup)
            assert np.abs(got - want).max() <= 1e-14 * (abs(xy) + abs(zz)) * np.abs(psi).max()


def reflect_mask(m, L):
    return sum(1 << (L - 1 - b) for b in range(L) if m >> b & 1)


@pytest.mark.parametrize("L,triple", [(5, (1, 2, 3)), (6, (2, 5, 3)), (6, (6, 1, 4))])
def test_chirality_is_the_triple_product(D, L, triple):
    i, j, k = triple
    terms = OR.chirality(i, j, k, coeff=1.0)
    dense = np.zeros((1 << L, 1 << L), dtype=np.complex128)
    for perm, sign in OR.EPS:
        dense += sign * kron_string(D, L, [("xyz"[a], s) for a, s in zip(perm, triple)])
    assert len(terms) == 6 and all(OR.popcount(P) == 1 and OR.popcount(M) == 1 and OR.popcount(Z) == 1 for P, M, Z, _c, _o in terms)
    assert np.abs(dense_terms(D, L, terms) - dense).max() <= 1e-15
    assert OR.is_hermitian(terms) and np.abs(dense - dense.conj().T).max() == 0.0
    # odd under reflection: R chi_ijk R = chi_{i'j'k'} with i' = L + 1 - i, and an odd permutation of the sites flips the sign, so
    # for ascending sites the reflected operator is minus the chirality of the reflected sites taken in ascending order
    refl = OR.simplify([(reflect_mask(P, L), reflect_mask(M, L), reflect_mask(Z, L), c, o) for P, M, Z, c, o in terms])
    ri, rj, rk = (L + 1 - x for x in triple)
    assert refl == OR.chirality(ri, rj, rk)
    assert refl == OR.simplify([(P, M, Z, -c, o) for P, M, Z, c, o in OR.chirality(rk, rj, ri)])
    # a real vector has no chirality
    for nup in (None, 2):
        psi = np.random.default_rng(3).standard_normal(len(OR.configurations(L, nup)))
        (val, scale), = OR.expectations(terms, psi, psi, L, nup)
        assert abs(val.real) <= 1e-15 * max(scale, 1.0)


def test_chirality_product_of_disjoint_triples(D):
    L = 6
    a, b = OR.chirality(1, 2, 3), OR.chirality(4, 6, 5)
    want = dense_terms(D, L, a) @ dense_terms(D, L, b)
    assert np.abs(dense_terms(D, L, OR.product(a, b)) - want).max() <= 1e-15
    assert OR.is_hermitian(OR.product(a, b))


@pytest.mark.parametrize("L,nup,i,j", [(6, 3, 1, 2), (6, 3, 2, 5), (7, None, 1, 7), (8, 4, 3, 6)])
def test_string_order_is_its_dense_definition(D, L, nup, i, j):
    st = np.arange(1 << L, dtype=np.int64) if nup is None else D.sector_states(L, nup).astype(np.int64)
    sz = lambda site: ((st >> (site - 1)) & 1) - 0.5                    # noqa: E731
    diag = -sz(i) * np.exp(1j * np.pi * sum((sz(l) for l in range(i + 1, j)), np.zeros(len(st)))) * sz(j)
    psi = rand_vec(np.random.default_rng(L + i), len(st), True)
    got = OR.apply_rows(OR.string_order(i, j), psi, L, nup)
    assert np.abs(got - diag * psi).max() <= 1e-14 * np.abs(psi).max()
    if j == i + 1:
        assert OR.string_order(i, j) == [(0, 0, OR.bit(i) | OR.bit(j), -1.0 + 0j, 0)]


def test_fused_form_is_one_multiply_and_one_add():
    rng = np.random.default_rng(0)
    o, y = rand_vec(rng, 50, True), rand_vec(rng, 50, True)
    b = 0.3 - 1.7j
    got = OR.fused(o, y, b)
    assert np.abs(got - (o + b * y)).max() <= 4e-16 * (np.abs(o).max() + abs(b) * np.abs(y).max())
    assert np.array_equal(OR.fused(o.real + 0j, y.real, 0.5, real=True), o.real + 0.5 * y.real)
