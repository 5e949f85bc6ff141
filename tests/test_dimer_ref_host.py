"""tests/dimer_ref.py against Kronecker-product operators (oracle/dense.py::site_op) on the full 2^L space, the sector embedded with
sector_states: D_b = xy/2 (S^+_i S^-_j + S^-_i S^+_j) + zz S^z_i S^z_j as a dense matrix, D_b psi row by row, D_ab = (D_a psi)^dagger
(D_b psi) and e_b = psi^dagger D_b psi for every ordered pair, real and complex random vectors; then the identities and the
Majumdar-Ghosh values the GPU tests rely on.  CPU only.  Tolerance 1e-13 <psi|psi>, the bar of tests/test_pair_ref_host.py: every
entry is a sum of at most 2^10 products bounded by |psi|^2 (|xy|, |zz| <= 1), formed in double precision on both sides."""
import numpy as np
import pytest

import dimer_ref as DR
from test_pair_ref_host import embed

# (L, nup); None: the full basis
CASES = [(8, None), (8, 4), (10, 3), (9, 0), (9, 9)]
WEIGHTS = [(1.0, 1.0), (0.8, 0.7)]


def bond_list(L):
    """all nearest-neighbour bonds with the closing one, plus two long bonds (one reversed)"""
    return [(i, i % L + 1) for i in range(1, L + 1)] + [(1, L - 2), (L - 1, 2)]


def dense_bond(D, L, i, j, xy, zz):
    sp_i, sm_i, sp_j, sm_j = D.site_op(D.SP, i, L), D.site_op(D.SM, i, L), D.site_op(D.SP, j, L), D.site_op(D.SM, j, L)
    return 0.5 * xy * (sp_i @ sm_j + sm_i @ sp_j) + zz * D.site_op(D.SZ, i, L) @ D.site_op(D.SZ, j, L)


def sector_rows(D, L, nup):
    return np.arange(1 << L) if nup is None else D.sector_states(L, nup).astype(np.int64)


def singlet_product(D, L):
    """prod_k (|up down> - |down up>)/sqrt 2 on sites (2k+1, 2k+2) as a vector of the sector (L, L/2); site 1 is the lowest bit"""
    pair = np.array([0.0, 1.0, -1.0, 0.0]) / np.sqrt(2.0)       # index = bit of site 1 + 2 * bit of site 2
    full = pair
    for _ in range(L // 2 - 1):
        full = np.kron(full, pair)
    return full[sector_rows(D, L, L // 2)]


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("L,nup", CASES)
def test_dimer_ref_matches_kronecker_operators(D, L, nup, cplx):
    import torch
    rows = sector_rows(D, L, nup)
    N = len(rows)
    rng = np.random.default_rng(2000 * L + (77 if nup is None else nup) + (500 if cplx else 0))
    psi = rng.standard_normal(N) + (1j * rng.standard_normal(N) if cplx else 0.0)
    if not cplx:
        psi = psi.real.astype(np.float64)
    full = embed(D, psi, L, nup)
    norm = float(np.vdot(psi, psi).real)
    bonds = bond_list(L)
    s = DR.configurations(N, L, nup, "cpu")
    assert np.array_equal(s.numpy(), rows)
    for xy, zz in WEIGHTS:
        dense = [dense_bond(D, L, i, j, xy, zz) @ full for (i, j) in bonds]
        for (i, j), want in zip(bonds, dense):
            got = DR.bond_rows(torch.from_numpy(psi), s, L, nup, i, j, xy, zz).numpy()
            assert got.dtype == psi.dtype and np.abs(got - want[rows]).max() <= 1e-13 * np.sqrt(norm)
            outside = np.ones(1 << L, dtype=bool)
            outside[rows] = False
            assert np.all(want[outside] == 0.0)                 # D_b conserves S^z: nothing leaves the sector
            rev = DR.bond_rows(torch.from_numpy(psi), s, L, nup, j, i, xy, zz).numpy()
            assert np.array_equal(rev, got)                     # symmetric in its two sites, to the bit
        G = np.array([[np.vdot(x, y) for y in dense] for x in dense])
        E = np.array([np.vdot(full, x).real for x in dense])
        Dm, e = DR.gram(psi, L, nup, bonds, xy, zz)
        assert Dm.shape == (len(bonds), len(bonds)) and e.shape == (len(bonds),)
        assert np.abs(Dm - G).max() <= 1e-13 * norm and np.abs(e - E).max() <= 1e-13 * norm
        if not cplx:
            assert np.all(Dm.imag == 0.0)
        pairs = [(0, 1), (1, 0), (3, 3), (0, len(bonds) - 1)]
        sub, e2 = DR.gram(psi, L, nup, bonds, xy, zz, pairs=pairs)
        assert all(sub[p] == Dm[p] for p in pairs) and np.array_equal(e, e2)


def test_identities_on_a_random_complex_vector(D):
    """xy = 0.8, zz = 0.7, L = 8 full basis, the periodic nearest-neighbour list: D is Hermitian to rounding, Im D_ab is far from
    rounding for overlapping bonds and zero to rounding for disjoint ones (they commute), and sum_ab D_ab = |H psi|^2 for
    H = sum_b D_b -- B^2 entries each within 1e-13 <psi|psi> of its value."""
    L, xy, zz = 8, 0.8, 0.7
    rng = np.random.default_rng(88)
    psi = rng.standard_normal(1 << L) + 1j * rng.standard_normal(1 << L)
    norm = float(np.vdot(psi, psi).real)
    bonds = [(i, i % L + 1) for i in range(1, L + 1)]
    Dm, e = DR.gram(psi, L, None, bonds, xy, zz)
    assert np.abs(Dm - Dm.conj().T).max() <= 1e-13 * norm
    assert np.abs(np.diagonal(Dm).imag).max() <= 1e-13 * norm
    over = np.array([[a != b and len({*bonds[a], *bonds[b]}) < 4 for b in range(L)] for a in range(L)])
    apart = np.array([[len({*bonds[a], *bonds[b]}) == 4 for b in range(L)] for a in range(L)])
    assert over.sum() == 2 * L and apart.sum() == L * (L - 3)
    assert np.abs(Dm.imag[over]).max() > 1e-3 * norm           # <[D_a, D_b]> / 2i of a random vector: ~ <psi|psi> / sqrt(N) each
    assert np.abs(Dm.imag[apart]).max() <= 1e-13 * norm
    H = sum(dense_bond(D, L, i, j, xy, zz) for (i, j) in bonds)
    hpsi = H @ psi
    want = float(np.vdot(hpsi, hpsi).real)
    assert abs(Dm.sum().real - want) <= 1e-13 * len(bonds) ** 2 * norm and abs(Dm.sum().imag) <= 1e-13 * len(bonds) ** 2 * norm
    assert abs(e.sum() - np.vdot(psi, hpsi).real) <= 1e-13 * len(bonds) * norm


def test_majumdar_ghosh_values(D):
    """The product of singlets on (1,2), (3,4), ..., L = 8, periodic bond list: e = (-3/4, 0, -3/4, 0, ...), D_ab = 9/16 for two
    singlet bonds, D_aa = 3/16 for a bond between singlets, every other entry 0; S_D(pi) follows.  The open chain with J2 = J1/2 has
    that state as its unique ground state, E0 = -3L/8, gap 0.44."""
    L = 8
    psi = singlet_product(D, L)
    assert abs(np.vdot(psi, psi) - 1.0) <= 1e-14
    bonds = [(i, i % L + 1) for i in range(1, L + 1)]
    Dm, e = DR.gram(psi, L, L // 2, bonds, 1.0, 1.0)
    want_e = np.array([-0.75 if b % 2 == 0 else 0.0 for b in range(L)])
    want_D = np.zeros((L, L))
    for a in range(L):
        for b in range(L):
            if a % 2 == 0 and b % 2 == 0:
                want_D[a, b] = 9 / 16
            elif a == b:
                want_D[a, b] = 3 / 16
    assert np.abs(e - want_e).max() <= 1e-14 and np.abs(Dm - want_D).max() <= 1e-14
    ph = np.exp(1j * np.pi * np.arange(L))
    sd_pi = (ph.conj() @ Dm @ ph).real / L
    assert abs(sd_pi - ((L / 2) ** 2 * 9 / 16 + (L / 2) * 3 / 16) / L) <= 1e-13
    # the open J1-J2 chain at J2 = J1/2
    hop = [(i, i + 1, 0.5) for i in range(1, L)] + [(i, i + 2, 0.25) for i in range(1, L - 1)]
    zz = [(i, i + 1, 1.0) for i in range(1, L)] + [(i, i + 2, 0.5) for i in range(1, L - 1)]
    w, v = np.linalg.eigh(D.dense_H(L, L // 2, hop, zz, [0.0] * L))
    assert abs(w[0] + 3 * L / 8) <= 1e-12 and 0.40 < w[1] - w[0] < 0.48
    assert abs(abs(np.vdot(v[:, 0], psi)) - 1.0) <= 1e-12
