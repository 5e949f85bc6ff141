"""tests/pair_ref.py against Kronecker-product operators (oracle/dense.py::site_op) on the full 2^L space, the sector embedded with
sector_states: <psi| S^+_i S^-_j |psi> = (S^-_i psi)^dagger (S^-_j psi) and <psi| S^z_i S^z_j |psi>, every ordered pair, real and
complex random vectors.  CPU only."""
import numpy as np
import pytest

import pair_ref as PR

# (L, nup); None: the full basis
CASES = [(2, 1), (5, 2), (6, 0), (6, 1), (6, 5), (6, 6), (7, 3), (9, 4), (10, 3), (10, 5), (10, 9), (8, None)]


def embed(D, psi, L, nup):
    if nup is None:
        return psi.astype(np.complex128)
    full = np.zeros(1 << L, dtype=np.complex128)
    full[D.sector_states(L, nup).astype(np.int64)] = psi
    return full


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("L,nup", CASES)
def test_pair_ref_matches_kronecker_operators(D, L, nup, cplx):
    N = (1 << L) if nup is None else len(D.sector_states(L, nup))
    rng = np.random.default_rng(1000 * L + (77 if nup is None else nup) + (500 if cplx else 0))
    psi = rng.standard_normal(N) + (1j * rng.standard_normal(N) if cplx else 0.0)
    if not cplx:
        psi = psi.real.astype(np.float64)
    full = embed(D, psi, L, nup)
    norm = float(np.vdot(psi, psi).real)
    lowered = [D.site_op(D.SM, i, L) @ full for i in range(1, L + 1)]
    szd = [D.site_op(D.SZ, i, L) @ full for i in range(1, L + 1)]
    G = np.array([[np.vdot(lowered[i], lowered[j]) for j in range(L)] for i in range(L)])
    Z = np.array([[np.vdot(szd[i], szd[j]) for j in range(L)] for i in range(L)])
    g = PR.correlations(psi, L, nup, "+-")
    z = PR.correlations(psi, L, nup, "zz")
    assert g.shape == z.shape == (L, L)
    assert np.abs(g - G).max() <= 1e-13 * norm
    assert np.abs(z - Z).max() <= 1e-13 * norm
    if not cplx:
        assert np.all(g.imag == 0.0)
    elif nup not in (0, L):
        assert np.abs(g.imag).max() > 1e-3            # the conjugation is exercised
    # a listed subset gives the same numbers as the matrix
    pairs = [(1, L), (L, 1), (1, 1), (max(1, L // 2), L)]
    sub = PR.correlations(psi, L, nup, "+-", pairs=pairs)
    assert all(sub[(i, j)] == g[i - 1, j - 1] for (i, j) in pairs)
