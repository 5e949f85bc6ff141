"""CPU-side proof of the thick-restart eigen-solver: the numpy restatement of the whole algorithm
(tests/eigs_ref.py, trlan_ref) against dense eigh of the oracle's matrices -- degenerate levels included, which is what the
confirmation step is for -- the Jacobi eigen-solver sd_sym_eig through ctypes, and the new exports.  No device is used."""
import ctypes as C

import numpy as np
import pytest

import eigs_cases as EC
from eigs_ref import U, trlan_ref

CASE_NAMES = ["xxz_open_L10", "xxz_ring_L10", "j1j2_ring_L12", "random_field_L10", "full_L8"]


@pytest.fixture(scope="module")
def dense(D, O):
    """name -> (H, ascending eigenvalues), computed once"""
    out = {}
    for name, case in EC.cases(D).items():
        H = EC.dense_matrix(case, D, O)
        assert np.array_equal(H, H.T)
        out[name] = (H, np.linalg.eigvalsh(H))
    return out


def seeds_for(N, seed, n=64):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(N) for _ in range(n)]


def test_the_two_dense_constructions_agree(D, O):
    """oracle/dense.py's matrix and the columns of the CPU oracle's apply_H are the same matrix (L = 10 ring): the L = 12 case
    uses the second, because the first takes minutes there."""
    case = EC.cases(D)["xxz_ring_L10"]
    A = D.dense_H(case["L"], case["nup"], case["hopping"], case["zz"], case["field"])
    B = EC.oracle_columns(case, O)
    assert np.abs(A - B).max() <= 8 * U * np.abs(A).max()


@pytest.mark.parametrize("k", EC.KS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_trlan_ref_against_dense_eigh(dense, name, k):
    """Conditions (a), (b), (d), (g) of tests/eigs_cases.py on the restatement; every multiplicity must be found: the J1-J2 ring at
    J2 = J1/2 has a twofold ground state, the rings +-k pairs, the full basis whole multiplets."""
    H, lam = dense[name]
    N = H.shape[0]
    E, X, info = trlan_ref(lambda x: H @ x, N, k, EC.basis_for(k), EC.TOL, True, seeds_for(N, 11))
    print(name, k, info)
    defect = EC.accept(H, lam, E, X, EC.TOL, next_level=info["next_level"], k=k)
    print(f"  orthonormality defect {defect:.2e}")
    assert info["restarts"] >= 3
    assert info["next_level"] is not None


def test_without_confirmation_a_degenerate_copy_is_missed(dense):
    """What the confirmation step is for: with confirm=False the sorted levels of the ring do not match the dense ones one to one
    for at least one of the seeded start vectors (a single Krylov sequence holds one direction per eigenspace; rounding does
    seed the second copy, but it emerges only after the level above it has converged).  k = 5 ends the window on the second copy
    of the ring's first +-k pair.  With confirm=True the same start vectors give every level."""
    H, lam = dense["xxz_ring_L10"]
    N = H.shape[0]
    k = 5
    assert lam[4] - lam[3] < 1e-12 and lam[5] - lam[4] > 0.1
    missed = 0
    for seed in range(4):
        E, X, info = trlan_ref(lambda x: H @ x, N, k, EC.basis_for(k), EC.TOL, False, seeds_for(N, 100 + seed))
        bad = len(E) < k or np.abs(E - lam[:k]).max() > 1e-6
        print(seed, np.round(E, 8), "missed" if bad else "complete")
        missed += bad
        E, X, info = trlan_ref(lambda x: H @ x, N, k, EC.basis_for(k), EC.TOL, True, seeds_for(N, 100 + seed))
        EC.accept(H, lam, E, X, EC.TOL, next_level=info["next_level"], k=k)
    print(np.round(lam[:10], 8))
    assert missed >= 1


def test_trlan_ref_runs_through_the_breakdown_path(D):
    """N = 6 (L = 4, nup = 2), k = 6: the basis is the whole space, the last step breaks down and every level comes back."""
    h, z, f = D.xxz_lists(4)
    H = D.dense_H(4, 2, h, z, f)
    lam = np.linalg.eigvalsh(H)
    E, X, info = trlan_ref(lambda x: H @ x, 6, 6, 9, EC.TOL, True, seeds_for(6, 3))
    EC.accept(H, lam, E, X, EC.TOL, k=6)
    assert info["next_level"] is None


def sym_cases():
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 31, 128):
        A = rng.standard_normal((n, n))
        yield f"random{n}", A + A.T
        # arrowhead plus tridiagonal: what the projected matrix of a restarted basis looks like
        l = n // 3
        T = np.diag(rng.standard_normal(n))
        for i in range(l):
            T[i, l] = T[l, i] = rng.standard_normal() * 1e-3
        for j in range(l, n - 1):
            T[j, j + 1] = T[j + 1, j] = abs(rng.standard_normal())
        yield f"arrow{n}", T
        # repeated eigenvalues
        Qm, _ = np.linalg.qr(rng.standard_normal((n, n)))
        d = np.repeat(rng.standard_normal((n + 2) // 3), 3)[:n]
        R = (Qm * d) @ Qm.T
        yield f"repeated{n}", (R + R.T) / 2


@pytest.mark.parametrize("name,A", list(sym_cases()), ids=[c[0] for c in sym_cases()])
def test_sym_eig_residual_orthogonality_eigenvalues(pkg, name, A):
    """sd_sym_eig (cyclic Jacobi): |A Z - Z diag(w)|_max <= 64 n u |A|_F, |Z^T Z - I|_max <= 64 n u, eigenvalues against
    numpy's eigvalsh within the first bar -- the form of Jacobi's backward error bounds, 64 a margin.  Largest ratios to
    n u |A|_F / n u observed over these inputs: residual 0.66, orthogonality 2.4, eigenvalues 1.4."""
    n = A.shape[0]
    w, Z = pkg.sym_eig(A)
    fro = np.linalg.norm(A)
    r1 = np.abs(A @ Z - Z * w).max() / (n * U * fro)
    r2 = np.abs(Z.T @ Z - np.eye(n)).max() / (n * U)
    r3 = np.abs(w - np.linalg.eigvalsh(A)).max() / (n * U * fro)
    print(name, f"residual {r1:.3f} orthogonality {r2:.3f} eigenvalues {r3:.3f} (in units of n u |A|_F, n u)")
    assert np.all(np.diff(w) >= 0)
    assert r1 <= 64 and r2 <= 64 and r3 <= 64


def test_sym_eig_argument_errors(pkg):
    dp = C.POINTER(C.c_double)
    a = np.zeros(4)
    for n in (0, 129):
        assert pkg.lib().sd_sym_eig(n, a.ctypes.data_as(dp), a.ctypes.data_as(dp), a.ctypes.data_as(dp)) == 1   # SD_EARG
    assert pkg.lib().sd_sym_eig(2, None, a.ctypes.data_as(dp), a.ctypes.data_as(dp)) == 1


def test_new_symbols_are_exported_and_prototyped(pkg):
    lib = C.CDLL(pkg.LIB_PATH)
    for name in ("sd_sym_eig", "sd_basis_rotate_dev", "sd_block_dots_dev", "sd_block_axpy_dev", "sd_lanczos_eigenpairs",
                 "sd_lanczos_eigenpairs_dev"):
        assert hasattr(lib, name), name
        assert name in pkg.PROTOTYPES, name
    for name in ("lanczos_eigenpairs", "lowest_eigenpairs", "spectral_gap", "lowest_levels", "sym_eig"):
        assert callable(getattr(pkg, name)), name
    # sd_eigs_info as the header lays it out: int, int, int64, int, int, double, int, double
    info = pkg._lib.sd_eigs_info
    assert [f[0] for f in info._fields_] == ["converged", "restarts", "applies", "basis_size", "workspace_vectors", "next_level",
                                             "have_next_level", "scale"]
    assert C.sizeof(info) == 48
