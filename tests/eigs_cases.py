"""The models, dense matrices and acceptance conditions shared by the eigen-solver tests (test_eigs_ref_host.py for the numpy
restatement, test_gpu_eigenpairs.py for the library)."""
import numpy as np

U = 2.0 ** -53
TOL = 1e-10
KS = (1, 4, 8)


def basis_for(k):
    """a basis small enough to force restarts: nev + 6 columns"""
    return k + 6


def _ring(L, J1, J2):
    hop = [(i, i % L + 1, J1 / 2) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2 / 2) for i in range(1, L + 1)]
    zz = [(i, i % L + 1, J1) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2) for i in range(1, L + 1)]
    return hop, zz


def cases(D):
    """name -> dict(L, nup, hopping, zz, field)"""
    out = {}
    h, z, f = D.xxz_lists(10)
    out["xxz_open_L10"] = dict(L=10, nup=5, hopping=h, zz=z, field=f)
    h, z, f = D.xxz_lists(10, boundary="periodic")
    out["xxz_ring_L10"] = dict(L=10, nup=5, hopping=h, zz=z, field=f)
    h, z = _ring(12, 1.0, 0.5)
    out["j1j2_ring_L12"] = dict(L=12, nup=6, hopping=h, zz=z, field=[0.0] * 12)
    h, z, _ = D.xxz_lists(10)
    out["random_field_L10"] = dict(L=10, nup=5, hopping=h, zz=z, field=list(np.random.default_rng(20261021).uniform(-1, 1, 10)))
    h, z, f = D.xxz_lists(8, Jxy=1.0, Jz=0.7, hz=0.3)
    out["full_L8"] = dict(L=8, nup=None, hopping=h, zz=z, field=f)
    return out


def dense_matrix(case, D, O):
    """The sector's matrix: oracle/dense.py's up to L = 10; at L = 12, where its 4096 x 4096 Kronecker products take minutes, the
    columns H e_j from the CPU oracle's apply_H (test_eigs_ref_host.py checks that the two constructions agree at L = 10)."""
    if case["L"] <= 10:
        return D.dense_H(case["L"], case["nup"], case["hopping"], case["zz"], case["field"])
    return oracle_columns(case, O)


def oracle_columns(case, O):
    m = O.build_model(case["L"], nup=case["nup"], hopping=case["hopping"], onsite_field=case["field"], zz=case["zz"])
    H = np.empty((m.N, m.N))
    e = np.zeros(m.N)
    for j in range(m.N):
        e[j] = 1.0
        H[:, j] = np.real(O.apply_H(m, e))
        e[j] = 0.0
    return H


def accept(H, lam, E, X, tol, residuals=None, next_level=None, k=None):
    """Conditions (a), (b) and (g) of the solver tests; returns the orthonormality defect of X for (c).
    (a) sorted E against sorted lam one to one: |E_i - lam_i| <= res_i + 16 N u |H|_F (an eigenvalue lies within |r| of the Ritz
        value of a unit vector; the second term covers eigh);
    (b) r_i = |H x_i - E_i x_i| recomputed from H: r_i <= tol |H|_2 + gamma_i, gamma_i = (nnz_row + 2) u (||H||x_i|| + |E_i|), and
        |r_i - residuals[i]| <= gamma_i;
    (g) next_level within bar (a) of lam[k] (with its own residual unknown, the bar is tol |H|_2 + 16 N u |H|_F)."""
    N = H.shape[0]
    k = len(E) if k is None else k
    assert len(E) == k and X.shape == (N, k)
    assert np.all(np.diff(E) >= 0)
    fro, two = np.linalg.norm(H), np.linalg.norm(H, 2)
    nnz = int((H != 0).sum(axis=1).max())
    aH = np.abs(H)
    for i in range(k):
        x = X[:, i]
        r = np.linalg.norm(H @ x - E[i] * x)
        gamma = (nnz + 2) * U * (np.linalg.norm(aH @ np.abs(x)) + abs(E[i]))
        print(f"  pair {i}: E={E[i]:+.12f} |E-lam|={abs(E[i] - lam[i]):.2e} r={r:.2e} bar_b={tol * two + gamma:.2e} gamma={gamma:.2e}"
              + (f" |r-res|={abs(r - residuals[i]):.2e}" if residuals is not None else ""))
        res = r if residuals is None else residuals[i]
        assert abs(E[i] - lam[i]) <= res + 16 * N * U * fro, (i, E[i], lam[i], res)
        assert r <= tol * two + gamma, (i, r, tol * two + gamma)
        if residuals is not None:
            assert abs(r - residuals[i]) <= gamma, (i, r, residuals[i], gamma)
    if next_level is not None and k < N:
        print(f"  next level {next_level:+.12f} lam[k]={lam[k]:+.12f}")
        assert abs(next_level - lam[k]) <= tol * two + 16 * N * U * fro, (next_level, lam[k])
    return float(np.abs(X.conj().T @ X - np.eye(k)).max()) if k else 0.0
