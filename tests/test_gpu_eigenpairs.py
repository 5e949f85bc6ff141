"""sd_lanczos_eigenpairs (thick-restart Lanczos) against dense eigh: the five models of
tests/test_eigs_ref_host.py in Float64 with a basis small enough to force restarts, a complex-Hermitian operator
(a Dzyaloshinskii-Moriya bond through operator_hamiltonian) and the momentum sectors of a ring (lowest_levels), then the edges.

Acceptance (tests/eigs_cases.py, accept): (a) sorted E against sorted lambda one to one within res_i + 16 N u |H|_F, which is
what makes a missed degenerate copy fail; (b) the residual recomputed from the dense matrix within tol |H|_2 + gamma and within
gamma of the returned one; (c) orthonormality |X^H X - I|_max within 16 times the defect of the numpy restatement (trlan_ref)
on the same case, floored at 64 u (not derivable to a constant: the summation orders differ); (d) restarts >= 2; (e)
workspace_vectors <= basis_size + 2; (f) info.applies equals the context's apply-count difference; (g) next_level within the
bar of lambda_k.

Orthonormality (c), |X^H X - I|_max, on an MI355X against the numpy restatement on the same case: 0 ... 7.7e-15 (largest:
full_L8, k = 8, restatement 1.2e-15) against 0 ... 1.6e-15 over the fifteen Float64 cells; the complex case 5.1e-16 against
6.6e-16.  Each cell prints both (run with -s)."""
import re

import numpy as np
import pytest

import eigs_cases as EC
from eigs_ref import U, trlan_ref

pytestmark = pytest.mark.gpu

CASE_NAMES = ["xxz_open_L10", "xxz_ring_L10", "j1j2_ring_L12", "random_field_L10", "full_L8"]


@pytest.fixture(scope="module")
def world(pkg, D, O):
    """name -> (case, model, H, ascending eigenvalues), computed once and read-only"""
    out = {}
    for name, case in EC.cases(D).items():
        H = EC.dense_matrix(case, D, O)
        H.setflags(write=False)
        m = pkg.build_model(case["L"], nup=case["nup"], hopping=case["hopping"], zz=case["zz"], onsite_field=np.array(case["field"]))
        out[name] = (case, m, H, np.linalg.eigvalsh(H))
    return out


def check_info(info, k, basis, restarts=True):
    assert info["converged"] == k
    if restarts:
        assert info["restarts"] >= 2                              # (d)
    assert info["workspace_vectors"] <= basis + 2                 # (e)


@pytest.mark.parametrize("k", EC.KS)
@pytest.mark.parametrize("name", CASE_NAMES)
def test_eigenpairs_against_dense_eigh(pkg, world, name, k):
    case, m, H, lam = world[name]
    N, basis = H.shape[0], EC.basis_for(k)
    a0 = m.ctx.apply_count()
    E, X, info = pkg.lowest_eigenpairs(m, k=k, basis_size=basis, tol=EC.TOL, seed=5)
    assert info["applies"] == m.ctx.apply_count() - a0            # (f)
    print(name, k, {n: v for n, v in info.items() if n != "residuals"})
    assert X.dtype == np.float64
    check_info(info, k, basis)
    defect = EC.accept(H, lam, E, X, EC.TOL, residuals=info["residuals"], next_level=info["next_level"], k=k)   # (a), (b), (g)
    assert info["next_level"] is not None
    rng = np.random.default_rng(11)
    _, Xr, _ = trlan_ref(lambda x: H @ x, N, k, basis, EC.TOL, True, [rng.standard_normal(N) for _ in range(64)])
    ref = float(np.abs(Xr.T @ Xr - np.eye(k)).max())
    print(f"  orthonormality defect {defect:.2e}, restatement {ref:.2e}")
    assert defect <= max(16 * ref, 64 * U)                        # (c)


def test_complex_hermitian_operator_with_a_dm_bond(pkg):
    """H + D (S_3 x S_4)_z on the open L = 8 chain, nup = 4, through applyH=: D (S^x_i S^y_j - S^y_i S^x_j) =
    (i D / 2)(S^+_i S^-_j - S^-_i S^+_j).  The dense matrix is the operator applied to the unit vectors on the device."""
    import torch
    m = pkg.XXZChain(8, nup=4)
    Dm = 0.8
    terms = pkg.op_string(0.5j * Dm, ("+", 3), ("-", 4)) + pkg.op_string(-0.5j * Dm, ("-", 3), ("+", 4))
    op = pkg.operator_hamiltonian(m, terms)
    N = m.N
    dev = torch.device("cuda", m.ctx.device)
    eye = torch.eye(N, dtype=torch.complex128, device=dev)
    cols = torch.empty_like(eye)
    for j in range(N):
        op(cols[j], eye[j], m)
    H = cols.cpu().numpy().T.copy()
    assert np.abs(H - H.conj().T).max() <= 4 * U * np.abs(H).max() and np.abs(H.imag).max() > 0.1
    H = (H + H.conj().T) / 2
    lam = np.linalg.eigvalsh(H)
    for k, basis in ((1, 7), (4, 10)):
        a0 = m.ctx.apply_count()
        E, X, info = pkg.lanczos_eigenpairs(op, m, k=k, basis_size=basis, tol=EC.TOL, seed=2)
        assert info["applies"] == m.ctx.apply_count() - a0
        assert X.dtype == np.complex128 and np.abs(X.imag).max() > 1e-3
        check_info(info, k, basis)
        defect = EC.accept(H, lam, E, X, EC.TOL, residuals=info["residuals"], next_level=info["next_level"], k=k)
        rng = np.random.default_rng(12)
        seeds = [rng.standard_normal(N) + 1j * rng.standard_normal(N) for _ in range(64)]
        _, Xr, _ = trlan_ref(lambda x: H @ x, N, k, basis, EC.TOL, True, seeds)
        ref = float(np.abs(Xr.conj().T @ Xr - np.eye(k)).max())
        print(f"  k={k}: orthonormality defect {defect:.2e}, restatement {ref:.2e}")
        assert defect <= max(16 * ref, 64 * U)


def test_lowest_levels_of_every_momentum_sector(pkg, world):
    """lowest_levels(momentum=n) on the L = 10 ring for every n against the ring's dense spectrum grouped by momentum: H and the
    translation T commute, so the eigenvectors of H + 0.37 (T + T^H)/2 + 0.21 (T - T^H)/(2i) are common eigenvectors; each
    gets its label from quantum_numbers and its level from <v|H|v>."""
    case, m, H, _ = world["xxz_ring_L10"]
    L, N = case["L"], H.shape[0]
    st = m.states.astype(np.uint64)
    rot = ((st << np.uint64(1)) | (st >> np.uint64(L - 1))) & np.uint64((1 << L) - 1)
    T = np.zeros((N, N))
    T[m.rank(rot), np.arange(N)] = 1.0
    assert np.abs(T @ H - H @ T).max() == 0.0
    _, V = np.linalg.eigh(H + 0.37 * (T + T.T) / 2 + 0.21 * (T - T.T) / 2j)
    levels = {n: [] for n in range(L)}
    for i in range(N):
        n = pkg.quantum_numbers(V[:, i], m)["momentum"]
        assert n is not None
        levels[n].append(float(np.real(V[:, i].conj() @ H @ V[:, i])))
    k = 3
    for n in range(L):
        lam = np.sort(levels[n])
        assert len(lam) >= 20
        E, X = pkg.lowest_levels(m, k, momentum=n, seed=3, tol=EC.TOL)
        X = X.cpu().numpy()
        print("momentum", n, E, lam[:k])
        EC.accept(H, lam, E, X, EC.TOL, k=k)
        for i in range(k):
            assert pkg.quantum_numbers(X[:, i], m)["momentum"] == n


def test_all_levels_through_the_breakdown_path(pkg, D):
    """N = 6 (L = 4, nup = 2), k = 6: the basis is clamped to N, the last step breaks down and every level comes back"""
    m = pkg.XXZChain(4, nup=2)
    h, z, f = D.xxz_lists(4)
    H = D.dense_H(4, 2, h, z, f)
    E, X, info = pkg.lowest_eigenpairs(m, k=6, basis_size=9, tol=EC.TOL)
    assert info["basis_size"] == 6 and info["next_level"] is None
    check_info(info, 6, 6, restarts=False)
    EC.accept(H, np.linalg.eigvalsh(H), E, X, EC.TOL, residuals=info["residuals"], k=6)


def test_k1_is_the_groundstate_of_lanczos_groundstate(pkg, world):
    case, m, H, lam = world["xxz_open_L10"]
    N = H.shape[0]
    E, X, info = pkg.lowest_eigenpairs(m, k=1, tol=EC.TOL)
    E0, gs = pkg.lanczos_groundstate(pkg.apply_H, m, lanc_m=100)
    res = info["residuals"][0]
    assert abs(E[0] - E0) <= res + 16 * N * U * np.linalg.norm(H)
    d = min(np.linalg.norm(X[:, 0] - gs), np.linalg.norm(X[:, 0] + gs))
    print("state difference", d, "bar", np.sqrt(res / (lam[1] - lam[0])))
    assert d <= np.sqrt(res / (lam[1] - lam[0]))


def test_argument_errors(pkg, world):
    case, m, H, lam = world["xxz_open_L10"]
    small = pkg.XXZChain(4, nup=2)
    for mod, kw, word in ((small, dict(k=7), "nev must be <= min"), (m, dict(k=25, basis_size=40), "nev must be <= min"),
                          (m, dict(k=0), "nev must be >= 1"), (m, dict(k=4, basis_size=6), "basis_size must be >= nev + 3"),
                          (m, dict(k=4, basis_size=129), "basis_size must be <= 128")):
        with pytest.raises(pkg.ArgumentError, match=re.escape(word)):
            pkg.lowest_eigenpairs(mod, **kw)
    sharded = pkg.XXZChain(16, nup=8)
    sharded.set_shard(0, 2)
    with pytest.raises(pkg.ArgumentError):
        pkg.lowest_eigenpairs(sharded, k=2)
    E, _, _ = pkg.lowest_eigenpairs(m, k=1, tol=EC.TOL, vectors=False)                      # the context still works
    assert abs(E[0] - lam[0]) <= 1e-9


def test_max_applies_returns_the_pairs_locked_so_far(pkg, world):
    case, m, H, lam = world["random_field_L10"]
    k, basis = 8, EC.basis_for(8)
    _, _, full = pkg.lowest_eigenpairs(m, k=k, basis_size=basis, tol=EC.TOL, seed=5, confirm=False)
    E, X, info = pkg.lowest_eigenpairs(m, k=k, basis_size=basis, tol=EC.TOL, seed=5, confirm=False, max_applies=full["applies"] // 2)
    print(info)
    nc = info["converged"]
    assert 1 <= nc < k and len(E) == nc and X.shape == (H.shape[0], nc)
    assert info["applies"] <= full["applies"] // 2 + nc                                     # the residuals' applies come on top
    EC.accept(H, lam, E, X, EC.TOL, residuals=info["residuals"], k=nc)


def test_same_call_same_bits_and_device_start_vector(pkg, world):
    import torch
    case, m, H, lam = world["xxz_ring_L10"]
    N = H.shape[0]
    kw = dict(k=4, basis_size=EC.basis_for(4), tol=EC.TOL, seed=9)
    E1, X1, i1 = pkg.lowest_eigenpairs(m, **kw)
    E2, X2, i2 = pkg.lowest_eigenpairs(m, **kw)
    assert np.array_equal(E1, E2) and np.array_equal(X1, X2) and np.array_equal(i1["residuals"], i2["residuals"])
    psi0 = np.random.default_rng(1).standard_normal(N)
    Eh, Xh, ih = pkg.lowest_eigenpairs(m, psi0=psi0, **kw)
    Ed, Xd, idv = pkg.lowest_eigenpairs(m, psi0=torch.as_tensor(psi0, device=torch.device("cuda", m.ctx.device)), **kw)
    assert torch.is_tensor(Xd) and Xd.shape == (N, 4)
    assert np.array_equal(Eh, Ed) and np.array_equal(Xh, Xd.cpu().numpy()) and ih["applies"] == idv["applies"]
    E0, gap, deg = pkg.spectral_gap(m, tol=EC.TOL)
    assert deg == 1 and abs(E0 - lam[0]) <= 1e-9 and abs(gap - (lam[1] - lam[0])) <= 1e-8
    j = world["j1j2_ring_L12"]
    E0, gap, deg = pkg.spectral_gap(j[1], tol=EC.TOL)
    assert deg == 2 and abs(E0 + 4.5) <= 1e-9 and abs(gap) <= 1e-8                       # E1 - E0 of a twofold ground state
