"""Site-resolved KPM correlations on the GPU: the projection kernel against numpy, the moments against the restatement
(tests/site_moments_ref.py, proven on the CPU by tests/test_site_moments_host.py) run on the oracle, S(q,w) from the site moments
against the oracle's kpm_sqw, the one-source shortcut and its guard, the correlation matrix, batching, a full-size run and
the refusals."""
import ctypes as C

import numpy as np
import pytest

import site_moments_ref as R

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)


def rand_vec(N, cplx, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(N)
    if cplx:
        x = x + 1j * rng.standard_normal(N)
    return x / np.linalg.norm(x)


def j1j2_lists(L, J1=1.0, J2=0.4):
    hop = [(i, i % L + 1, J1 / 2) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2 / 2) for i in range(1, L + 1)]
    zz = [(i, i % L + 1, J1) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2) for i in range(1, L + 1)]
    return hop, zz


def all_states(m):
    return m.states_range(0, m.N)


def check_project(pkg, m):
    sz = R.site_sz(all_states(m), m.L)
    for cplx in (False, True):
        bra = rand_vec(m.N, cplx, 11 + m.L)
        ket = rand_vec(m.N, True, 12 + m.L)
        got = pkg.site_project(m, bra, ket)
        want = R.project(sz, bra, ket)
        bar = 1e-13 * float(np.sum(np.abs(bra) * np.abs(ket)))
        err = np.abs(got - want).max()
        print(f"L={m.L} nup={m.nup} N={m.N} path={pkg.lib().sd_model_path(m.h)} bra={'c128' if cplx else 'f64'}: {err:.2e} (bar {bar:.2e})")
        assert got.shape == (m.L,) and got.dtype == np.complex128
        assert err <= bar
        again = pkg.site_project(m, bra, ket)
        assert np.array_equal(got.view(np.float64), again.view(np.float64))       # same call twice: equal bits


# ---- 1. the projection kernel ----
@pytest.mark.parametrize("L,nup", [(4, 2), (9, 4), (12, 6), (16, 8), (20, 10), (13, 0), (13, 13)])
@pytest.mark.parametrize("boundary", ["open", "periodic"])
def test_site_project_tiled_sectors(pkg, L, nup, boundary):
    check_project(pkg, pkg.XXZChain(L, Jz=0.5, hz=0.3, nup=nup, boundary=boundary))


def test_site_project_j1j2(pkg):
    L = 14
    hop, zz = j1j2_lists(L)
    check_project(pkg, pkg.build_model(L, nup=7, hopping=hop, zz=zz, onsite_field=np.full(L, 0.1)))


@pytest.mark.parametrize("L", [10, 14])
def test_site_project_full_basis(pkg, L):
    check_project(pkg, pkg.XXZChain(L, Jz=0.5))


def test_site_project_per_row_plan(pkg):
    m = pkg.XXZChain(24, nup=2, boundary="periodic").adjacent_sector(-1)
    assert pkg.lib().sd_model_path(m.h) == 0
    check_project(pkg, m)
    m2 = pkg.XXZChain(24, nup=2, boundary="periodic").adjacent_sector(1)
    check_project(pkg, m2)


def test_site_project_device_tensors(pkg):
    import torch
    m = pkg.XXZChain(16, nup=8, boundary="periodic")
    dev = torch.device("cuda", m.ctx.device)
    sz = R.site_sz(all_states(m), m.L)
    for cplx in (False, True):
        bra, ket = rand_vec(m.N, cplx, 1), rand_vec(m.N, True, 2)
        got = pkg.site_project(m, torch.as_tensor(bra, device=dev), torch.as_tensor(ket, device=dev))
        assert np.array_equal(got.view(np.float64), pkg.site_project(m, bra, ket).view(np.float64))
        assert np.abs(got - R.project(sz, bra, ket)).max() <= 1e-13 * float(np.sum(np.abs(bra) * np.abs(ket)))


# ---- 2. the moments against the restatement on the oracle ----
def moments_case(pkg, O, L, boundary, cplx, M=1024):
    nup = L // 2
    m = pkg.XXZChain(L, Jz=0.8, nup=nup, boundary=boundary)
    ref = O.XXZChain(L, Jz=0.8, nup=nup, boundary=boundary)
    psi0 = rand_vec(m.N, cplx, 100 + L)
    a, b = 0.55 * L, -0.1
    sources = [2, L - 3]
    got = pkg.kpm_site_moments(psi0, m, M, a, b, sources=sources)
    want = R.site_moments(O, ref, psi0, sources, M, a, b)
    err = np.abs(got - want).max()
    print(f"L={L} {boundary} {'c128' if cplx else 'f64'}: site moments vs restatement {err:.2e}")
    assert got.shape == (2, M, L)
    assert err <= 1e-12
    if not cplx:
        assert np.abs(got.imag).max() == 0.0


@pytest.mark.parametrize("L", [16, 18])
@pytest.mark.parametrize("boundary", ["open", "periodic"])
@pytest.mark.parametrize("cplx", [False, True])
def test_site_moments_match_the_restatement(pkg, O, L, boundary, cplx):
    moments_case(pkg, O, L, boundary, cplx)


# ---- 3. S(q,w) from all sources against the oracle's kpm_sqw ----
@pytest.mark.parametrize("L", [12, 16])
@pytest.mark.parametrize("boundary", ["open", "periodic"])
def test_sqw_from_all_sources_matches_the_oracle(pkg, O, L, boundary):
    nup = L // 2
    m = pkg.XXZChain(L, nup=nup, boundary=boundary)
    ref = O.XXZChain(L, nup=nup, boundary=boundary)
    omega = np.linspace(0.0, 4.0, 60)
    a, b = 0.55 * L, 0.0
    for cplx in (False, True):
        psi0 = rand_vec(m.N, cplx, 7 + L)
        want = O.kpm_sqw(ref, psi0, O.momenta(ref), omega, a, b, kpm_m=1024)
        got = pkg.kpm_sqw_sites(psi0, m, pkg.momenta(m), omega, a=a, b=b, kpm_m=1024)
        err, bar = np.abs(got - want).max(), 1e-8 * max(1.0, np.abs(want).max())
        print(f"L={L} {boundary} {'c128' if cplx else 'f64'}: kpm_sqw_sites vs O.kpm_sqw {err:.2e} (bar {bar:.2e})")
        assert got.shape == want.shape
        assert err <= bar
        via_api = pkg.dynamical_structure_factor(m, psi0, pkg.momenta(m), omega, method="kpm_sites", a=a, b=b, kpm_m=1024)
        assert np.array_equal(via_api, got)


# ---- 4. one source for a translation-invariant state ----
def dense_ground_state(O, ref):
    eye = np.eye(ref.N)
    H = np.array([O.apply_H(ref, eye[k]) for k in range(ref.N)]).T
    w, V = np.linalg.eigh(H)
    assert w[1] - w[0] > 1e-6
    return V[:, 0].copy()


@pytest.mark.parametrize("L", [12, 14])
def test_translation_invariant_one_source(pkg, O, L):
    nup = L // 2
    m = pkg.XXZChain(L, nup=nup, boundary="periodic")
    ref = O.XXZChain(L, nup=nup, boundary="periodic")
    gs = dense_ground_state(O, ref)
    omega = np.linspace(0.0, 4.0, 60)
    a, b = 0.55 * L, 0.0
    want = O.kpm_sqw(ref, gs, O.momenta(ref), omega, a, b, kpm_m=1024)
    for source in (1, L // 2):
        got = pkg.kpm_sqw_sites(gs, m, pkg.momenta(m), omega, a=a, b=b, kpm_m=1024, translation_invariant=True, source=source)
        defect = pkg.kpm_sqw_sites.last_defect
        err, bar = np.abs(got - want).max(), 1e-8 * max(1.0, np.abs(want).max())
        print(f"L={L} source={source}: one source vs O.kpm_sqw {err:.2e} (bar {bar:.2e}), defect {defect:.2e}")
        assert err <= bar
        assert defect <= 1e-10
    with pytest.raises(pkg.ArgumentError):                                # a random state is not invariant
        pkg.kpm_sqw_sites(rand_vec(m.N, True, 3), m, pkg.momenta(m), omega, a=a, b=b, kpm_m=64, translation_invariant=True)
    mo = pkg.XXZChain(L, nup=nup, boundary="open")                        # nor is the open chain
    with pytest.raises(pkg.ArgumentError):
        pkg.kpm_sqw_sites(gs, mo, pkg.momenta(mo), omega, a=a, b=b, kpm_m=64, translation_invariant=True)
    # the library's own guard, without the mirror's list check: the open chain's ground state has a large defect
    refo = O.XXZChain(L, nup=nup, boundary="open")
    gso = dense_ground_state(O, refo)
    S = np.empty((L, len(omega)))
    q = np.ascontiguousarray(pkg.momenta(mo), dtype=np.float64)
    src = np.array([1], dtype=np.int32)
    d = C.c_double(0.0)
    pkg.check(pkg.lib().sd_kpm_sqw_sites(mo.ctx.h, mo.h, 1, gso.ctypes.data, len(gso), q.ctypes.data_as(_dp), len(q),
                                         omega.ctypes.data_as(_dp), len(omega), src.ctypes.data_as(_ip), 1, 1, 1, a, b, 64, 0, 0,
                                         S.ctypes.data_as(_dp), C.byref(d)), mo.ctx.h)
    print(f"L={L} open chain: defect {d.value:.2e}")
    assert d.value >= 0.05


# ---- 5. the correlation matrix ----
def test_correlation_matrix_against_dense_spectral_moments(pkg, O, D):
    L, nup, M = 10, 5, 400
    for boundary in ("open", "periodic"):
        hop, zz, field = D.xxz_lists(L, boundary=boundary)
        H = D.dense_H(L, nup, hop, zz, field)
        m = pkg.XXZChain(L, nup=nup, boundary=boundary)
        w = np.linalg.eigvalsh(H)
        a, b = (w[-1] - w[0]) / (2 * 0.99), (w[-1] + w[0]) / 2
        omega = np.linspace(-0.5, 6.0, 90)
        g = O.get_kernel(M, "jackson")
        for cplx in (False, True):
            psi0 = rand_vec(m.N, cplx, 21)
            E0 = float(np.real(np.vdot(psi0, H @ psi0)))
            sources = list(range(1, L + 1))
            mu = R.dense_spectral_moments(H, all_states(m), L, psi0, sources, M, a, b)
            want = np.empty((L, L, len(omega)), dtype=np.complex128)
            for s in range(L):
                for i in range(L):
                    md = mu[s, :, i] * g
                    want[i, s] = R.reconstruct_signed(md.real, omega, a, b, E0) + 1j * R.reconstruct_signed(md.imag, omega, a, b, E0)
            got = pkg.kpm_correlation_matrix(psi0, m, omega, a=a, b=b, kpm_m=M)
            scale = np.abs(want).max()
            err = np.abs(got - want).max()
            herm = np.abs(got - np.conj(got.transpose(1, 0, 2))).max()
            colsum = np.abs(got.sum(axis=0)).max()
            print(f"{boundary} {'c128' if cplx else 'f64'}: C vs dense {err:.2e}, |C - C^H| {herm:.2e}, |sum_i C_ij| {colsum:.2e}, max|C| {scale:.2e}")
            assert got.shape == (L, L, len(omega))
            assert err <= 1e-8 * scale
            assert herm <= 1e-8 * scale               # C_ij = conj(C_ji)
            assert colsum <= 1e-8 * scale             # sum_i S^z_i = 0 in the Sz = 0 sector
            assert (got.real < -1e-3 * scale).any()   # off-diagonal entries are signed: nothing is clamped
            part = pkg.kpm_correlation_matrix(psi0, m, omega, sources=[3, 7], a=a, b=b, kpm_m=M)
            assert np.array_equal(part, got[:, [2, 6], :])


# ---- 6. batched sources = one at a time, bit for bit ----
def test_batched_sources_are_bit_identical(pkg):
    L = 14
    m = pkg.XXZChain(L, Jz=0.7, nup=7, boundary="periodic")
    for cplx in (False, True):
        psi0 = rand_vec(m.N, cplx, 5)
        n0 = m.ctx.apply_count()
        batched = pkg.kpm_site_moments(psi0, m, 200, 8.0, 0.1)
        assert m.ctx.apply_count() - n0 == L * 199          # M - 1 applies per source
        m.ctx.set_q_batch(False)
        try:
            single = pkg.kpm_site_moments(psi0, m, 200, 8.0, 0.1)
        finally:
            m.ctx.set_q_batch(True)
        assert batched.shape == (L, 200, L)
        assert np.array_equal(batched.view(np.float64), single.view(np.float64))
        one = pkg.kpm_site_moments(psi0, m, 200, 8.0, 0.1, sources=[5])
        assert np.array_equal(one[0].view(np.float64), batched[4].view(np.float64))


# ---- 7. full size, no oracle ----
def test_full_size_identities(pkg):
    import torch
    L, nup, M = 28, 14, 8
    m = pkg.XXZChain(L, nup=nup, boundary="periodic")
    dev = torch.device("cuda", m.ctx.device)
    gen = torch.Generator(device=dev)
    gen.manual_seed(28)
    psi0 = torch.randn(m.N, dtype=torch.complex128, device=dev, generator=gen)
    a, b = 16.0, -2.0
    sources = [1, 14]
    mu = pkg.kpm_site_moments(psi0, m, M, a, b, sources=sources)
    torch.cuda.synchronize(dev)
    n2 = float((psi0.real ** 2 + psi0.imag ** 2).sum().item())
    assert mu.shape == (2, M, L)
    # the projection of S^z_j psi0 and of H~ S^z_j psi0, formed with torch from the basis states (the operator-level calls are
    # pinned bit-exact by their own tests)
    states = torch.as_tensor(all_states(m).astype(np.int64), device=dev)
    for s, j in enumerate(sources):
        assert abs(mu[s, 0, j - 1] - 0.25 * n2) <= 1e-13 * n2                      # mu_0^{jj} = |psi0|^2 / 4
        tot = np.abs(mu[s].sum(axis=1))
        print(f"source {j}: max_n |sum_i mu_n^(ij)| / |psi0|^2 = {tot.max() / n2:.2e}")
        assert tot.max() <= 1e-12 * n2                                             # sum_i S^z_i = 0 in the Sz = 0 sector
        v0 = psi0 * (((states >> (j - 1)) & 1).to(torch.float64) - 0.5)
        v1 = torch.empty_like(v0)
        pkg.apply_rescaled_H(v1, v0, pkg.apply_H, m, a, b)
        for n, v in ((0, v0), (1, v1)):
            w = torch.conj(psi0) * v
            want = np.array([complex((w * (((states >> i) & 1).to(torch.float64) - 0.5)).sum().item()) for i in range(L)])
            bar = 1e-13 * float((psi0.abs() * v.abs()).sum().item())
            err = np.abs(mu[s, n] - want).max()
            print(f"source {j} n={n}: {err:.2e} (bar {bar:.2e})")
            assert err <= bar
        del v0, v1, w


# ---- 8. refusals ----
def test_refusals_and_the_spectrum_guard(pkg, O):
    L = 16
    m = pkg.XXZChain(L, nup=8, boundary="periodic")
    psi0 = rand_vec(m.N, False, 1)
    for bad in ([0], [L + 1], [1, L + 1]):
        with pytest.raises(pkg.ArgumentError):
            pkg.kpm_site_moments(psi0, m, 16, 9.0, 0.0, sources=bad)
    with pytest.raises(pkg.ArgumentError):
        pkg.kpm_site_moments(psi0, m, 1, 9.0, 0.0, sources=[1])
    with pytest.raises(pkg.DimensionMismatch):
        pkg.kpm_site_moments(psi0[:-1], m, 16, 9.0, 0.0, sources=[1])
    sh = pkg.XXZChain(L, nup=8, boundary="periodic")
    sh.set_shard(0, 2)
    with pytest.raises(pkg.ArgumentError):
        pkg.kpm_site_moments(psi0, sh, 16, 9.0, 0.0, sources=[1])
    with pytest.raises(pkg.ArgumentError):
        pkg.site_project(sh, psi0, psi0.astype(np.complex128))
    # translation_invariant with two sources; all-sources with a site missing
    omega = np.linspace(0, 3, 10)
    q = np.ascontiguousarray(pkg.momenta(m), dtype=np.float64)
    S = np.empty((L, len(omega)))

    def raw(src, ti):
        src = np.array(src, dtype=np.int32)
        return pkg.lib().sd_kpm_sqw_sites(m.ctx.h, m.h, 1, psi0.ctypes.data, len(psi0), q.ctypes.data_as(_dp), len(q),
                                          omega.ctypes.data_as(_dp), len(omega), src.ctypes.data_as(_ip), len(src), ti, 1, 9.0, 0.0,
                                          16, 0, 0, S.ctypes.data_as(_dp), None)
    assert raw([1, 2], 1) == 1                                   # SD_EARG
    assert raw(list(range(1, L)), 0) == 1
    assert raw([1] * L, 0) == 1
    assert raw(list(range(1, L + 1)), 0) == 0
    with pytest.raises(pkg.ArgumentError):
        pkg.dynamical_structure_factor(m, psi0, q, omega, method="kpm_sites", component="+-")
    # bounds that do not contain the spectrum: SD_EARG naming a and b; the same context then computes correctly
    with pytest.raises(pkg.ArgumentError) as ei:
        pkg.kpm_site_moments(psi0, m, 256, 0.1, 0.0, sources=[1, 2])
    assert "a = 0.1" in str(ei.value) and "b = 0.0" in str(ei.value)
    moments_case(pkg, O, 16, "periodic", True)
