"""Transverse S(q,w): S^-_q / S^+_q between adjacent sectors, the adjacent-sector model, and S^{+-}, S^{-+}, S^{xx} against
a composition of the CPU oracle's recursions on the target sector (the operator itself against tests/transverse_ref.py)."""
import ctypes as C
import math

import numpy as np
import pytest

import transverse_ref as R

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)


def j1j2_lists(L, J1=1.0, J2=0.4):
    hop = [(i, i % L + 1, J1 / 2) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2 / 2) for i in range(1, L + 1)]
    zz = [(i, i % L + 1, J1) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2) for i in range(1, L + 1)]
    return hop, zz


def rand_psi(N, cplx, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(N)
    if cplx:
        x = x + 1j * rng.standard_normal(N)
    return x / np.linalg.norm(x)


def check_phi(got, want, q):
    assert got.shape == want.shape and got.dtype == np.complex128
    if q == 0.0:
        assert np.array_equal(got, want)
    else:
        scale = max(np.abs(want).max(), 1e-300)
        assert np.abs(got - want).max() <= 2e-15 * scale


# ---- 1. the operator against numpy ----
@pytest.mark.parametrize("L,nup", [(4, 2), (9, 4), (12, 6), (16, 8), (20, 10), (13, 0), (13, 13)])
@pytest.mark.parametrize("boundary", ["open", "periodic"])
def test_operator_matches_numpy_xxz(pkg, L, nup, boundary):
    m = pkg.XXZChain(L, Jz=0.5, hz=0.3, nup=nup, boundary=boundary)
    qs = pkg.momenta(m) if L <= 16 else pkg.momenta(m)[:4]
    for cplx in (False, True):
        psi = rand_psi(m.N, cplx, L + nup)
        for q in qs:
            for op, fn in (("minus", pkg.Sminus_q_vector), ("plus", pkg.Splus_q_vector)):
                target = nup + (-1 if op == "minus" else 1)
                got = fn(m, psi, q)
                if target < 0 or target > L:
                    assert len(got) == 0
                    continue
                check_phi(got, R.spm(L, nup, psi, q, op), q)


def test_operator_matches_numpy_j1j2(pkg):
    L, nup = 14, 7
    hop, zz = j1j2_lists(L)
    m = pkg.build_model(L, nup=nup, hopping=hop, zz=zz, onsite_field=np.full(L, 0.1))
    for cplx in (False, True):
        psi = rand_psi(m.N, cplx, 3)
        for q in pkg.momenta(m):
            check_phi(pkg.Sminus_q_vector(m, psi, q), R.spm(L, nup, psi, q, "minus"), q)
            check_phi(pkg.Splus_q_vector(m, psi, q), R.spm(L, nup, psi, q, "plus"), q)


@pytest.mark.parametrize("L", [5, 10, 14])
def test_full_basis_matches_the_site_operators(pkg, L):
    m = pkg.XXZChain(L, Jz=0.5)
    psi = rand_psi(m.N, True, L)
    for q in (0.0, 2 * np.pi * 2 / L):
        for name, fn in (("minus", pkg.Sminus_q_vector), ("plus", pkg.Splus_q_vector)):
            want = np.zeros(m.N, complex)
            for r in range(L):
                want += np.exp(1j * q * r) / np.sqrt(L) * pkg.create_spin_operator(r + 1, name)(psi, m)
            got = fn(m, psi, q)
            assert np.abs(got - want).max() <= 1e-14
            check_phi(got, R.spm(L, None, psi, q, name), q)


def test_per_row_plan(pkg):
    L, nup = 24, 2
    m = pkg.XXZChain(L, nup=nup, boundary="periodic")
    for dn, op, fn in ((-1, "minus", pkg.Sminus_q_vector), (1, "plus", pkg.Splus_q_vector)):
        assert pkg.lib().sd_model_path(m.adjacent_sector(dn).h) == 0
        for cplx in (False, True):
            psi = rand_psi(m.N, cplx, 5)
            for q in (0.0, 2 * np.pi * 5 / L):
                check_phi(fn(m, psi, q), R.spm(L, nup, psi, q, op), q)


@pytest.mark.parametrize("L", [28, 32])
def test_sampled_rows_at_full_size(pkg, L):
    import torch
    nup = L // 2
    m = pkg.XXZChain(L, nup=nup, boundary="periodic")
    dev = torch.device("cuda", m.ctx.device)
    g = torch.Generator(device=dev)
    g.manual_seed(L)
    dtype = torch.complex128 if L == 28 else torch.float64
    psi = torch.randn(m.N, dtype=dtype, device=dev, generator=g)
    rng = np.random.default_rng(L)
    for op, fn, dn in (("minus", pkg.Sminus_q_vector, -1), ("plus", pkg.Splus_q_vector, 1)):
        for q in (0.0, 2 * np.pi * 3 / L):
            phi = fn(m, psi, q)
            torch.cuda.synchronize(dev)
            dst = m.adjacent_sector(dn)
            assert phi.shape[0] == dst.N
            rows = np.unique(rng.integers(0, dst.N, 3000))
            rows = np.concatenate([rows, [0, dst.N - 1]])
            states = R.unrank(rows, L, nup + dn)

            def psi_at(j):
                return psi[torch.as_tensor(j, device=dev)].cpu().numpy()
            want = R.spm_rows(L, nup, psi_at, states, q, op)
            got = phi[torch.as_tensor(rows, device=dev)].cpu().numpy()
            check_phi(got, want, q)
            del phi


# ---- 2. the adjacent-sector model ----
def _model_cases(pkg, O):
    L = 14
    hop, zz = j1j2_lists(L)
    lr = pkg.long_range_hopping(L, lambda i, j: 0.5 / (j - i) ** 2)
    return [
        (dict(L=L, hopping=[(i, i + 1, 0.5) for i in range(1, L)], zz=[(i, i + 1, 0.7) for i in range(1, L)],
              onsite_field=np.linspace(-0.3, 0.4, L))),
        dict(L=L, hopping=hop, zz=zz, onsite_field=np.full(L, 0.2)),
        dict(L=L, hopping=lr, zz=[(i, i + 1, 1.0) for i in range(1, L)], onsite_field=None),
    ]


def test_adjacent_sector_apply_matches_oracle(pkg, O):
    for kw in _model_cases(pkg, O):
        m = pkg.build_model(kw["L"], nup=6, hopping=kw["hopping"], zz=kw["zz"], onsite_field=kw["onsite_field"])
        for dn in (-1, 1):
            a = m.adjacent_sector(dn)
            assert a is m.adjacent_sector(dn) and a.nup == 6 + dn and a.ctx is m.ctx
            ref = O.build_model(kw["L"], nup=6 + dn, hopping=kw["hopping"], zz=kw["zz"], onsite_field=kw["onsite_field"])
            psi = rand_psi(a.N, True, 11)
            out = np.empty_like(psi)
            pkg.apply_H(out, psi, a)
            assert np.array_equal(out, O.apply_H(ref, psi))
    with pytest.raises(pkg.ArgumentError):
        pkg.XXZChain(6).adjacent_sector(1)
    with pytest.raises(pkg.ArgumentError):
        pkg.XXZChain(6, nup=6).adjacent_sector(1)
    with pytest.raises(pkg.ArgumentError):
        pkg.XXZChain(6, nup=0).adjacent_sector(-1)


def _spm_call(pkg, ctx, src, dst, op, psi, out):
    return pkg.lib().sd_spm_q(ctx.h, src.h, dst.h, op, pkg._lib.SD_F64, psi.ctypes.data, len(psi), 0.3, out.ctypes.data, len(out) // 2)


def test_incompatible_models_are_refused(pkg):
    L, nup = 16, 8
    src = pkg.XXZChain(L, Jz=0.5, nup=nup)
    good = src.adjacent_sector(-1)
    psi = rand_psi(src.N, False, 2)
    want = R.spm(L, nup, psi, 0.3, "minus")
    ctx = src.ctx

    def refused(dst, op=2):
        out = np.zeros(2 * dst.N)
        assert _spm_call(pkg, ctx, src, dst, op, psi, out) == pkg._lib.SD_EARG
        assert pkg.lib().sd_last_error(ctx.h)
        out = np.zeros(2 * good.N)
        assert _spm_call(pkg, ctx, src, good, 2, psi, out) == pkg._lib.SD_OK
        check_phi(out.view(np.complex128), want, 0.3)

    refused(pkg.XXZChain(L + 1, Jz=0.5, nup=nup - 1))                              # different L
    refused(pkg.XXZChain(L, Jz=0.5 + 2 ** -40, nup=nup - 1))                      # one coupling differs
    refused(pkg.XXZChain(L, Jz=0.5, nup=nup + 1))                                  # wrong sector for S^-
    refused(good, op=1)                                                            # wrong sector for S^+
    sh = pkg.XXZChain(L, Jz=0.5, nup=nup - 1)
    sh.set_shard(0, 2)
    refused(sh)                                                                    # sharded
    other = pkg.XXZChain(L, Jz=0.5, nup=nup - 1)
    other.set_apply(lambda out, x, model: None)                                    # a caller's operator on the context
    try:
        out = np.zeros(2 * good.N)
        assert _spm_call(pkg, ctx, src, good, 2, psi, out) == pkg._lib.SD_EARG
        with pytest.raises(pkg.ArgumentError):
            pkg.kpm_sqw_transverse(psi, src, [0.3], [0.0], a=10.0, b=0.0, kpm_m=8)
    finally:
        other.set_apply(None)
    out = np.zeros(2 * good.N)
    assert _spm_call(pkg, ctx, src, good, 2, psi, out) == pkg._lib.SD_OK
    check_phi(out.view(np.complex128), want, 0.3)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.Sminus_q_vector(src, psi[:-1], 0.3)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.kpm_sqw_transverse(psi[:-1], src, [0.3], [0.0], a=10.0, b=0.0)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.lanczos_sqw_transverse(psi[:-1], src, [0.3], [0.0], component="xx")


# ---- 3. spectra against the oracle composition ----
def oracle_kpm(O, L, lists, nup, psi, qs, omega, a, b, M, op):
    src = O.build_model(L, nup=nup, **lists)
    dst = O.build_model(L, nup=nup + (-1 if op == "minus" else 1), **lists)
    psic = np.asarray(psi, dtype=np.complex128)
    E0 = np.vdot(psic, O.apply_H(src, psic)).real
    g = O.get_kernel(M, "jackson")
    S, mus = np.zeros((len(qs), len(omega))), []
    for k, q in enumerate(qs):
        phi = R.spm(L, nup, psi, q, op)
        n = np.linalg.norm(phi)
        if n == 0:
            mus.append(None)
            continue
        mu = O.compute_chebyshev_moments(dst, phi / n, M, a, b)
        mus.append(mu)
        S[k] = O.kpm_reconstruct(mu * g, omega, a, b, E0) * n * n
    return S, mus


def oracle_lanczos(O, L, lists, nup, psi, qs, omega, m, op):
    src = O.build_model(L, nup=nup, **lists)
    dst = O.build_model(L, nup=nup + (-1 if op == "minus" else 1), **lists)
    psic = np.asarray(psi, dtype=np.complex128)
    E0 = np.sum(psic * O.apply_H(src, psic)).real
    S = np.zeros((len(qs), len(omega)))
    for k, q in enumerate(qs):
        phi = R.spm(L, nup, psi, q, op)
        if np.linalg.norm(phi) == 0:
            continue
        al, be, nv = O.lanczos_tridiag(dst, phi, m)
        S[k] = O.spectral_from_tridiagonal(al, be, nv, E0, omega)
    return S


def xxz_lists(L, Jz, hz, boundary):
    hop = [(i, i + 1, 0.5) for i in range(1, L)]
    zz = [(i, i + 1, Jz) for i in range(1, L)]
    if boundary == "periodic":
        hop.append((L, 1, 0.5))
        zz.append((L, 1, Jz))
    return dict(hopping=hop, zz=zz, onsite_field=np.full(L, hz))


def close(got, want, rel):
    assert np.abs(got - want).max() <= rel * max(1.0, np.abs(want).max())


@pytest.mark.parametrize("L", [16, 18])
@pytest.mark.parametrize("boundary", ["open", "periodic"])
def test_kpm_spectra_match_oracle(pkg, O, L, boundary):
    lists = xxz_lists(L, 0.5, 0.3, boundary)
    nup = L // 2
    m = pkg.build_model(L, nup=nup, **lists)
    _, psi = pkg.groundstate(m)
    qs = pkg.momenta(m)
    omega = np.linspace(-1.0, 4.0, 41)
    a, b, M = 0.8 * L, 0.0, 1024
    ref = {op: oracle_kpm(O, L, lists, nup, psi, qs, omega, a, b, M, op) for op in ("minus", "plus")}
    want = {"+-": ref["minus"][0], "-+": ref["plus"][0], "xx": 0.25 * (ref["minus"][0] + ref["plus"][0])}
    for pair in (True, False):
        m.ctx.set_kpm_pair_q(pair)
        try:
            for comp in ("+-", "-+", "xx"):
                got = pkg.kpm_sqw_transverse(psi, m, qs, omega, component=comp, a=a, b=b, kpm_m=M)
                close(got, want[comp], 1e-8)
        finally:
            m.ctx.set_kpm_pair_q(True)
    # moments of the device recursion on the target sector, on the device's phi
    for op, fn, dn in (("minus", pkg.Sminus_q_vector, -1), ("plus", pkg.Splus_q_vector, 1)):
        k = 3
        phi = fn(m, psi, qs[k])
        mu = pkg.compute_chebyshev_moments(pkg.apply_H, phi / np.linalg.norm(phi), M, a, b, m.adjacent_sector(dn))
        assert np.abs(mu - ref[op][1][k]).max() <= 1e-12
    if L == 16:   # a complex psi0 (no pairing of q and 2 pi - q)
        psic = psi * np.exp(0.3j)
        refc = {op: oracle_kpm(O, L, lists, nup, psic, qs, omega, a, b, M, op)[0] for op in ("minus", "plus")}
        close(pkg.kpm_sqw_transverse(psic, m, qs, omega, component="xx", a=a, b=b, kpm_m=M),
              0.25 * (refc["minus"] + refc["plus"]), 1e-8)


@pytest.mark.parametrize("boundary", ["open", "periodic"])
def test_lanczos_spectra_match_oracle(pkg, O, boundary):
    L = 16
    lists = xxz_lists(L, 0.5, 0.3, boundary)
    nup = L // 2
    m = pkg.build_model(L, nup=nup, **lists)
    _, psi = pkg.groundstate(m)
    qs = pkg.momenta(m)
    omega = np.linspace(-1.0, 4.0, 41)
    # a short recursion keeps its orthogonality: agreement to reduction-order noise.  A long one without
    # re-orthogonalisation (lanc_m = 100) amplifies rounding differences chaotically once orthogonality is lost (ghost Ritz
    # values, as for S^zz in test_gpu_recursions.py): only the broadened spectrum is comparable, to ~1e-3.
    for lm, rel in ((12, 1e-8), (100, 2e-3)):
        ref = {op: oracle_lanczos(O, L, lists, nup, psi, qs, omega, lm, op) for op in ("minus", "plus")}
        close(pkg.lanczos_sqw_transverse(psi, m, qs, omega, component="+-", lanc_m=lm), ref["minus"], rel)
        close(pkg.lanczos_sqw_transverse(psi, m, qs, omega, component="-+", lanc_m=lm), ref["plus"], rel)
        close(pkg.lanczos_sqw_transverse(psi, m, qs, omega, component="xx", lanc_m=lm),
              0.25 * (ref["minus"] + ref["plus"]), rel)


# ---- 4. SU(2): <S^a_{-q} f(H) S^b_q> = delta_ab g for a singlet and an SU(2)-invariant H ----
def dimer_singlet(L):
    """prod_k (|up down> - |down up>)/sqrt 2 on sites (2k+1, 2k+2): 2^(L/2) nonzero rows, placed with the numpy rank."""
    h = L // 2
    b = np.arange(1 << h, dtype=np.int64)
    s = np.zeros(len(b), dtype=np.int64)
    sign = np.ones(len(b))
    for k in range(h):
        first_up = (b >> k) & 1
        s |= np.where(first_up == 1, np.int64(1) << (2 * k), np.int64(1) << (2 * k + 1))
        sign *= np.where(first_up == 1, 1.0, -1.0)
    psi = np.zeros(math.comb(L, h))
    psi[R.rank(s, L, h)] = sign * 2.0 ** (-h / 2)
    return psi


@pytest.mark.parametrize("L", [28, 32])
def test_su2_identity_at_full_size(pkg, L):
    m = pkg.XXZChain(L, Jxy=1.0, Jz=1.0, nup=L // 2, boundary="periodic")
    psi = dimer_singlet(L)
    qs = np.array([np.pi, 2 * np.pi * 3 / L])
    omega = np.linspace(-2.0, 4.0, 31)
    a, b = 1.01 * L / 2, -L / 4            # the spectrum of every sector lies in [-3L/4, L/4]
    szz = pkg.kpm_sqw(psi, m, qs, omega, a=a, b=b, kpm_m=64)
    spm = pkg.kpm_sqw_transverse(psi, m, qs, omega, component="+-", a=a, b=b, kpm_m=64)
    smp = pkg.kpm_sqw_transverse(psi, m, qs, omega, component="-+", a=a, b=b, kpm_m=64)
    scale = np.abs(szz).max()
    assert scale > 0
    assert np.abs(spm - 2 * szz).max() <= 2e-9 * scale
    assert np.abs(smp - 2 * szz).max() <= 2e-9 * scale
    assert np.abs(0.25 * (spm + smp) - szz).max() <= 1e-9 * scale


def test_su2_moments(pkg):
    L = 20
    m = pkg.XXZChain(L, nup=L // 2, boundary="periodic")
    psi = dimer_singlet(L)
    a, b = 1.01 * L / 2, -L / 4
    for q in (np.pi, 2 * np.pi * 3 / L):
        pz = pkg.Sz_q_vector(m, psi, q)
        mz = pkg.compute_chebyshev_moments(pkg.apply_H, pz / np.linalg.norm(pz), 64, a, b, m) * np.vdot(pz, pz).real
        for fn, dn in ((pkg.Sminus_q_vector, -1), (pkg.Splus_q_vector, 1)):
            p = fn(m, psi, q)
            mt = pkg.compute_chebyshev_moments(pkg.apply_H, p / np.linalg.norm(p), 64, a, b, m.adjacent_sector(dn)) * np.vdot(p, p).real
            assert np.abs(mt - 2 * mz).max() <= 1e-10 * abs(2 * mz[0])


# ---- 5. a uniform field shifts the target sector's H by hz (n - L/2) ----
def test_field_shift(pkg):
    L, nup, hz = 20, 10, 0.4
    m0 = pkg.XXZChain(L, Jz=0.7, nup=nup)
    m1 = pkg.XXZChain(L, Jz=0.7, hz=hz, nup=nup)
    psi = rand_psi(m0.N, False, 9)
    a, b = 12.0, 0.5
    phi = pkg.Sminus_q_vector(m0, psi, 2 * np.pi * 4 / L)
    phi /= np.linalg.norm(phi)
    mu0 = pkg.compute_chebyshev_moments(pkg.apply_H, phi, 128, a, b, m0.adjacent_sector(-1))
    mu1 = pkg.compute_chebyshev_moments(pkg.apply_H, phi, 128, a, b + hz * (nup - 1 - L / 2), m1.adjacent_sector(-1))
    assert np.abs(mu1 - mu0).max() <= 1e-12


# ---- 6. edges ----
def test_edges(pkg):
    L = 10
    omega = np.linspace(0, 3, 7)
    m0 = pkg.XXZChain(L, nup=0)
    mL = pkg.XXZChain(L, nup=L)
    qs = pkg.momenta(m0)
    assert not pkg.kpm_sqw_transverse(np.ones(1), m0, qs, omega, component="+-", a=8.0, b=0.0).any()
    assert not pkg.lanczos_sqw_transverse(np.ones(1), mL, qs, omega, component="-+").any()
    # S^{xx} at nup = 0 is a quarter of S^{-+}
    s = pkg.kpm_sqw_transverse(np.ones(1), m0, qs, omega, component="xx", a=8.0, b=0.0)
    assert np.array_equal(s, 0.25 * (0.0 + pkg.kpm_sqw_transverse(np.ones(1), m0, qs, omega, component="-+", a=8.0, b=0.0)))
    with pytest.raises(pkg.DimensionMismatch):
        pkg.Splus_q_vector(m0, np.ones(2), 0.0)
    with pytest.raises(pkg.ArgumentError):
        pkg.dynamical_structure_factor(m0, np.ones(1), qs, omega, component="yy")


def test_zz_component_is_todays_call(pkg):
    L = 12
    m = pkg.XXZChain(L, Jz=0.5, hz=0.1, nup=6, boundary="periodic")
    _, psi = pkg.groundstate(m)
    qs, omega = pkg.momenta(m), np.linspace(-1, 3, 21)
    assert np.array_equal(pkg.dynamical_structure_factor(m, psi, qs, omega, method="kpm", component="zz", a=6.0, b=0.0),
                          pkg.kpm_sqw(psi, m, qs, omega, a=6.0, b=0.0))
    assert np.array_equal(pkg.dynamical_structure_factor(m, psi, qs, omega, component="zz"), pkg.lanczos_sqw(psi, m, qs, omega))
    assert np.array_equal(pkg.dynamical_structure_factor(m, psi, qs, omega, method="kpm", component="xx", a=6.0, b=0.0),
                          pkg.kpm_sqw_transverse(psi, m, qs, omega, component="xx", a=6.0, b=0.0))
    # without a, b each target sector's bounds are estimated (seeded): the same call twice gives the same rows
    s1 = pkg.kpm_sqw_transverse(psi, m, qs, omega, component="+-", kpm_m=64, seed=3)
    s2 = pkg.kpm_sqw_transverse(psi, m, qs, omega, component="+-", kpm_m=64, seed=3)
    assert np.array_equal(s1, s2) and np.isfinite(s1).all()
