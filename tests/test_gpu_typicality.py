"""Finite temperature by typicality on the GPU: the spin-current kernel against the row loop of tests/typicality_ref.py (bit for
bit), the bracket against its worst-case summation bound, the thermal state and the per-sample correlation functions against
dense propagators -- the library gets twice the error of the numpy restatement of the same truncated series plus the
project's Chebyshev bar of 1e-12, for both evolution methods (the Krylov thermal state also against the restatement's Krylov at
1e-11, the existing Krylov bar) --, batching, a full-size run and the refusals."""
import ctypes as C

import numpy as np
import pytest

import typicality_ref as R

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)


def chain(L, boundary="open", Jxy=1.0, Jz=1.0, hz=0.0):
    hop = [(i, i + 1, Jxy / 2) for i in range(1, L)]
    zz = [(i, i + 1, Jz) for i in range(1, L)]
    if boundary == "periodic":
        hop.append((L, 1, Jxy / 2))
        zz.append((L, 1, Jz))
    return hop, zz, np.full(L, hz)


def j1j2(L, J1=1.0, J2=0.4):
    hop = [(i, i % L + 1, J1 / 2) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2 / 2) for i in range(1, L + 1)]
    zz = [(i, i % L + 1, J1) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2) for i in range(1, L + 1)]
    return hop, zz, np.full(L, 0.1)


def long_range(L):
    hop = [(i, j, 0.5 / (j - i) ** 2) for i in range(1, L + 1) for j in range(i + 1, L + 1)]
    zz = [(i, i + 1, 0.6) for i in range(1, L)]
    return hop, zz, np.zeros(L)


LISTS = {"open": lambda L: chain(L, "open", Jz=0.7), "periodic": lambda L: chain(L, "periodic", Jz=0.7),
         "field": lambda L: chain(L, "open", Jxy=0.8, Jz=0.7, hz=0.3), "j1j2": j1j2, "long_range": long_range}


def rand_vec(N, cplx, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(N)
    if cplx:
        x = x + 1j * rng.standard_normal(N)
    return x / np.linalg.norm(x)


def build(pkg, name, L, nup):
    hop, zz, field = LISTS[name](L)
    m = pkg.build_model(L, nup=nup, hopping=hop, zz=zz, onsite_field=field)
    states, index = R.basis(L, nup)
    assert np.array_equal(m.states_range(0, m.N), states)
    return m, hop, zz, field, states, index


def weight_sets(nh, seed):
    return [None, np.eye(nh)[nh // 2], np.random.default_rng(seed).standard_normal(nh)]


def bits(x):
    return np.ascontiguousarray(x).view(np.float64)


# ---- 1. the current kernel: write form ----
CURRENT_CASES = [("open", 8, 4), ("periodic", 12, 6), ("periodic", 16, 8), ("field", 14, 3), ("periodic", 16, 1), ("periodic", 13, 12),
                 ("j1j2", 12, 5), ("long_range", 10, 5), ("long_range", 12, 2), ("periodic", 10, None), ("j1j2", 14, None),
                 ("open", 9, 0), ("open", 9, 9), ("periodic", 3, 1)]


@pytest.mark.parametrize("name,L,nup", CURRENT_CASES)
def test_spin_current_equals_the_row_loop(pkg, name, L, nup):
    import torch
    m, hop, zz, field, states, index = build(pkg, name, L, nup)
    plan = R.CurrentPlan(L, nup, hop, states, index)
    dev = torch.device("cuda", m.ctx.device)
    for cplx in (False, True):
        psi = rand_vec(m.N, cplx, 7 + L)
        for w in weight_sets(len(hop), L):
            want = plan.apply(psi, w)
            got = pkg.spin_current(psi, m, w)
            assert got.dtype == np.complex128 and got.shape == (m.N,)
            assert np.array_equal(got, want), (name, L, nup, cplx, np.abs(got - want).max())
            got_dev = pkg.spin_current(torch.as_tensor(psi, device=dev), m, w)
            assert np.array_equal(got_dev.cpu().numpy(), want)
    print(f"{name} L={L} nup={nup} N={m.N} path={pkg.lib().sd_model_path(m.h)}: equal to the row loop")


def test_spin_current_per_row_plan(pkg):
    m = pkg.XXZChain(24, nup=2, boundary="periodic").adjacent_sector(-1)
    assert pkg.lib().sd_model_path(m.h) == 0
    states, index = R.basis(24, 1)
    plan = R.CurrentPlan(24, 1, m.hopping_list, states, index)
    psi = rand_vec(m.N, True, 3)
    assert np.array_equal(pkg.spin_current(psi, m), plan.apply(psi))


# ---- 2. the current kernel: bracket form ----
@pytest.mark.parametrize("name,L,nup", [("periodic", 12, 6), ("periodic", 16, 8), ("field", 14, 3), ("j1j2", 12, 5), ("long_range", 10, 5),
                                        ("j1j2", 14, None), ("periodic", 16, 1)])
def test_current_expectation_within_the_summation_bound(pkg, name, L, nup):
    import torch
    m, hop, zz, field, states, index = build(pkg, name, L, nup)
    plan = R.CurrentPlan(L, nup, hop, states, index)
    dev = torch.device("cuda", m.ctx.device)
    for cplx in (False, True):
        bra, ket = 3.0 * rand_vec(m.N, cplx, 1 + L), 0.5 * rand_vec(m.N, True, 2 + L)
        for w in weight_sets(len(hop), L):
            wt = np.abs(np.array([t for _, _, t in hop]) * (1.0 if w is None else w)).sum()
            bar = 2 * m.N * 2.0 ** -53 * np.linalg.norm(bra) * np.linalg.norm(ket) * wt      # worst-case summation bound
            want = np.vdot(bra, plan.apply(ket, w))
            got = pkg.current_expectation(bra, ket, m, w)
            print(f"{name} L={L} nup={nup} bra={'c128' if cplx else 'f64'}: {abs(got - want):.2e} (bar {bar:.2e})")
            assert abs(got - want) <= bar
            again = pkg.current_expectation(bra, ket, m, w)
            assert got.real.hex() == again.real.hex() and got.imag.hex() == again.imag.hex()      # same call twice: equal bits
            on_dev = pkg.current_expectation(torch.as_tensor(bra, device=dev), torch.as_tensor(ket, device=dev), m, w)
            assert on_dev.real.hex() == got.real.hex() and on_dev.imag.hex() == got.imag.hex()


# ---- 3. the thermal state ----
def dense_thermal(Hd, r, beta):
    w, U = np.linalg.eigh(Hd)
    v = U @ (np.exp(-0.5 * beta * (w - w[0])) * (U.conj().T @ r))
    n = np.linalg.norm(v)
    return v / n, np.log(n) - 0.5 * beta * w[0], w


@pytest.mark.parametrize("name,L,nup", [("periodic", 10, 5), ("field", 12, 6), ("j1j2", 10, 4)])
@pytest.mark.parametrize("beta", [0.5, 2.0, 10.0])
def test_thermal_state_against_dense(pkg, name, L, nup, beta):
    import torch
    m, hop, zz, field, states, index = build(pkg, name, L, nup)
    H = R.hamiltonian(L, nup, hop, zz, field, states, index)
    r = 2.0 * rand_vec(m.N, True, 11)
    want, ln_want, w = dense_thermal(H.toarray(), r, beta)
    Eb = (w[0] - 0.05, w[-1] + 0.05)
    ref, ln_ref = R.imag_chebyshev(H, r, beta / 2, Eb)
    err_ref, eln_ref = np.abs(ref - want).max(), abs(ln_ref - ln_want)
    got, ln = pkg.thermal_state(m, beta, r=r, Ebounds=Eb)
    err, eln = np.abs(got - want).max(), abs(ln - ln_want)
    print(f"{name} L={L} beta={beta}: state {err:.2e} (reference {err_ref:.2e}), log_norm {eln:.2e} (reference {eln_ref:.2e})")
    assert err <= 2 * err_ref + 1e-12
    assert eln <= 2 * eln_ref + 1e-12
    got_dev, ln_dev = pkg.thermal_state(m, beta, r=torch.as_tensor(r, device=torch.device("cuda", m.ctx.device)), Ebounds=Eb)
    assert np.array_equal(got_dev.cpu().numpy(), got) and ln_dev == ln
    # the Krylov method against the reference's Krylov
    kref, kln_ref = R.imag_krylov(H, r, beta / 2, 30)
    kgot, kln = pkg.thermal_state(m, beta, r=r, method="krylov", kry_m=30)
    print(f"   krylov vs reference krylov: state {np.abs(kgot - kref).max():.2e}, log_norm {abs(kln - kln_ref):.2e}")
    assert np.abs(kgot - kref).max() <= 1e-11
    assert abs(kln - kln_ref) <= 1e-11


def test_thermal_state_substeps_when_z_exceeds_600(pkg):
    L, nup, beta = 10, 5, 10.0
    m, hop, zz, field, states, index = build(pkg, "periodic", L, nup)
    H = R.hamiltonian(L, nup, hop, zz, field, states, index)
    r = rand_vec(m.N, True, 12)
    want, ln_want, w = dense_thermal(H.toarray(), r, beta)
    Eb = (w[0] - 0.05, w[-1] + 300.0)                       # the upper bound widened: z = a beta / 2 > 600
    assert R.rescaling(*Eb)[0] * beta / 2 > 600
    ref, ln_ref = R.imag_chebyshev(H, r, beta / 2, Eb)
    got, ln = pkg.thermal_state(m, beta, r=r, Ebounds=Eb)
    err, err_ref = np.abs(got - want).max(), np.abs(ref - want).max()
    eln, eln_ref = abs(ln - ln_want), abs(ln_ref - ln_want)
    print(f"sub-stepped: state {err:.2e} (reference {err_ref:.2e}), log_norm {eln:.2e} (reference {eln_ref:.2e})")
    assert err <= 2 * err_ref + 1e-12
    assert eln <= 2 * eln_ref + 1e-12


def test_thermal_state_from_the_seed_stream_and_estimated_bounds(pkg):
    L, nup, beta = 12, 6, 2.0
    m, hop, zz, field, states, index = build(pkg, "periodic", L, nup)
    H = R.hamiltonian(L, nup, hop, zz, field, states, index)
    r = np.empty(m.N, dtype=np.complex128)
    assert pkg.lib().sd_fill_randn_host(r.ctypes.data_as(_dp), 2 * m.N, 5, 0) == 0
    r /= np.linalg.norm(r)
    want, ln_want, w = dense_thermal(H.toarray(), r, beta)
    ref, ln_ref = R.imag_chebyshev(H, r, beta / 2, (w[0] - 0.05, w[-1] + 0.05))
    got, ln = pkg.thermal_state(m, beta, seed=5)            # bounds estimated by the library
    err, eln = np.abs(got - want).max(), abs(ln - ln_want)
    print(f"seed stream: state {err:.2e}, log_norm {eln:.2e}")
    assert err <= 2 * np.abs(ref - want).max() + 1e-12
    assert eln <= 2 * abs(ln_ref - ln_want) + 1e-12


# ---- 4. the correlation function, per sample ----
def op_norm(op, L, hop):
    if op[0] == "current":
        return np.abs(np.array([t for _, _, t in hop]) * (1.0 if op[1] is None else op[1])).sum()
    return 0.5 * np.sqrt(L) if op[0] == "Szq" else 0.5


def ref_op(op, L, states, plan):
    return R.Operator("Sz_all", None, L, states) if op == "Sz_all" else R.Operator(op[0], op[1], L, states, plan)


def check_sample(pkg, m, H, Hd, hop, states, plan, A, B, beta, r, times, method, Eb, seed=None):
    L = m.L
    Ao, Bo = ref_op(A, L, states, plan), ref_op(B, L, states, plan)
    An = 0.5 if A == "Sz_all" else op_norm(A, L, hop)
    scale = An * op_norm(B, L, hop)
    num_d, ln_d, en_d = R.dqt_dense(Hd, Ao, Bo, beta, r, times)
    num_r, ln_r, en_r = R.dqt_sample(H, Ao, Bo, beta, r, times, method=method, Ebounds=Eb, kry_m=30)
    kw = dict(method=method, kry_m=30)
    if method == "chebyshev":
        kw["Ebounds"] = Eb
    got = pkg.typicality_correlation_function(m, beta, A, B, times, r=None if seed is not None else r,
                                              seed=0 if seed is None else seed, **kw)
    num = got.num[0]
    if A != "Sz_all":
        num = num.reshape(-1, 1)
        assert got.shape == (len(times),)
    else:
        assert got.shape == (len(times), L)
    assert got.den[0] == 1.0 and np.array_equal(np.asarray(got), got.num[0])         # one sample: the ratio is the sample's num
    hs = np.abs(np.linalg.eigvalsh(Hd)[[0, -1]]).max()
    base = 1e-12
    e_num, r_num = np.abs(num - num_d).max(), np.abs(num_r - num_d).max()
    e_den, r_den = abs(np.expm1(2 * (got.log_norm[0] - ln_d))), abs(np.expm1(2 * (ln_r - ln_d)))
    e_en, r_en = abs(got.energy[0] - en_d), abs(en_r - en_d)
    print(f"L={L} A={A} B={B} beta={beta} {method}: num {e_num:.2e} (ref {r_num:.2e}), den {e_den:.2e} (ref {r_den:.2e}), "
          f"energy {e_en:.2e} (ref {r_en:.2e})")
    assert e_num <= 2 * r_num + base * scale
    assert e_den <= 2 * r_den + base
    assert e_en <= 2 * r_en + base * hs
    return got


PAIRS = [(("Sz", 3), ("Sz", 1)), ("Sz_all", ("Sz", 2)), (("Szq", 2 * np.pi * 2 / 10), ("Szq", 2 * np.pi * 2 / 10)), (("current", None), ("current", None))]


def sample_case(pkg, name, L, nup):
    m, hop, zz, field, states, index = build(pkg, name, L, nup)
    H = R.hamiltonian(L, nup, hop, zz, field, states, index)
    Hd = H.toarray()
    w = np.linalg.eigvalsh(Hd)
    return m, H, Hd, hop, states, R.CurrentPlan(L, nup, hop, states, index), (w[0] - 0.05, w[-1] + 0.05)


@pytest.mark.parametrize("beta", [0.0, 0.5, 4.0])
@pytest.mark.parametrize("method", ["chebyshev", "krylov"])
def test_correlations_per_sample_against_dense(pkg, beta, method):
    L, nup = 10, 5
    m, H, Hd, hop, states, plan, Eb = sample_case(pkg, "periodic", L, nup)
    r = rand_vec(m.N, True, 21)
    uniform = [0.0, 0.4, 0.8, 1.2, 1.6]
    for A, B in PAIRS:
        check_sample(pkg, m, H, Hd, hop, states, plan, A, B, beta, r, uniform, method, Eb)
    check_sample(pkg, m, H, Hd, hop, states, plan, ("Sz", 3), ("Sz", 1), beta, r, [0.3, 0.3, 0.5, 1.7, 2.0], method, Eb)   # non-uniform, t_0 > 0, a repeated time


def test_correlations_other_models_and_weights(pkg):
    m, H, Hd, hop, states, plan, Eb = sample_case(pkg, "j1j2", 10, 4)
    r = rand_vec(m.N, True, 22)
    w = np.random.default_rng(1).standard_normal(len(hop))
    u = np.eye(len(hop))[3]
    check_sample(pkg, m, H, Hd, hop, states, plan, ("current", u), ("current", w), 1.0, r, [0.0, 0.5, 1.0], "chebyshev", Eb)
    check_sample(pkg, m, H, Hd, hop, states, plan, "Sz_all", ("current", None), 1.0, r, [0.0, 0.5, 1.0], "chebyshev", Eb)
    m, H, Hd, hop, states, plan, Eb = sample_case(pkg, "field", 8, None)             # full basis
    r = rand_vec(m.N, True, 23)
    check_sample(pkg, m, H, Hd, hop, states, plan, ("current", None), ("current", None), 0.7, r, [0.0, 0.6], "chebyshev", Eb)
    check_sample(pkg, m, H, Hd, hop, states, plan, "Sz_all", ("Sz", 4), 0.7, r, [0.0, 0.6], "krylov", Eb)


def test_correlations_from_the_seed_stream(pkg):
    """r = None: the library draws the counter-based normal stream of `seed`; sd_fill_randn_host feeds the reference"""
    L, nup = 10, 5
    m, H, Hd, hop, states, plan, Eb = sample_case(pkg, "periodic", L, nup)
    r = np.empty(m.N, dtype=np.complex128)
    assert pkg.lib().sd_fill_randn_host(r.ctypes.data_as(_dp), 2 * m.N, 9, 0) == 0
    for A, B in PAIRS:
        check_sample(pkg, m, H, Hd, hop, states, plan, A, B, 1.0, r, [0.0, 0.5, 1.0, 1.5], "chebyshev", Eb, seed=9)
    # several samples: sample k uses seed + k; the estimate is sum num / sum den
    got = pkg.typicality_correlation_function(m, 1.0, ("Sz", 3), ("Sz", 1), [0.0, 0.5], n_samples=3, seed=9, Ebounds=Eb)
    one = [pkg.dqt_sample(m, 1.0, ("Sz", 3), ("Sz", 1), [0.0, 0.5], seed=9 + k, Ebounds=Eb) for k in range(3)]
    den = np.exp(2 * np.array([s["log_norm"] for s in one]))
    want = sum(d * s["num"] for d, s in zip(den, one)) / den.sum()
    assert np.abs(np.asarray(got) - want).max() <= 1e-15
    assert got.num.shape == (3, 2) and got.den.shape == (3,) and got.energy.shape == (3,) and got.stderr.shape == (2,)
    assert np.all(got.stderr.real > 0)


def test_batched_equals_unbatched_bit_for_bit(pkg):
    L, nup = 14, 7
    m = pkg.XXZChain(L, Jz=0.7, nup=nup, boundary="periodic")
    assert pkg.lib().sd_model_path(m.h) == 1               # a tiled plan: the two states do share their launches by default
    r = rand_vec(m.N, True, 31)
    times = [0.0, 0.5, 1.0, 1.7]
    for A, B in [("Sz_all", ("Sz", 2)), (("current", None), ("current", None))]:
        n0 = m.ctx.apply_count()
        a = pkg.dqt_sample(m, 1.0, A, B, times, r=r, Ebounds=(-8.0, 5.0))
        n1 = m.ctx.apply_count()
        m.ctx.set_q_batch(False)
        try:
            b = pkg.dqt_sample(m, 1.0, A, B, times, r=r, Ebounds=(-8.0, 5.0))
        finally:
            m.ctx.set_q_batch(True)
        assert m.ctx.apply_count() - n1 == n1 - n0           # the same operator applications either way
        assert np.array_equal(bits(a["num"]), bits(b["num"]))
        assert a["log_norm"] == b["log_norm"] and a["energy"] == b["energy"]


def test_full_size_sum_rule_and_current_conservation(pkg):
    """L = 20, nup = 10, periodic chain at Jz = 0, against the restatement on a sparse H (no dense matrix).  [J, H] = 0 there, so
    C_JJ(t) is constant; sum_i <S^z_i(t) S^z_j> = (nup - L/2) <S^z_j> = 0.  Bars: ten times the residuals of the restatement itself
    in this very case (measured on the CPU, DESIGN.md 14: drift 2.9e-15 of |C_JJ|, sum rule 3.7e-17; two other seeds gave 2.3e-15 /
    8.4e-17 and 2.9e-15 / 4.4e-17), for the longer sums."""
    L, nup, beta = 20, 10, 1.0
    hop, zz, field = chain(L, "periodic", Jz=0.0)
    m = pkg.build_model(L, nup=nup, hopping=hop, zz=zz, onsite_field=field)
    states, index = R.basis(L, nup)
    H = R.hamiltonian(L, nup, hop, zz, field, states, index)
    plan = R.CurrentPlan(L, nup, hop, states, index)
    Eb = (-0.5 * L * 2 / np.pi - 0.5, 0.5 * L * 2 / np.pi + 0.5)       # the free-fermion band: |E| <= (L / pi) Jxy
    r = rand_vec(m.N, True, 41)
    times = [0.0, 0.5, 1.0, 1.5, 2.0]
    Jop = R.Operator("current", None, L, states, plan)
    ref_jj, _, _ = R.dqt_sample(H, Jop, Jop, beta, r, times, Ebounds=Eb)
    jj = pkg.dqt_sample(m, beta, ("current", None), ("current", None), times, r=r, Ebounds=Eb)
    drift = np.abs(jj["num"] - jj["num"][0]).max() / abs(jj["num"][0])
    dev_jj = np.abs(jj['num'] - ref_jj[:, 0]).max()
    print(f"L=20: C_JJ = {jj['num'][0].real:.6f}, drift {drift:.2e} (reference {np.abs(ref_jj - ref_jj[0]).max() / abs(ref_jj[0, 0]):.2e}), "
          f"vs reference {dev_jj:.2e}")
    assert drift <= 10 * 2.9e-15
    assert dev_jj <= 1e-12 * op_norm(("current", None), L, hop) ** 2          # 1e-12 |A| |B|, the base term of check_sample
    ref_zz, _, _ = R.dqt_sample(H, R.Operator("Sz_all", None, L, states), R.Operator("Sz", 2, L, states), beta, r, times, Ebounds=Eb)
    zzc = pkg.dqt_sample(m, beta, "Sz_all", ("Sz", 2), times, r=r, Ebounds=Eb)
    res = np.abs(zzc["num"].sum(axis=1)).max()
    dev_zz = np.abs(zzc['num'] - ref_zz).max()
    print(f"L=20: sum rule residual {res:.2e} (reference {np.abs(ref_zz.sum(axis=1)).max():.2e}), vs reference {dev_zz:.2e}")
    assert res <= 10 * 3.7e-17
    assert dev_zz <= 1e-12 * 0.5 * op_norm(("Sz", 2), L, hop)                  # |S^z_i| = |S^z_j| = 1/2


def test_all_sectors_against_the_full_space_trace(pkg):
    """all_sectors=True at L = 8 against sum_s N_s <r_s| e^{-beta H/2} A(t) B e^{-beta H/2} |r_s> / sum_s N_s <r_s|e^{-beta H}|r_s> from
    dense propagators with the same per-sector start vectors"""
    L, beta = 8, 1.0
    hop, zz, field = chain(L, "periodic", Jz=0.7, hz=0.2)
    m = pkg.build_model(L, nup=4, hopping=hop, zz=zz, onsite_field=field)
    times = [0.0, 0.5, 1.0]
    rs, num, den = [], 0.0, 0.0
    for s in range(L + 1):
        states, index = R.basis(L, s)
        Hd = R.hamiltonian(L, s, hop, zz, field, states, index).toarray()
        r = rand_vec(len(states), True, 50 + s)
        rs.append(r)
        A, B = R.Operator("Sz", 3, L, states), R.Operator("Sz", 1, L, states)
        nm, ln, _ = R.dqt_dense(Hd, A, B, beta, r, times)
        num = num + len(states) * np.exp(2 * ln) * nm[:, 0]
        den = den + len(states) * np.exp(2 * ln)
    got = pkg.typicality_correlation_function(m, beta, ("Sz", 3), ("Sz", 1), times, r=rs, all_sectors=True)
    err = np.abs(np.asarray(got) - num / den).max()
    print(f"all sectors: {err:.2e}")
    assert err <= 1e-12 * 0.25


def test_thermal_energy_against_dense(pkg):
    """E(beta) and ln Z_r(beta) from successive imaginary-time steps of the seeded samples against the dense spectrum"""
    L, nup = 10, 5
    m, H, Hd, hop, states, plan, Eb = sample_case(pkg, "periodic", L, nup)
    betas = [0.0, 0.5, 1.0, 3.0]
    E, lnZ = pkg.thermal_energy(m, betas, n_samples=2, seed=4, Ebounds=Eb)
    w, U = np.linalg.eigh(Hd)
    num, den, want_lnZ = np.zeros(len(betas)), np.zeros(len(betas)), np.zeros((2, len(betas)))
    for k in range(2):
        r = np.empty(m.N, dtype=np.complex128)
        assert pkg.lib().sd_fill_randn_host(r.ctypes.data_as(_dp), 2 * m.N, 4 + k, 0) == 0
        c2 = np.abs(U.T @ (r / np.linalg.norm(r))) ** 2
        for i, b in enumerate(betas):
            z = np.sum(c2 * np.exp(-b * w))
            num[i] += np.sum(c2 * w * np.exp(-b * w)); den[i] += z; want_lnZ[k, i] = np.log(z)
    print(f"thermal energy: {np.abs(E - num / den).max():.2e}, ln Z_r: {np.abs(lnZ - want_lnZ).max():.2e}")
    assert np.abs(E - num / den).max() <= 1e-12 * np.abs(w).max()
    assert np.abs(lnZ - want_lnZ).max() <= 1e-12 * len(betas)


# ---- 5. refusals ----
def test_errors_leave_the_context_usable(pkg):
    L = 12
    m = pkg.XXZChain(L, nup=6, boundary="periodic")
    psi = rand_vec(m.N, True, 1)
    t = [0.0, 0.5]
    sh = pkg.XXZChain(L, nup=6, boundary="periodic")
    sh.set_shard(0, 2)
    for f in (lambda: pkg.spin_current(psi, sh), lambda: pkg.current_expectation(psi, psi, sh),
              lambda: pkg.thermal_state(sh, 1.0, r=psi), lambda: pkg.typicality_correlation_function(sh, 1.0, ("Sz", 1), ("Sz", 1), t)):
        with pytest.raises((pkg.ArgumentError, pkg.DimensionMismatch)):
            f()
    bad = [lambda: pkg.typicality_correlation_function(m, 1.0, ("Sz", 0), ("Sz", 1), t),
           lambda: pkg.typicality_correlation_function(m, 1.0, ("Sz", 1), ("Sz", L + 1), t),
           lambda: pkg.typicality_correlation_function(m, 1.0, ("Szq", [0.1, 0.2]), ("Sz", 1), t),
           lambda: pkg.typicality_correlation_function(m, 1.0, ("Szq", float("nan")), ("Sz", 1), t),
           lambda: pkg.typicality_correlation_function(m, 1.0, ("current", np.ones(3)), ("Sz", 1), t),
           lambda: pkg.typicality_correlation_function(m, 1.0, ("Sz", 1), ("Sz", 1), [0.5, 0.2]),
           lambda: pkg.typicality_correlation_function(m, 1.0, ("Sz", 1), ("Sz", 1), [-0.1, 0.2]),
           lambda: pkg.typicality_correlation_function(m, -1.0, ("Sz", 1), ("Sz", 1), t),
           lambda: pkg.typicality_correlation_function(m, 1.0, ("Sz", 1), ("Sz", 1), t, method="rk4"),
           lambda: pkg.typicality_correlation_function(m, 1.0, ("Sz", 1), "Sz_all", t),
           lambda: pkg.thermal_state(m, -0.5, r=psi),
           lambda: pkg.thermal_state(m, 1.0, r=psi, Ebounds=(-float("inf"), 5.0)),
           lambda: pkg.typicality_correlation_function(m, 1.0, ("Sz", 1), ("Sz", 1), t, Ebounds=(-8.0, float("inf"))),
           lambda: pkg.typicality_correlation_function(m, 0.0, ("Sz", 1), ("Sz", 1), [0.0, 1e9], Ebounds=(-8.0, 5.0)),
           lambda: pkg.spin_current(psi, m, np.ones(5))]
    for f in bad:
        with pytest.raises(pkg.ArgumentError):
            f()
    with pytest.raises(pkg.DimensionMismatch):
        pkg.spin_current(psi[:-1], m)
    # status codes at the C ABI: a decreasing time list and a negative beta
    num, den, en, ln = np.empty(4), C.c_double(), C.c_double(), C.c_double()
    tt = np.array([0.5, 0.2])
    args = lambda beta: (m.ctx.h, m.h, beta, None, 0, 0, 1.0, None, 0, 1.0, None, tt.ctypes.data_as(_dp), 2, 0, 0, 30, 0.0, 0.0,
                         num.ctypes.data_as(_dp), C.byref(den), C.byref(en), C.byref(ln))
    assert pkg.lib().sd_dqt_correlations(*args(1.0)) == 1
    tt[:] = [0.2, 0.5]
    assert pkg.lib().sd_dqt_correlations(*args(-1.0)) == 1
    # the context runs a normal apply correctly afterwards
    states, index = R.basis(L, 6)
    hop, zz, field = chain(L, "periodic")
    H = R.hamiltonian(L, 6, hop, zz, field, states, index)
    out = np.empty_like(psi)
    pkg.apply_H(out, psi, m)
    assert np.abs(out - H @ psi).max() <= 1e-14
