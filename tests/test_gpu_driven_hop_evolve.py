"""sd_driven_hop_evolve (stage_evolve, driven_time_evolve with hopping drives in the list) on the GPU.

(a) KH >= 1 with every hopping coefficient exactly zero, and KH = 0, give the bits of sd_driven_evolve_dev.
(b) The order problem of tests/test_hopdrive_ref_host.py (L = 8, the Peierls phase of A(t) = 0.9 sin^2(pi t / 2) from the ground state)
    at n = 10, 20, 40 steps of order 4 with kry_m = 20: both error ratios against the dense 1600-step reference >= 12, and each result
    within the tolerance of the dense product of the same stages.
(c) A constant exchange drive delta = 0.5 against a model built with Jxy * 1.5.
(d) Gauge equivalence: the Peierls run against the existing gradient_drive run with f = -dA/dt, L = 10, nup = 5, site magnetisations at
    t = T.  n = 120 steps: in dense arithmetic on the CPU the two gauges then agree to 4.2e-10 (<= 1e-9; 2.1e-9 at n = 80, 6.7e-9 at
    n = 60); the GPU runs must agree to 10 times the CPU bound, 1e-8.  Measured on an MI355X: 4.21e-10 (0.56 with the other sign; the
    pulse moves the magnetisations by 0.28).
(e) The full basis at L = 7 and the per-row plan L = 14, nup = 1 against dense.
(f) Norm 1 after every stage.   (g) A torch device vector gives the bits of the numpy vector.
(h) A Float64 psi0 with a complex-form list equals the same psi0 passed as ComplexF64, bit for bit.

Tolerance of (b), (c), (e): the scheme of tests/test_gpu_driven_evolve.py.  The floor is the 2-norm deviation of the existing
krylov_time_evolve, on the same model with the same stage durations, kry_m and number of calls, from the dense propagator of H0,
measured by the test itself in the same run.  The drive amplitudes keep sum_b |sum_k c_k z_{k,b}| <= sum_b |t_b| at every stage (the
hopping drives merged bond by bond: amplitude_ok), so the bound of the operator's norm at most doubles; the driven result may deviate
from its own dense product by 16 floors: the project's factor 8, times 2 for the doubled norm bound.  In (b) psi0 is an eigenstate of
H0, from which the parent's recursion stops at its first beta: the floor is taken from a seeded random state there.  Every test prints
floor -> deviation.  Measured on an MI355X (floor -> driven deviation):
    (b) n = 10: 2.46e-14 -> 8.11e-15;  n = 20: 4.71e-14 -> 1.27e-14;  n = 40: 9.66e-14 -> 1.82e-14  (from the eigenstate the floors would
        be 1.70e-14, 3.40e-14, 6.96e-14; errors against the 1600-step reference 3.810e-06, 2.337e-07, 1.454e-08: ratios 16.30, 16.07)
    (c) 8.88e-15 -> 8.59e-15 (the built-in model against dense 8.41e-15, driven against built-in 2.93e-15)
    (e) L = 7 full basis 2.48e-14 -> 6.25e-15, L = 14 nup = 1 1.55e-14 -> 4.84e-15
Norm (f): as tests/test_gpu_driven_evolve.py, |norm - 1| <= 1e-14."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import driven_ref as DR
import hopdrive_ref as HR

pytestmark = pytest.mark.gpu

A_OF = lambda t: 0.9 * math.sin(math.pi * t / 2) ** 2                                        # noqa: E731
DA_OF = lambda t: 0.9 * (math.pi / 2) * math.sin(math.pi * t)                                # noqa: E731


def make(pkg, D, L, nup, Jxy=1.0, Jz=0.7):
    """(model, dense H0).  Up to L = 10 the dense matrix is the oracle's, cut out of the 2^L x 2^L Kronecker products; beyond that
    (L = 14, nup = 1) it is built on the sector's own states (hopdrive_ref.sector_hop, driven_ref.dense_diag)."""
    hop, zz, field = D.xxz_lists(L, Jxy=Jxy, Jz=Jz)
    m = pkg.build_model(L, nup=nup, hopping=hop, zz=zz, onsite_field=field)
    if L <= 10:
        return m, D.dense_H(L, nup, hop, zz, field)
    st = D.sector_states(L, nup)
    H = HR.sector_hop(L, ([(i, j) for i, j, _J in hop], [J for _i, _j, J in hop]), st).real
    return m, H + np.diag(DR.dense_diag(st, L, (np.asarray(field, dtype=np.float64), [(i, j) for i, j, _J in zz], [J for _i, _j, J in zz])))


def states_of(D, L, nup):
    return np.arange(1 << L, dtype=np.uint64) if nup is None else D.sector_states(L, nup)


def rand_state(N, seed, cplx=True):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(N) + (1j * rng.standard_normal(N) if cplx else 0.0)
    return x / np.linalg.norm(x)


def krylov_floor(pkg, m, H0, psi0, tau, kry_m):
    """|successive krylov_time_evolve calls - dense propagator of H0|: the parent's own deviation"""
    psi = psi0
    for t in tau:
        psi = pkg.krylov_time_evolve(psi, float(t), pkg.apply_H, m, kry_m=kry_m)
    return float(np.linalg.norm(psi - DR.dense_stages(H0, [], tau, np.zeros((len(tau), 0)), psi0)))


def dense_ops(D, L, st, drives):
    """dense matrices of a mixed list of the package's drives"""
    out = []
    for d in drives:
        if hasattr(d, "weights"):
            out.append(HR.dense_hop(D, L, (d.bonds, d.weights), st) if L <= 10 else HR.sector_hop(L, (d.bonds, d.weights), st))
        else:
            out.append(np.diag(DR.dense_diag(st, L, (d.site_weights, d.bonds, list(d.bond_weights)))).astype(np.complex128))
    return out


def amplitude_ok(m, drives, coef):
    """sum_b |sum_k c_k z_{k,b}| <= sum_b |t_b| at every stage: the hopping drives of the list merged bond by bond (a bond listed
    backwards counts with its conjugate weight), which bounds the norm of sum_k c_k B_k as sum |t_b| bounds that of H0's hopping"""
    tsum = sum(abs(t) for _i, _j, t in m.hopping_list)
    for c in np.atleast_2d(coef):
        w = {}
        for ck, d in zip(c, drives):
            if hasattr(d, "weights"):
                for (i, j), z in zip(d.bonds, d.weights):
                    key, z = ((i, j), z) if i < j else ((j, i), np.conj(z))
                    w[key] = w.get(key, 0j) + ck * z
        if sum(abs(z) for z in w.values()) > tsum * (1 + 1e-12):
            return False
    return True


# ---- (a) ----
@pytest.mark.parametrize("L,nup", [(12, 6), (10, 1), (7, None)])
def test_no_hopping_is_the_diagonal_entry_bit_for_bit(pkg, L, nup):
    import torch
    m = pkg.XXZChain(L, Jxy=1.0, Jz=0.7, hz=0.2, nup=nup)
    dev = torch.device("cuda", m.ctx.device)
    tau = np.array([0.13, 0.4, 0.05])
    g, z = pkg.gradient_drive(m), pkg.zz_drive(m)
    e, c = pkg.exchange_drive(m), pkg.current_drive(m)
    dcoef = np.array([[0.3, -0.2], [0.0, 0.0], [0.0, 0.7]])
    lib = pkg.lib()
    for cplx in (False, True):
        psi0 = torch.as_tensor(rand_state(m.N, 3 + L, cplx) * 1.7, device=dev)
        if not cplx:
            psi0 = psi0.real.contiguous()
        want = pkg.stage_evolve(m, psi0, [g, z], tau, dcoef, kry_m=12)
        # hopping drives in the list (the complex-form current among them), every one of their coefficients exactly zero
        mixed = np.array([[0.0, 0.3, 0.0, -0.2], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 0.7]])
        got, info = pkg.stage_evolve(m, psi0, [e, g, c, z], tau, mixed, kry_m=12, return_info=True)
        if cplx:
            assert torch.equal(torch.view_as_real(got), torch.view_as_real(want)), (L, nup, cplx)
        else:                                   # complex form promotes a Float64 psi0 first: the bits of the ComplexF64 start
            wc = pkg.stage_evolve(m, psi0.to(torch.complex128), [g, z], tau, dcoef, kry_m=12)
            assert torch.equal(torch.view_as_real(got), torch.view_as_real(wc)), (L, nup, cplx)
        assert info["stages"] == 3
        # real form: a Float64 first stage stays Float64, as today
        got = pkg.stage_evolve(m, psi0, [e, g, z], tau, np.insert(dcoef, 0, 0.0, axis=1), kry_m=12)
        assert torch.equal(torch.view_as_real(got), torch.view_as_real(want)), (L, nup, cplx, "real form")
        # KH = 0 through the new entry itself
        dp = C.POINTER(C.c_double)
        arr, K, _keep = pkg.driven._pack(m, [g, z])
        out = torch.empty(m.N, dtype=torch.complex128, device=dev)
        cc = np.ascontiguousarray(dcoef)
        code = pkg._lib.SD_C128 if cplx else pkg._lib.SD_F64
        pkg.check(lib.sd_driven_hop_evolve_dev(m.ctx.h, m.h, code, psi0.data_ptr(), m.N, arr, K, None, 0, 3, tau.ctypes.data_as(dp),
                                               cc.ctypes.data_as(dp), 12, out.data_ptr(), None), m.ctx.h)
        assert torch.equal(torch.view_as_real(out), torch.view_as_real(want)), (L, nup, cplx, "KH = 0")
        # no coefficient at all in effect: successive Krylov calls
        plain = psi0
        for t in tau:
            plain = pkg.krylov_time_evolve(plain, float(t), pkg.apply_H, m, kry_m=12)
        got = pkg.stage_evolve(m, psi0, [e], tau, np.zeros((3, 1)), kry_m=12)
        assert torch.equal(torch.view_as_real(got), torch.view_as_real(plain)), (L, nup, cplx, "nothing in effect")


# ---- (b) ----
@functools.lru_cache(maxsize=None)
def order_problem():
    from oracle import dense as D
    L, nup = 8, 4
    hop, zz, field = D.xxz_lists(L, Jxy=1.0, Jz=0.7)
    H0 = D.dense_H(L, nup, hop, zz, field)
    st = D.sector_states(L, nup)
    w, v = np.linalg.eigh(H0)
    return H0, st, v[:, 0].astype(np.complex128)


def test_fourth_order_on_the_device(pkg, D):
    H0, st, psi0 = order_problem()
    m, H0m = make(pkg, D, 8, 4)
    assert np.array_equal(H0, H0m)
    drives, disp = pkg.peierls_drives(m)
    fs = pkg.peierls_functions(A_OF, disp)
    ops = dense_ops(D, 8, st, drives)
    ref = HR.dense_stages_general(H0, ops, *pkg.magnus_schedule(fs, 0.0, 2.0 / 1600, 1600), psi0)
    errs = []
    for n in (10, 20, 40):
        tau, coef = pkg.magnus_schedule(fs, 0.0, 2.0 / n, n, order=4)
        assert amplitude_ok(m, drives, coef)
        got = pkg.stage_evolve(m, psi0, drives, tau, coef, kry_m=20)
        errs.append(float(np.linalg.norm(got - ref)))
        dev = float(np.linalg.norm(got - HR.dense_stages_general(H0, ops, tau, coef, psi0)))
        # The floor is measured from a seeded random state: psi0 is an eigenstate of H0, from which the parent's recursion stops at
        # its first beta and its deviation (printed too) measures a phase, not the rounding of kry_m applies per stage.
        floor = krylov_floor(pkg, m, H0, rand_state(len(st), 20261021), tau, 20)
        eig = krylov_floor(pkg, m, H0, psi0, tau, 20)
        print(f"(b) n = {n}: error {errs[-1]:.3e}; floor {floor:.2e} (from the eigenstate {eig:.2e}) -> driven deviation {dev:.2e} "
              f"(allowed {16 * floor:.2e})")
        assert dev <= 16 * floor, (n, dev, floor)
    ratios = [errs[0] / errs[1], errs[1] / errs[2]]
    print("(b) ratios", ratios)
    assert all(r >= 12 for r in ratios), (errs, ratios)


# ---- (c) ----
def test_constant_exchange_drive_equals_a_scaled_model(pkg, D):
    L, nup, delta = 10, 5, 0.5
    tau = np.full(5, 0.2)
    m, H0 = make(pkg, D, L, nup)
    mb, Hb = make(pkg, D, L, nup, Jxy=1.5)
    st = states_of(D, L, nup)
    e = pkg.exchange_drive(m)
    coef = np.full((5, 1), delta)
    assert amplitude_ok(m, [e], coef)
    assert np.abs(Hb - (H0 + delta * dense_ops(D, L, st, [e])[0].real)).max() <= 1e-14
    psi0 = rand_state(len(st), 11)
    got = pkg.stage_evolve(m, psi0, [e], tau, coef, kry_m=25)
    floor = krylov_floor(pkg, m, H0, psi0, tau, 25)
    dense = DR.dense_stages(Hb, [], tau, np.zeros((5, 0)), psi0)
    dev = float(np.linalg.norm(got - dense))
    print(f"(c): floor {floor:.2e} -> driven deviation {dev:.2e} (allowed {16 * floor:.2e})")
    assert dev <= 16 * floor
    built = psi0
    for t in tau:
        built = pkg.krylov_time_evolve(built, float(t), pkg.apply_H, mb, kry_m=25)
    fb = float(np.linalg.norm(built - dense))
    print(f"(c) built-in model vs dense {fb:.2e}; driven vs built-in {np.linalg.norm(got - built):.2e}")
    assert np.linalg.norm(got - built) <= 16 * floor + fb


# ---- (d) ----
def test_gauge_equivalence_on_the_device(pkg, D):
    """Velocity gauge (Peierls drives) against length gauge (gradient_drive with -dA/dt), L = 10, nup = 5, n = 120 steps: CPU dense
    restatements agree to 4.2e-10; the assertion is 1e-8 = 10 x the CPU bound of 1e-9."""
    import torch
    L, nup, n, T = 10, 5, 120, 2.0
    m, H0 = make(pkg, D, L, nup)
    w, v = np.linalg.eigh(H0)
    psi0 = torch.as_tensor(v[:, 0].astype(np.complex128), device=torch.device("cuda", m.ctx.device))
    drives, disp = pkg.peierls_drives(m)
    vel, _ = pkg.driven_time_evolve(m, psi0, drives, pkg.peierls_functions(A_OF, disp), 0.0, T / n, n, order=4, kry_m=20)
    res = {}
    for sign in (-1.0, 1.0):
        out, _ = pkg.driven_time_evolve(m, psi0, [pkg.gradient_drive(m)], [lambda t, sign=sign: sign * DA_OF(t)], 0.0, T / n, n, order=4,
                                        kry_m=20)
        res[sign] = pkg.magnetization_per_site(out, m)
    mv, m0 = pkg.magnetization_per_site(vel, m), pkg.magnetization_per_site(psi0, m)
    d_right, d_wrong, moved = np.abs(mv - res[-1.0]).max(), np.abs(mv - res[1.0]).max(), np.abs(mv - m0).max()
    print(f"(d) gauges: E = -dA/dt {d_right:.2e} (allowed 1e-8), E = +dA/dt {d_wrong:.2e}, the pulse moves the magnetisations by {moved:.2e}")
    assert d_right <= 1e-8 and d_wrong > 0.1 and moved > 0.1


# ---- (e) ----
@pytest.mark.parametrize("L,nup", [(7, None), (14, 1)])
def test_full_basis_and_per_row_plan_against_dense(pkg, D, L, nup):
    m, H0 = make(pkg, D, L, nup)
    assert pkg.lib().sd_model_path(m.h) == 0
    st = states_of(D, L, nup)
    rng = np.random.default_rng(L)
    chain = [(i, i + 1) for i in range(1, L)]
    z = rng.standard_normal(L - 1) + 1j * rng.standard_normal(L - 1)
    hd = pkg.HoppingDrive(chain + [(L, 1)], np.append(z, 0.3 - 0.2j) * (0.4 * (L - 1) * 0.5 / np.abs(np.append(z, 0.3 - 0.2j)).sum()))
    drives = [pkg.gradient_drive(m), hd, pkg.exchange_drive(m)]
    fs = [lambda t: 0.8 * np.sin(3 * t), lambda t: math.cos(2 * t), lambda t: 0.5 * t]
    tau, coef = pkg.magnus_schedule(fs, 0.0, 0.1, 8, order=4)
    assert amplitude_ok(m, drives, coef)
    psi0 = rand_state(len(st), L)
    got = pkg.stage_evolve(m, psi0, drives, tau, coef, kry_m=20)
    dev = float(np.linalg.norm(got - HR.dense_stages_general(H0, dense_ops(D, L, st, drives), tau, coef, psi0)))
    floor = krylov_floor(pkg, m, H0, psi0, tau, 20)
    print(f"(e) L = {L} nup = {nup}: floor {floor:.2e} -> driven deviation {dev:.2e} (allowed {16 * floor:.2e})")
    assert dev <= 16 * floor


# ---- (f), (g), (h) ----
def test_norm_torch_numpy_and_promotion(pkg):
    import torch
    m = pkg.XXZChain(12, Jxy=1.0, Jz=0.7, nup=6)                         # tiled plan; no dense matrix at this size
    dev = torch.device("cuda", m.ctx.device)
    drives, disp = pkg.peierls_drives(m)
    pd = [pkg.gradient_drive(m)] + drives
    fs = [lambda t: 0.8 * math.sin(3 * t)] + pkg.peierls_functions(lambda t: 0.9 * math.sin(2 * t), disp)
    psi0 = rand_state(m.N, 21) * 3.0                                       # not normalised: the first stage does that
    norms = []

    def measure(t, psi):
        assert psi.is_cuda
        norms.append(float(torch.linalg.vector_norm(psi)))
        return t

    out_np, ts = pkg.driven_time_evolve(m, psi0, pd, fs, 0.0, 0.1, 6, order=4, kry_m=15, measure=measure, measure_every=1)
    assert len(ts) == 7 and abs(norms[0] - 3.0) <= 1e-14
    assert max(abs(x - 1.0) for x in norms[1:]) <= 1e-14, norms
    tau, coef = pkg.magnus_schedule(fs, 0.0, 0.1, 6, order=4)
    for k in range(1, len(tau) + 1):                                       # (f) ... and after every stage, not only every step
        part = pkg.stage_evolve(m, psi0, pd, tau[:k], coef[:k], kry_m=15)
        assert abs(np.linalg.norm(part) - 1.0) <= 1e-14, k
    assert np.array_equal(part.view(np.float64), out_np.view(np.float64))   # one call of 12 stages = 6 calls of 2
    # (g)
    out_t, _ = pkg.driven_time_evolve(m, torch.as_tensor(psi0, device=dev), pd, fs, 0.0, 0.1, 6, order=4, kry_m=15)
    assert out_t.is_cuda and np.array_equal(out_t.cpu().numpy().view(np.float64), out_np.view(np.float64))
    # (h) a Float64 psi0: complex form promotes it once -- the bits of the same vector passed as ComplexF64, host and device
    x = np.ascontiguousarray(psi0.real)
    a = pkg.stage_evolve(m, x, pd, tau, coef, kry_m=15)
    b = pkg.stage_evolve(m, x.astype(np.complex128), pd, tau, coef, kry_m=15)
    c = pkg.stage_evolve(m, torch.as_tensor(x, device=dev), pd, tau, coef, kry_m=15)
    assert np.array_equal(a.view(np.float64), b.view(np.float64)) and np.array_equal(a.view(np.float64), c.cpu().numpy().view(np.float64))
    # real form keeps a Float64 first stage: torch and numpy agree there as well
    rd, rf = [pkg.exchange_drive(m), pkg.gradient_drive(m)], [lambda t: 0.4 * math.sin(t), lambda t: 0.3 * t]
    tr, cr = pkg.magnus_schedule(rf, 0.0, 0.1, 3, order=4)
    a = pkg.stage_evolve(m, x, rd, tr, cr, kry_m=15)
    c = pkg.stage_evolve(m, torch.as_tensor(x, device=dev), rd, tr, cr, kry_m=15)
    assert np.array_equal(a.view(np.float64), c.cpu().numpy().view(np.float64)) and abs(np.linalg.norm(a) - 1.0) <= 1e-14
    # instantaneous energy and the drive expectations of a mixed list agree with each other
    en = pkg.instantaneous_energy(out_np, m, pd, coef[-1])
    e0 = pkg.instantaneous_energy(out_np, m, [], [])
    assert abs(en - (e0 + float(np.dot(coef[-1], pkg.drive_expectation(out_np, m, pd))))) <= 1e-12
    # refusals
    with pytest.raises(pkg.ArgumentError):
        pkg.stage_evolve(m, psi0, pd, [0.1], [[np.nan, 0.0, 0.0]])
    with pytest.raises(pkg.ArgumentError):
        pkg.stage_evolve(m, psi0, [pkg.HoppingDrive([(1, 13)])], [0.1], [[1.0]])
    with pytest.raises(pkg.DimensionMismatch):
        pkg.stage_evolve(m, psi0[:-1].copy(), pd, [0.1], [[1.0, 0.0, 0.0]])
