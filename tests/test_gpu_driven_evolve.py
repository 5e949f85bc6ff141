"""sd_driven_evolve (stage_evolve, driven_time_evolve) on the GPU.

(a) K = 0, and a stage whose coefficients are all exactly zero, give the bits of as many successive sd_krylov_evolve_dev calls.
(b) The order-test problem of tests/test_driven_ref_host.py at n = 10, 20, 40 steps of order 4 with kry_m = 20: both error ratios
    against the dense 1600-step reference >= 12, and each result within the tolerance of the dense product of the same stages.
(c) A constant drive against a model with the same field and Jz built in.
(d) The commuting drive D = sum_i S^z_i (L = 8, nup = 3: M = -1), cubic f(t) = 0.3 + 0.5 t - 0.7 t^2 + 0.2 t^3, T = 1.5, 6 steps of
    order 4: two-point Gauss quadrature is exact for a cubic, so the result is e^{-i M int f} times the same stages of H0 alone.
(e) The full basis at L = 7 and the dilute sector L = 10, nup = 1 (tiles of at most 10 rows) against dense.
(f) Norm 1 after every stage.   (g) A torch device vector gives the bits of the numpy vector.

Tolerance of (b)-(e).  The floor is the 2-norm deviation of the existing krylov_time_evolve, on the same model with the same stage
durations, kry_m and number of calls, from the dense propagator of H0: code from before the drives, measured by the test itself in
the same run.  The driven result may deviate from its own dense product by 8 times that: the drive adds one rounding per row and
apply, the Krylov space is otherwise the same.  Measured on an MI355X (floor -> driven deviation):
    (b) n = 10: 2.46e-14 -> 7.22e-15;  n = 20: 4.71e-14 -> 9.96e-15;  n = 40: 9.66e-14 -> 1.69e-14  (errors against the 1600-step
        reference 1.567e-05, 9.685e-07, 6.036e-08: ratios 16.18, 16.04)
    (c) 8.88e-15 -> 9.57e-15;  (d) 1.74e-14 -> 1.01e-14;  (e) L = 7 full basis 2.48e-14 -> 6.18e-15, L = 10 nup = 1 9.69e-15 -> 5.28e-15
Norm (f): every stage ends with a division by the computed norm; that norm and the check's own are sums of N products, each good to
(log2 N + 2) 2^-53 relative, so |norm - 1| <= 1e-14 with room for N up to 2^40."""
import functools
import math

import numpy as np
import pytest

import driven_ref as DR

pytestmark = pytest.mark.gpu


def make(pkg, D, L, nup, Jz=0.7, hz=0.0):
    hop, zz, field = D.xxz_lists(L, Jxy=1.0, Jz=Jz, hz=hz)
    return pkg.build_model(L, nup=nup, hopping=hop, zz=zz, onsite_field=field), D.dense_H(L, nup, hop, zz, field)


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


def to_pkg(pkg, drives):
    return [pkg.DiagonalDrive(site_weights=w, bonds=b, bond_weights=v) for (w, b, v) in drives]


def driven_case(pkg, D, L, nup, drives, tau, coef, kry_m, label, seed=1, Jz=0.7):
    m, H0 = make(pkg, D, L, nup, Jz=Jz)
    st = states_of(D, L, nup)
    psi0 = rand_state(len(st), seed)
    diags = [DR.dense_diag(st, L, d) for d in drives]
    got = pkg.stage_evolve(m, psi0, to_pkg(pkg, drives), tau, coef, kry_m=kry_m)
    dev = float(np.linalg.norm(got - DR.dense_stages(H0, diags, tau, coef, psi0)))
    floor = krylov_floor(pkg, m, H0, psi0, tau, kry_m)
    print(f"{label}: floor {floor:.2e} -> driven deviation {dev:.2e} (allowed {8 * floor:.2e})")
    assert dev <= 8 * floor, (label, dev, floor)
    return got, m, H0, psi0, diags


# ---- (a) ----
@pytest.mark.parametrize("L,nup", [(12, 6), (10, 1), (7, None)])
def test_no_drive_is_successive_krylov_calls_bit_for_bit(pkg, L, nup):
    import torch
    m = pkg.XXZChain(L, Jxy=1.0, Jz=0.7, hz=0.2, nup=nup)
    dev = torch.device("cuda", m.ctx.device)
    tau = np.array([0.13, 0.4, 0.05])
    for cplx in (False, True):
        psi0 = torch.as_tensor(rand_state(m.N, 3 + L, cplx) * 1.7, device=dev)
        if not cplx:
            psi0 = psi0.real.contiguous()
        want = psi0
        for t in tau:
            want = pkg.krylov_time_evolve(want, float(t), pkg.apply_H, m, kry_m=12)
        before = m.ctx.apply_count()
        got, info = pkg.stage_evolve(m, psi0, [], tau, np.zeros((3, 0)), kry_m=12, return_info=True)
        assert torch.equal(torch.view_as_real(got), torch.view_as_real(want)), (L, nup, cplx)
        assert info["stages"] == 3 and info["applies"] == m.ctx.apply_count() - before and info["min_beta"] >= 0
        # drives present, every coefficient exactly zero: the same path, the same bits
        got = pkg.stage_evolve(m, psi0, [pkg.gradient_drive(m), pkg.zz_drive(m)], tau, np.zeros((3, 2)), kry_m=12)
        assert torch.equal(torch.view_as_real(got), torch.view_as_real(want)), (L, nup, cplx, "zero coefficients")


# ---- (b) ----
@functools.lru_cache(maxsize=None)
def order_problem():
    from oracle import dense as D
    L, nup = 8, 4
    hop, zz, field = D.xxz_lists(L, Jxy=1.0, Jz=0.7)
    H0 = D.dense_H(L, nup, hop, zz, field)
    st = D.sector_states(L, nup)
    drives = [(np.arange(L) - 3.5, [], []), (None, [(i, i + 1) for i in range(1, L)], [1.0] * (L - 1))]
    diags = [DR.dense_diag(st, L, d) for d in drives]
    fs = (lambda t: 0.8 * np.sin(3 * t), lambda t: 0.5 * t)
    psi0 = rand_state(len(st), 20261021)
    ref = DR.dense_stages(H0, diags, *DR.magnus_schedule(fs, 0.0, 2.0 / 1600, 1600), psi0)
    return drives, diags, fs, psi0, ref, H0


def test_fourth_order_on_the_device(pkg, D):
    drives, diags, fs, psi0, ref, H0 = order_problem()
    m, H0m = make(pkg, D, 8, 4)
    assert np.array_equal(H0, H0m)
    pd = [pkg.gradient_drive(m), pkg.zz_drive(m)]
    assert np.array_equal(pd[0].site_weights, drives[0][0]) and pd[1].bonds == drives[1][1]
    errs = []
    for n in (10, 20, 40):
        tau, coef = pkg.magnus_schedule(fs, 0.0, 2.0 / n, n, order=4)
        got = pkg.stage_evolve(m, psi0, pd, tau, coef, kry_m=20)
        errs.append(float(np.linalg.norm(got - ref)))
        dev = float(np.linalg.norm(got - DR.dense_stages(H0, diags, tau, coef, psi0)))
        floor = krylov_floor(pkg, m, H0, psi0, tau, 20)
        print(f"(b) n = {n}: error {errs[-1]:.3e}; floor {floor:.2e} -> driven deviation {dev:.2e} (allowed {8 * floor:.2e})")
        assert dev <= 8 * floor, (n, dev, floor)
    ratios = [errs[0] / errs[1], errs[1] / errs[2]]
    print("(b) ratios", ratios)
    assert all(r >= 12 for r in ratios), (errs, ratios)


# ---- (c) ----
def test_constant_drive_equals_the_built_in_couplings(pkg, D):
    L, nup, hz, dJz = 10, 5, 0.35, 0.4
    tau = np.full(5, 0.2)
    coef = np.tile([hz, dJz], (5, 1))
    chain = [(i, i + 1) for i in range(1, L)]
    drives = [(np.ones(L), [], []), (None, chain, [1.0] * (L - 1))]
    got, m, H0, psi0, diags = driven_case(pkg, D, L, nup, drives, tau, coef, 25, "(c)", seed=11)
    mb, Hb = make(pkg, D, L, nup, Jz=0.7 + dJz, hz=hz)
    assert np.abs(Hb - (H0 + hz * np.diag(diags[0]) + dJz * np.diag(diags[1]))).max() <= 1e-14
    built = psi0
    for t in tau:
        built = pkg.krylov_time_evolve(built, float(t), pkg.apply_H, mb, kry_m=25)
    dense = DR.dense_stages(Hb, [], tau, np.zeros((5, 0)), psi0)
    fb = float(np.linalg.norm(built - dense))
    print(f"(c) built-in model vs dense {fb:.2e}; driven vs built-in {np.linalg.norm(got - built):.2e}")
    # the two deviations from the one dense propagator, added: 8 floors for the driven run, its own for the built-in one
    assert np.linalg.norm(got - built) <= 8 * krylov_floor(pkg, m, H0, psi0, tau, 25) + fb


# ---- (d) ----
def test_commuting_drive_is_a_phase(pkg, D):
    L, nup, T, n = 8, 3, 1.5, 6
    f = lambda t: 0.3 + 0.5 * t - 0.7 * t ** 2 + 0.2 * t ** 3          # noqa: E731
    integral = 0.3 * T + 0.25 * T ** 2 - 0.7 / 3 * T ** 3 + 0.05 * T ** 4
    tau, coef = pkg.magnus_schedule([f], 0.0, T / n, n, order=4)
    assert abs(float((tau * coef[:, 0]).sum()) - integral) <= 1e-14      # two-point Gauss quadrature is exact for a cubic (12 rounded terms)
    got, m, H0, psi0, diags = driven_case(pkg, D, L, nup, [(np.ones(L), [], [])], tau, coef, 20, "(d)", seed=4)
    M = nup - L / 2
    assert np.array_equal(diags[0], np.full(len(psi0), M))
    alone = DR.dense_stages(H0, [], tau, np.zeros((len(tau), 0)), psi0)
    floor = krylov_floor(pkg, m, H0, psi0, tau, 20)
    err = float(np.linalg.norm(got - np.exp(-1j * M * integral) * alone))
    print(f"(d) against the phase times the stages of H0 alone: {err:.2e} (allowed {8 * floor:.2e})")
    assert err <= 8 * floor


# ---- (e) ----
@pytest.mark.parametrize("L,nup", [(7, None), (10, 1)])
def test_full_basis_and_dilute_sector_against_dense(pkg, D, L, nup):
    drives = [(np.arange(L) - (L - 1) / 2, [(1, 2), (2, L)], [0.6, -0.9]), (None, [(i, i + 1) for i in range(1, L)], [1.0] * (L - 1))]
    fs = [lambda t: 0.8 * np.sin(3 * t), lambda t: 0.5 * t]
    tau, coef = pkg.magnus_schedule(fs, 0.0, 0.1, 8, order=4)
    got, m, *_ = driven_case(pkg, D, L, nup, drives, tau, coef, 20, f"(e) L = {L} nup = {nup}", seed=L)
    assert m.nup == nup and (nup is not None or pkg.lib().sd_model_path(m.h) == 0)       # L = 7: the full basis row by row


# ---- (f), (g) ----
def test_norm_after_every_stage_and_torch_equals_numpy(pkg):
    import torch
    m = pkg.XXZChain(12, Jxy=1.0, Jz=0.7, nup=6)                         # tiled plan; no dense matrix at this size
    dev = torch.device("cuda", m.ctx.device)
    pd = [pkg.gradient_drive(m), pkg.zz_drive(m)]
    fs = [lambda t: 0.8 * math.sin(3 * t), lambda t: 0.5 * t]
    psi0 = rand_state(m.N, 21) * 3.0                                       # not normalised: the first stage does that
    norms = []

    def measure(t, psi):
        assert psi.is_cuda
        norms.append(float(torch.linalg.vector_norm(psi)))
        return t

    out_np, ts = pkg.driven_time_evolve(m, psi0, pd, fs, 0.0, 0.1, 6, order=4, kry_m=15, measure=measure, measure_every=1)
    assert len(ts) == 7 and abs(ts[-1] - 0.6) <= 1e-15 and abs(norms[0] - 3.0) <= 1e-14
    assert max(abs(x - 1.0) for x in norms[1:]) <= 1e-14, norms
    tau, coef = pkg.magnus_schedule(fs, 0.0, 0.1, 6, order=4)
    for k in range(1, len(tau) + 1):                                       # ... and after every stage, not only every step
        part = pkg.stage_evolve(m, psi0, pd, tau[:k], coef[:k], kry_m=15)
        assert abs(np.linalg.norm(part) - 1.0) <= 1e-14, k
    assert np.array_equal(part.view(np.float64), out_np.view(np.float64))   # one call of 12 stages = 6 calls of 2
    out_t, _ = pkg.driven_time_evolve(m, torch.as_tensor(psi0, device=dev), pd, fs, 0.0, 0.1, 6, order=4, kry_m=15)
    assert out_t.is_cuda and np.array_equal(out_t.cpu().numpy().view(np.float64), out_np.view(np.float64))
    # a real start vector
    x = np.ascontiguousarray(psi0.real)
    a = pkg.stage_evolve(m, x, pd, tau, coef, kry_m=15)
    b = pkg.stage_evolve(m, torch.as_tensor(x, device=dev), pd, tau, coef, kry_m=15)
    assert np.array_equal(a.view(np.float64), b.cpu().numpy().view(np.float64))
    # refusals
    with pytest.raises(pkg.ArgumentError):
        pkg.stage_evolve(m, psi0, pd, [0.1], [[np.nan, 0.0]])
    with pytest.raises(pkg.ArgumentError):
        pkg.stage_evolve(m, psi0, [pkg.DiagonalDrive(bonds=[(1, 13)])], [0.1], [[1.0]])
    with pytest.raises(pkg.DimensionMismatch):
        pkg.stage_evolve(m, psi0[:-1].copy(), pd, [0.1], [[1.0, 0.0]])
