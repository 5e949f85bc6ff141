"""CPU checks of the hopping-drive layer: the restatement tests/hopdrive_ref.py against an independent dense
construction, the Peierls decomposition, the order of the Magnus schedule with non-commuting hopping drives, the gauge equivalence
with the existing gradient drive, the limits sd_hop_drive_check answers with SD_EARG, the exports, and the column permutation of
mixed drive lists."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import driven_ref as DR
import hopdrive_ref as HR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53


def lists(L):
    """name -> (drives as hopdrive_ref tuples, coefficients)"""
    rng = np.random.default_rng(40 + L)
    chain = [(i, i + 1) for i in range(1, L)]
    cz = lambda n: rng.standard_normal(n) + 1j * rng.standard_normal(n)                      # noqa: E731
    return {
        "real chain": ([(chain, rng.standard_normal(L - 1))], [0.8]),
        "complex chain": ([(chain, cz(L - 1))], [-1.3]),
        "reversed and repeated": ([([(2, 1), (1, 2), (1, 2), (L, 1), (1, L), (5, 3)], cz(6))], [0.6]),
        "real reversed and repeated": ([([(2, 1), (1, 2), (1, 2), (L, 1), (5, 3)], rng.standard_normal(5))], [1.1]),
        "K3 with a zero": ([(chain, cz(L - 1)), ([(1, 3), (2, 4)], [2.0, -1.0]), ([(L, 1), (3, 1)], [0.5, 0.25j])], [0.9, 0.0, -0.35]),
    }


@pytest.mark.parametrize("nup", [1, 4, 7, None])
def test_restatement_against_dense_B_on_every_row(D, nup):
    """Both sides are sums of at most n products; either carries at most (n + 2) u sum |c z| max |psi| per component for a real list
    (the forward bound of a sequential sum with one rounding per product) and twice that where a product is complex (two real
    products and an add per component): the difference is allowed the sum of the two."""
    L = 8
    st = D.sector_states(L, nup).astype(np.int64) if nup is not None else np.arange(1 << L, dtype=np.int64)
    index = {int(s): k for k, s in enumerate(st)}
    rank = lambda cfg: np.array([index.get(int(c), -1) for c in cfg], dtype=np.int64)        # noqa: E731
    idx = np.arange(len(st), dtype=np.int64)
    rng = np.random.default_rng(9)
    psi_c = rng.standard_normal(len(st)) + 1j * rng.standard_normal(len(st))
    for name, (drives, coefs) in lists(L).items():
        cf, el = HR.effective_list(drives, coefs)
        assert cf == ("real" not in name)
        assert len(el) == sum(len(d[0]) for d, c in zip(drives, coefs) if c != 0.0)
        B = sum(c * HR.dense_hop(D, L, d, st) for c, d in zip(coefs, drives))
        assert np.abs(B - B.conj().T).max() == 0.0                                           # Hermitian, exactly
        if nup is not None:                                                                  # the sector-level construction is the same matrix
            assert np.array_equal(B, sum(c * HR.sector_hop(L, d, st) for c, d in zip(coefs, drives)))
        for psi in ([psi_c] if cf else [psi_c, psi_c.real.copy()]):
            parts = HR.partner_rows(st, idx, el, rank if nup is not None else None)
            got = HR.hop_rows(None, psi, st, parts, el, cf)
            want = B @ psi
            wsum = sum(abs(complex(x, y)) for (_i, _j, x, y) in el)
            bound = 2 * 2 * (len(el) + 2) * U * wsum * np.abs(psi).max()
            err = np.abs(got - want).max()
            assert np.abs(want).max() > 0.1 and err <= bound, (name, nup, err, bound)
            assert got.dtype == psi.dtype
            # acc is carried through: y + B psi
            y = rng.standard_normal(len(st)) + (1j * rng.standard_normal(len(st)) if np.iscomplexobj(psi) else 0)
            y = y if np.iscomplexobj(psi) else y.real
            assert np.abs(HR.hop_rows(y, psi, st, parts, el, cf) - (y + want)).max() <= bound + 4 * U * np.abs(y).max()


def test_the_order_and_the_selection_are_the_contracts(D):
    """one row by a plain loop: list order, y' selected by which site is up"""
    L = 6
    drives = [([(4, 2), (2, 4), (1, 6)], [0.3 + 0.7j, -1.1 + 0.2j, 0.5 - 0.4j])]
    cf, el = HR.effective_list(drives, [1.7])
    assert cf and el[0][:2] == (3, 1)
    st = np.arange(1 << L, dtype=np.int64)
    rng = np.random.default_rng(3)
    psi = rng.standard_normal(1 << L) + 1j * rng.standard_normal(1 << L)
    got = HR.hop_rows(None, psi, st, HR.partner_rows(st, st, el), el, cf)
    for cfg in (0b001010, 0b000010, 0b100010, 0b001001):
        re, im = 0.0, 0.0
        for (bi, bj, x, y) in el:
            ui, uj = (cfg >> bi) & 1, (cfg >> bj) & 1
            if ui == uj:
                continue
            v = psi[cfg ^ ((1 << bi) | (1 << bj))]
            yp = y if ui else -y
            tr = x * v.real - yp * v.imag
            ti = x * v.imag + yp * v.real
            re, im = re + tr, im + ti
        assert got[cfg].real == re and got[cfg].imag == im


def peierls_model(pkg, L, nup):
    hop = [(i, i + 1, 0.5) for i in range(1, L)] + [(i, i + 2, 0.15 * (1 + 0.1 * i)) for i in range(1, L - 1)] + [(5, 3, -0.2)]
    zz = [(i, i + 1, 0.7) for i in range(1, L)]
    return pkg.Model(L, nup=nup, hopping=hop, zz=zz, ctx=None), hop, zz


def test_peierls_decomposition_is_exact(pkg, D):
    """H0 + sum_delta [(cos(delta A) - 1) T_delta + sin(delta A) J_delta] against the Hamiltonian built directly with the phases
    e^{i A (j - i)} on S^+_i S^-_j, nearest neighbours plus a second-neighbour class (one bond of it listed backwards).  The two differ
    by the rounding of t cos(delta A) against t + t (cos(delta A) - 1): a few ulp of max |t|."""
    L, nup = 8, 4
    m, hop, zz = peierls_model(pkg, L, nup)
    st = D.sector_states(L, nup)
    H0 = D.dense_H(L, nup, hop, zz, np.zeros(L))
    drives, disp = pkg.peierls_drives(m)
    assert disp == [1, 2] and len(drives) == 4
    assert all(d.is_real for d in drives[0::2]) and not any(d.is_real for d in drives[1::2])
    assert (3, 5) in drives[2].bonds and (5, 3) not in drives[2].bonds               # turned round: delta > 0
    ops = [HR.dense_hop(D, L, (d.bonds, d.weights), st) for d in drives]
    for A in (0.0, 0.37, -1.9):
        fs = pkg.peierls_functions(lambda t: A, disp)
        H = H0.astype(np.complex128)
        for f, op in zip(fs, ops):
            H = H + f(0.0) * op
        direct = D.dense_H(L, nup, [], zz, np.zeros(L)).astype(np.complex128)
        full = np.zeros((1 << L, 1 << L), dtype=np.complex128)
        for (i, j, t) in hop:
            pm = D.site_op(D.SP, i, L) @ D.site_op(D.SM, j, L)
            z = t * np.exp(1j * A * (j - i))
            full += z * pm + np.conj(z) * pm.T
        s64 = st.astype(np.int64)
        direct = direct + full[np.ix_(s64, s64)]
        assert np.abs(H - H.conj().T).max() == 0.0
        assert np.abs(H - direct).max() <= 8 * U * 0.5, (A, np.abs(H - direct).max())
    # the current classes add up to the spin current towards higher sites: current_drive with -1 on the bond listed backwards
    cd = pkg.current_drive(m, weights=[1.0 if j > i else -1.0 for (i, j, _t) in hop])
    cur = HR.dense_hop(D, L, (cd.bonds, cd.weights), st)
    assert np.abs(ops[1] + ops[3] - cur).max() <= 4 * U
    # a ring: minimum images, and the ambiguous displacement refused
    ring = pkg.XXZChain(8, nup=4, boundary="periodic", ctx=None)
    dr, dp = pkg.peierls_drives(ring, boundary="periodic")
    assert dp == [1] and (8, 1) in dr[0].bonds
    with pytest.raises(pkg.ArgumentError):
        pkg.peierls_drives(pkg.Model(8, nup=4, hopping=[(1, 5, 1.0)], ctx=None), boundary="periodic")


def pulse_problem(pkg, D):
    """the order problem: open XXZ chain L = 8, nup = 4, Jxy = 1, Jz = 0.7, from its ground state under the Peierls phase of
    A(t) = 0.9 sin^2(pi t / 2), T = 2"""
    L, nup = 8, 4
    hop, zz, field = D.xxz_lists(L, Jxy=1.0, Jz=0.7)
    H0 = D.dense_H(L, nup, hop, zz, field)
    st = D.sector_states(L, nup)
    m = pkg.XXZChain(L, Jxy=1.0, Jz=0.7, nup=nup, ctx=None)
    drives, disp = pkg.peierls_drives(m)
    ops = [HR.dense_hop(D, L, (d.bonds, d.weights), st) for d in drives]
    A = lambda t: 0.9 * math.sin(math.pi * t / 2) ** 2                                       # noqa: E731
    w, v = np.linalg.eigh(H0)
    return m, H0, st, ops, pkg.peierls_functions(A, disp), v[:, 0].astype(np.complex128), 2.0


def test_order_with_hopping_drives(pkg, D):
    """Errors against 1600 steps at n = 10, 20, 40, 80 of magnus_schedule (unchanged by the new operators) through the dense stage
    propagator with the non-commuting T_1, J_1: 3.81e-6, 2.34e-7, 1.45e-8, 9.08e-10, ratios 16.30, 16.07, 16.02.  Condition: every ratio
    in [14, 18]; with the two stages of a step exchanged the method is second order, ratio ~ 4 (condition: in [3, 6])."""
    _m, H0, _st, ops, fs, psi0, T = pulse_problem(pkg, D)
    ref = HR.dense_stages_general(H0, ops, *pkg.magnus_schedule(fs, 0.0, T / 1600, 1600, order=4), psi0)
    errs = []
    for n in (10, 20, 40, 80):
        tau, coef = pkg.magnus_schedule(fs, 0.0, T / n, n, order=4)
        errs.append(np.linalg.norm(HR.dense_stages_general(H0, ops, tau, coef, psi0) - ref))
    r = [a / b for a, b in zip(errs[:-1], errs[1:])]
    print("order 4", errs, r)
    assert all(14 <= x <= 18 for x in r), (errs, r)
    es = [np.linalg.norm(HR.dense_stages_general(H0, ops, *DR.magnus_schedule(fs, 0.0, T / n, n, swap=True), psi0) - ref) for n in (40, 80)]
    print("swapped", es, es[0] / es[1])
    assert 3 <= es[0] / es[1] <= 6


def test_gauge_equivalence_dense(pkg, D):
    """The Peierls run (velocity gauge) against the existing gradient_drive with f = -dA/dt (length gauge), site magnetisations at
    t = T.  At n = 160 fourth-order steps either run is within ~6e-11 of its limit (the order test: 9.08e-10 at n = 80, a factor 16 per
    halving), so the two sets of magnetisations must agree to 1e-9; with the other sign they differ by ~0.5."""
    m, H0, st, ops, fs, psi0, T = pulse_problem(pkg, D)
    L, n = 8, 160
    s = st.astype(np.int64)
    sz = np.array([((s >> i) & 1) - 0.5 for i in range(L)])
    mags = lambda psi: sz @ (np.abs(psi) ** 2)                                               # noqa: E731
    vel = HR.dense_stages_general(H0, ops, *pkg.magnus_schedule(fs, 0.0, T / n, n), psi0)
    g = pkg.gradient_drive(m)
    gd = [DR.dense_diag(st, L, (g.site_weights, [], []))]
    dA = lambda t: 0.9 * (math.pi / 2) * math.sin(math.pi * t)                               # noqa: E731   d/dt 0.9 sin^2(pi t / 2)
    got = {}
    for sign in (-1.0, 1.0):
        tau, coef = pkg.magnus_schedule([lambda t, sign=sign: sign * dA(t)], 0.0, T / n, n)
        got[sign] = mags(DR.dense_stages(H0, gd, tau, coef, psi0))
    d_right, d_wrong = np.abs(mags(vel) - got[-1.0]).max(), np.abs(mags(vel) - got[1.0]).max()
    moved = np.abs(mags(vel) - mags(psi0)).max()
    print(f"gauge: E = -dA/dt {d_right:.2e}, E = +dA/dt {d_wrong:.2e}, the pulse moves the magnetisations by {moved:.2e}")
    assert d_right <= 1e-9 and d_wrong > 0.1 and moved > 0.1


def test_hop_drive_check_rejections(pkg):
    m = pkg.XXZChain(8, nup=4, ctx=None)
    H = pkg.HoppingDrive
    pkg.drive_check(m, [pkg.exchange_drive(m), pkg.current_drive(m), H([(1, 3), (3, 1), (1, 3)], [1.0, 2j, 0.5])])
    pkg.drive_check(m, [H([])] * 16)
    pkg.drive_check(m, [H([(1, 2)] * 64)] * 2)                                               # exactly 128 terms
    pkg.drive_check(m, [pkg.gradient_drive(m)] * 8 + [H([(1, 2)])] * 8)                      # K + KH = 16
    bad = {
        "too many drives": [H([])] * 17,
        "too many with the diagonal ones": [pkg.gradient_drive(m)] * 8 + [H([(1, 2)])] * 9,
        "too many terms": [H([(1, 2)] * 65)] * 2,
        "site 0": [H([(0, 2)])],
        "site L + 1": [H([(2, 9)])],
        "i == j": [H([(3, 3)])],
        "nan weight": [H([(1, 2)], [np.nan])],
        "inf imaginary part": [H([(1, 2)], [complex(0.0, np.inf)])],
    }
    for name, drives in bad.items():
        with pytest.raises(pkg.ArgumentError):
            pkg.drive_check(m, drives)
    with pytest.raises(pkg.ArgumentError):
        pkg.drive_check(m, [object()])
    # the raw status
    hd = (pkg._lib.sd_hop_drive * 1)()
    hi, hj, re = (C.c_int * 1)(3), (C.c_int * 1)(3), (C.c_double * 1)(1.0)
    hd[0].n, hd[0].i, hd[0].j, hd[0].re = 1, hi, hj, re
    assert pkg.lib().sd_hop_drive_check(m.h, hd, 1) == pkg._lib.SD_EARG
    hj[0] = 4
    assert pkg.lib().sd_hop_drive_check(m.h, hd, 1) == pkg._lib.SD_OK
    assert pkg.lib().sd_hop_drive_check(m.h, hd, -1) == pkg._lib.SD_EARG
    hd[0].re = None
    assert pkg.lib().sd_hop_drive_check(m.h, hd, 1) == pkg._lib.SD_EARG                      # a null list


def test_exports_and_layout(pkg):
    for name in ("HoppingDrive", "exchange_drive", "current_drive", "peierls_drives", "peierls_functions", "hopping_apply",
                 "drive_expectation"):
        assert hasattr(pkg, name) and name in pkg.__all__, name
    for name in ("sd_hop_drive_check", "sd_hop_apply", "sd_hop_apply_dev", "sd_driven_hop_apply", "sd_driven_hop_apply_dev",
                 "sd_driven_hop_evolve", "sd_driven_hop_evolve_dev"):
        assert name in pkg.PROTOTYPES and hasattr(pkg.lib(), name), name
    assert [f[0] for f in pkg._lib.sd_hop_drive._fields_] == ["n", "i", "j", "re", "im"]
    assert C.sizeof(pkg._lib.sd_hop_drive) == 40 and pkg._lib.sd_hop_drive.i.offset == 8
    assert pkg.driven.MAX_HOP_BONDS == 128
    src = open(os.path.join(ROOT, "include", "spindyn.h")).read()
    assert "#define SD_HOP_MAX_BONDS 128" in src
    m = pkg.XXZChain(6, Jxy=0.8, nup=3, ctx=None)
    e = pkg.exchange_drive(m)
    assert e.bonds == [(i, i + 1) for i in range(1, 6)] and np.array_equal(e.weights, np.full(5, 0.4 + 0j)) and e.is_real
    c = pkg.current_drive(m, weights=[1, 2, 3, 4, 5])
    assert np.array_equal(c.weights, 1j * 0.4 * np.arange(1, 6)) and not c.is_real
    assert pkg.HoppingDrive([(1, 2)], [1.0 + 0j])._im is None                               # real weights travel without an im list


def test_mixed_lists_reach_the_library_with_the_diagonal_columns_first(pkg):
    m = pkg.XXZChain(6, nup=3, ctx=None)
    g, z, e, c = pkg.gradient_drive(m), pkg.zz_drive(m), pkg.exchange_drive(m), pkg.current_drive(m)
    drives, di, hi = pkg.driven._split([e, g, c, z])
    assert di == [1, 3] and hi == [0, 2] and drives == [e, g, c, z]
    coef = np.arange(12, dtype=np.float64).reshape(3, 4)
    got = pkg.driven._permute_columns(coef, di, hi)
    assert got.flags["C_CONTIGUOUS"] and np.array_equal(got, coef[:, [1, 3, 0, 2]])
    assert np.array_equal(pkg.driven._permute_columns(coef[0], di, hi), [1.0, 3.0, 0.0, 2.0])
    assert pkg.driven._split(g) == ([g], [0], []) and pkg.driven._split(e) == ([e], [], [0])
    # the hop array as the library reads it
    arr, KH = pkg.driven._pack_hops([e, c])
    assert KH == 2 and arr[0].n == 5 and not arr[0].im and bool(arr[1].im)
    assert [arr[1].i[b] for b in range(5)] == [1, 2, 3, 4, 5] and arr[1].im[2] == 0.5 * 1.0
