"""CPU checks of the driven-dynamics layer: the restatement tests/driven_ref.py against an independent dense
construction, the limits sd_drive_check answers with SD_EARG, the exports, and the order of the two stage schedules -- the
package's own magnus_schedule, run through the dense stage propagator."""
import ctypes as C

import numpy as np
import pytest

import driven_ref as DR


def problem(D):
    """the order test's problem: open XXZ chain L = 8, nup = 4, Jxy = 1, Jz = 0.7; D1 = gradient (0-based weights i - 3.5) with
    f1 = 0.8 sin 3t, D2 = the chain's zz bonds of weight 1 with f2 = 0.5 t; T = 2; a seeded random normalised complex psi0"""
    L, nup = 8, 4
    hop, zz, field = D.xxz_lists(L, Jxy=1.0, Jz=0.7)
    H0 = D.dense_H(L, nup, hop, zz, field)
    st = D.sector_states(L, nup)
    drives = [(np.arange(L) - 3.5, [], []), (None, [(i, i + 1) for i in range(1, L)], [1.0] * (L - 1))]
    diags = [DR.dense_diag(st, L, d) for d in drives]
    fs = [lambda t: 0.8 * np.sin(3 * t), lambda t: 0.5 * t]
    rng = np.random.default_rng(20261021)
    psi0 = rng.standard_normal(len(st)) + 1j * rng.standard_normal(len(st))
    return H0, diags, fs, psi0 / np.linalg.norm(psi0), 2.0


def test_diag_values_against_an_independent_dense_operator(D):
    L = 8
    rng = np.random.default_rng(5)
    drives = [(rng.standard_normal(L), [(1, 2), (3, 7), (8, 1)], [0.3, -1.1, 2.0]),
              (None, [(3, 7), (2, 5)], [0.7, 0.25]),
              (rng.standard_normal(L), [], [])]
    coefs = [0.8, -0.35, 1.7]
    s = np.arange(1 << L)
    got = DR.diag_values(s, L, DR.effective_weights(L, drives, coefs))
    SZ = D.SZ
    want = np.zeros((1 << L, 1 << L))
    mag = 0.0
    for c, (w, bonds, v) in zip(coefs, drives):
        if w is not None:
            for i in range(L):
                want += c * w[i] * D.site_op(SZ, i + 1, L)
                mag += abs(c * w[i]) / 2
        for (i, j), x in zip(bonds, v):
            want += c * x * D.site_op(SZ, i, L) @ D.site_op(SZ, j, L)
            mag += abs(c * x) / 4
    assert np.count_nonzero(want - np.diag(np.diag(want))) == 0
    assert np.diag(D.site_op(SZ, 1, L))[1] > 0              # state index 1 = site 1 up = +1/2
    n_terms = 2 * L + 5
    err = np.abs(got - np.diag(want)).max()
    assert err <= 2 * n_terms * 2.0 ** -53 * mag, err
    # without site weights the site loop is skipped; a zero coefficient leaves exact zeros behind
    tb = DR.effective_weights(L, drives[1:2], [0.0])
    assert not tb[0] and np.array_equal(DR.diag_values(s, L, tb), np.zeros(1 << L))
    # the order of the sum is the contract's: one configuration by a plain loop
    has, wh, bits, vq = DR.effective_weights(L, drives, coefs)
    cfg = 0b10110010
    d = 0.0
    for i in range(L):
        d += wh[i] if (cfg >> i) & 1 else -wh[i]
    for (bi, bj), q in zip(bits, vq):
        d += q if ((cfg >> bi) & 1) == ((cfg >> bj) & 1) else -q
    assert got[cfg] == d


def _check(pkg, m, drives):
    pkg.drive_check(m, drives)


def test_drive_check_rejections(pkg):
    m = pkg.XXZChain(8, nup=4, ctx=None)
    ok = [pkg.gradient_drive(m), pkg.zz_drive(m), pkg.field_drive(m), pkg.DiagonalDrive(bonds=[(1, 3), (1, 3)], bond_weights=[1.0, 2.0])]
    _check(pkg, m, ok)
    _check(pkg, m, [])
    _check(pkg, m, [pkg.DiagonalDrive()] * 16)
    bad = {
        "too many drives": [pkg.DiagonalDrive()] * 17,
        "too many bonds": [pkg.DiagonalDrive(bonds=[(1, 2)] * 65)] * 2,
        "site 0": [pkg.DiagonalDrive(bonds=[(0, 2)])],
        "site L + 1": [pkg.DiagonalDrive(bonds=[(2, 9)])],
        "i == j": [pkg.DiagonalDrive(bonds=[(3, 3)])],
        "nan site weight": [pkg.DiagonalDrive(site_weights=[0, 1, 2, np.nan, 4, 5, 6, 7])],
        "inf bond weight": [pkg.DiagonalDrive(bonds=[(1, 2)], bond_weights=[np.inf])],
    }
    for name, drives in bad.items():
        with pytest.raises(pkg.ArgumentError):
            _check(pkg, m, drives)
    _check(pkg, m, [pkg.DiagonalDrive(bonds=[(1, 2)] * 64)] * 2)          # exactly 128 terms
    with pytest.raises(pkg.ArgumentError):                                 # the wrong number of site weights never reaches the library
        _check(pkg, m, [pkg.DiagonalDrive(site_weights=np.ones(7))])
    # the raw status
    dr = (pkg._lib.sd_drive * 1)()
    zi, zj, zw = (C.c_int * 1)(3), (C.c_int * 1)(3), (C.c_double * 1)(1.0)
    dr[0].n_zz, dr[0].zz_i, dr[0].zz_j, dr[0].zz_w = 1, zi, zj, zw
    assert pkg.lib().sd_drive_check(m.h, dr, 1) == pkg._lib.SD_EARG
    zj[0] = 4
    assert pkg.lib().sd_drive_check(m.h, dr, 1) == pkg._lib.SD_OK
    assert pkg.lib().sd_drive_check(m.h, dr, -1) == pkg._lib.SD_EARG


def test_exports(pkg):
    for name in ("DiagonalDrive", "field_drive", "gradient_drive", "zz_drive", "diagonal_apply", "driven_apply", "magnus_schedule",
                 "piecewise_schedule", "stage_evolve", "driven_time_evolve", "diagonal_expectation", "instantaneous_energy", "drive_check"):
        assert hasattr(pkg, name) and name in pkg.__all__, name
    for name in ("sd_drive_check", "sd_diag_apply", "sd_diag_apply_dev", "sd_driven_apply", "sd_driven_apply_dev", "sd_driven_evolve",
                 "sd_driven_evolve_dev"):
        assert name in pkg.PROTOTYPES and hasattr(pkg.lib(), name), name
    # the structs as the header lays them out
    assert [f[0] for f in pkg._lib.sd_drive._fields_] == ["site_w", "n_zz", "zz_i", "zz_j", "zz_w"]
    assert C.sizeof(pkg._lib.sd_drive) == 40
    assert [f[0] for f in pkg._lib.sd_driven_info._fields_] == ["stages", "applies", "min_beta"] and C.sizeof(pkg._lib.sd_driven_info) == 24
    m = pkg.XXZChain(6, Jz=0.5, nup=3, ctx=None)
    g = pkg.gradient_drive(m)
    assert np.array_equal(g.site_weights, np.arange(1, 7) - 3.5) and g.bonds == []
    z = pkg.zz_drive(m)
    assert z.bonds == [(i, i + 1) for i in range(1, 6)] and np.array_equal(z.bond_weights, np.ones(5)) and z.site_weights is None
    assert np.array_equal(pkg.field_drive(m).site_weights, np.ones(6))
    tau, coef = pkg.piecewise_schedule([(0.5, [1.0, -1.0]), (0.25, [0.0, 2.0])])
    assert np.array_equal(tau, [0.5, 0.25]) and np.array_equal(coef, [[1.0, -1.0], [0.0, 2.0]])


def test_schedules_equal_the_restatement(pkg):
    fs = [lambda t: 0.8 * np.sin(3 * t), lambda t: 0.5 * t, 0.25]
    fr = fs[:2] + [lambda t: 0.25]
    for order in (2, 4):
        tau, coef = pkg.magnus_schedule(fs, 0.3, 0.07, 5, order=order)
        tr, cr = DR.magnus_schedule(fr, 0.3, 0.07, 5, order=order)
        assert tau.shape == tr.shape and coef.shape == cr.shape == (5 * order // 2, 3)
        assert np.abs(tau - tr).max() <= 1e-16 and np.abs(coef - cr).max() <= 1e-15


def test_order_of_the_schedules(pkg, D):
    """Errors against order 4 at 1600 steps, n = 10, 20, 40, 80 steps of the package's magnus_schedule through the dense stage
    propagator.  Measured with this psi0: order 4 1.6e-5, 9.7e-7, 6.0e-8, 3.8e-9 (ratios 16.18, 16.04, 16.01); order 2 6.5e-3,
    1.6e-3, 4.0e-4, 1.0e-4 (4.03, 4.01, 4.00); order 4 with the stages swapped 4.00 between 40 and 80 steps.
    Conditions: order 4 every ratio >= 12, order 2 every ratio in
    [3.5, 4.6]."""
    H0, diags, fs, psi0, T = problem(D)
    ref = DR.dense_stages(H0, diags, *pkg.magnus_schedule(fs, 0.0, T / 1600, 1600, order=4), psi0)
    errs = {}
    for order in (4, 2):
        errs[order] = []
        for n in (10, 20, 40, 80):
            tau, coef = pkg.magnus_schedule(fs, 0.0, T / n, n, order=order)
            assert abs(tau.sum() - T) <= 1e-14
            errs[order].append(np.linalg.norm(DR.dense_stages(H0, diags, tau, coef, psi0) - ref))
    r4 = [a / b for a, b in zip(errs[4][:-1], errs[4][1:])]
    r2 = [a / b for a, b in zip(errs[2][:-1], errs[2][1:])]
    print("order 4", errs[4], r4)
    print("order 2", errs[2], r2)
    assert all(r >= 12 for r in r4), (errs[4], r4)
    assert all(3.5 <= r <= 4.6 for r in r2), (errs[2], r2)
    # the negative control: the two stages of a step exchanged give a second-order method
    es = [np.linalg.norm(DR.dense_stages(H0, diags, *DR.magnus_schedule(fs, 0.0, T / n, n, swap=True), psi0) - ref) for n in (40, 80)]
    print("swapped", es, es[0] / es[1])
    assert es[0] / es[1] < 6
