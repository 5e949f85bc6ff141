"""Host-side checks of the transverse structure factor: the numpy reference of S^-+_q (tests/transverse_ref.py) against a
Kronecker construction, and the new entry points' behaviour without a device."""
import ctypes as C

import numpy as np
import pytest

import transverse_ref as R


@pytest.mark.parametrize("op", ["minus", "plus"])
def test_reference_matches_dense_kronecker(D, op):
    L, nup = 8, 4
    rng = np.random.default_rng(4)
    src = R.sector_states(L, nup)
    dst = R.sector_states(L, nup + (-1 if op == "minus" else 1))
    psi = rng.standard_normal(len(src)) + 1j * rng.standard_normal(len(src))
    full = np.zeros(1 << L, complex)
    full[src] = psi
    one = D.SM if op == "minus" else D.SP
    for q in (0.0, 2 * np.pi * 3 / L, 2.1):
        Sq = sum(np.exp(1j * q * r) / np.sqrt(L) * D.site_op(one, r + 1, L) for r in range(L))
        want = (Sq @ full)[dst]
        assert np.abs(R.spm(L, nup, psi, q, op) - want).max() <= 1e-14
        # full basis: the same formula with row = configuration
        assert np.abs(R.spm(L, None, full, q, op) - Sq @ full).max() <= 1e-14
    # the dense basis order is the combinadic rank's
    assert np.array_equal(np.array(D.sector_states(L, nup), dtype=np.int64), src)


def test_new_entry_points_need_a_device(pkg):
    l = pkg.lib()
    if l.sd_device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.SpinDynError):
        pkg.kpm_sqw_transverse(np.ones(6), pkg.XXZChain(4, nup=2), [0.0], [0.0], a=4.0, b=0.0)
    with pytest.raises(pkg.SpinDynError):
        pkg.Sminus_q_vector(pkg.XXZChain(4, nup=2), np.ones(6), 0.0)
    # the C entry points refuse a null context
    d = np.zeros(4)
    dp = d.ctypes.data_as(C.POINTER(C.c_double))
    assert l.sd_spm_q(None, None, None, 2, 1, d.ctypes.data, 1, 0.0, d.ctypes.data, 1) == pkg._lib.SD_EARG
    assert l.sd_spm_q_dev(None, None, None, 1, 1, d.ctypes.data, 1, 0.0, d.ctypes.data, 1) == pkg._lib.SD_EARG
    assert l.sd_kpm_sqw_transverse(None, None, None, 2, 1, d.ctypes.data, 1, dp, 1, dp, 1, 1, 1.0, 0.0, 8, 0, 0, dp) == pkg._lib.SD_EARG
    assert l.sd_lanczos_sqw_transverse(None, None, None, 2, 1, d.ctypes.data, 1, dp, 1, dp, 1, 8, 0.05, 0, dp) == pkg._lib.SD_EARG


def test_unknown_component_is_an_argument_error(pkg):
    with pytest.raises(pkg.ArgumentError):
        pkg.dynamical_structure_factor(None, np.ones(4), [0.0], [0.0], component="yy")
    with pytest.raises(pkg.ArgumentError):
        pkg.kpm_sqw_transverse(np.ones(4), None, [0.0], [0.0], component="zz")
    with pytest.raises(pkg.ArgumentError):
        pkg.lanczos_sqw_transverse(np.ones(4), None, [0.0], [0.0], component="+")
