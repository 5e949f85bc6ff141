"""Host-only entry points of the S^z-basis statistics: the uniforms of the projective snapshots, bit for bit against a
numpy uint64 restatement of the hash, and the reachable range of a subsystem's counting statistics against brute force over the
basis.  No device compute is called here."""
import ctypes as C
import itertools

import numpy as np
import pytest

import basis_stats_ref as BR

_dp = C.POINTER(C.c_double)
NEW = ["sd_basis_moments", "sd_basis_moments_dev", "sd_counting_range", "sd_counting_statistics", "sd_counting_statistics_dev",
       "sd_sample_uniforms_host", "sd_sample_configurations", "sd_sample_configurations_dev"]


def test_new_names_are_in_the_prototype_table(pkg):
    for name in NEW:
        assert name in pkg.PROTOTYPES, name
        assert hasattr(pkg.lib(), name)
    for name in ("participation_entropy", "inverse_participation_ratio", "most_probable_configuration", "counting_statistics",
                 "cut_counting_statistics", "number_entropy", "magnetization_cumulants", "sample_configurations", "snapshot_spins"):
        assert callable(getattr(pkg, name))


@pytest.mark.parametrize("seed", [0, 1, 20260821, 2 ** 63 + 12345, 2 ** 64 - 1])
def test_sample_uniforms_bit_for_bit(pkg, seed):
    for first, n in ((0, 1), (0, 4097), (1000, 257), (2 ** 32 - 3, 100), (2 ** 63, 5)):
        u = np.full(n, np.nan)
        assert pkg.lib().sd_sample_uniforms_host(seed, first, n, u.ctypes.data_as(_dp)) == 0
        want = BR.uniforms(seed, first, n)
        assert np.array_equal(u.view(np.uint64), want.view(np.uint64)), (seed, first, n)
        assert (u >= 0.0).all() and (u < 1.0).all()
    # keyed by the shot number: a later window of the same stream
    a, b = np.empty(3000), np.empty(100)
    assert pkg.lib().sd_sample_uniforms_host(seed, 0, 3000, a.ctypes.data_as(_dp)) == 0
    assert pkg.lib().sd_sample_uniforms_host(seed, 2900, 100, b.ctypes.data_as(_dp)) == 0
    assert np.array_equal(a[2900:], b)
    assert 0.45 < a.mean() < 0.55 and len(np.unique(a)) == 3000
    assert pkg.lib().sd_sample_uniforms_host(seed, 0, -1, a.ctypes.data_as(_dp)) == pkg._lib.SD_EARG
    assert pkg.lib().sd_sample_uniforms_host(seed, 0, 1, None) == pkg._lib.SD_EARG


def test_sample_stream_is_not_the_normal_stream(pkg):
    """the salt: the uniforms of seed s are not the first uniforms the normal stream of seed s hashes"""
    u = BR.uniforms(7, 0, 64)
    with np.errstate(over="ignore"):
        plain = (BR._mix(np.uint64(7) ^ BR._mix(np.arange(64, dtype=np.uint64))) >> np.uint64(11)).astype(np.float64) / 2.0 ** 53
    assert not np.intersect1d(u, plain).size


def counting_range(pkg, m, mask):
    lo, nb = C.c_int(-7), C.c_int(-7)
    rc = pkg.lib().sd_counting_range(m.h, mask, C.byref(lo), C.byref(nb))
    return rc, lo.value, nb.value


@pytest.mark.parametrize("L,nup", [(6, 3), (9, 2), (9, 7)])
def test_counting_range_in_a_sector_by_brute_force(pkg, L, nup):
    m = pkg.XXZChain(L, nup=nup, ctx=None)
    states = [sum(1 << i for i in c) for c in itertools.combinations(range(L), nup)]
    assert len(states) == m.N
    for mask in range(1 << L):
        seen = {bin(s & mask).count("1") for s in states}
        rc, lo, nb = counting_range(pkg, m, mask)
        assert rc == 0 and lo == min(seen) and nb == len(seen) and seen == set(range(lo, lo + nb)), (mask, lo, nb, seen)
        assert BR.reachable(L, nup, mask) == (lo, lo + nb - 1)


def test_counting_range_in_the_full_basis_by_brute_force(pkg):
    L = 6
    m = pkg.XXZChain(L, nup=None, ctx=None)
    for mask in range(1 << L):
        seen = {bin(s & mask).count("1") for s in range(1 << L)}
        rc, lo, nb = counting_range(pkg, m, mask)
        assert rc == 0 and lo == 0 and nb == len(seen) and seen == set(range(nb))
    E = pkg._lib
    assert counting_range(pkg, m, 1 << L)[0] == E.SD_EARG and counting_range(pkg, m, (1 << 63) | 1)[0] == E.SD_EARG
    assert pkg.lib().sd_counting_range(None, 1, C.byref(C.c_int()), C.byref(C.c_int())) == E.SD_EARG
    assert pkg.lib().sd_counting_range(m.h, 1, None, C.byref(C.c_int())) == E.SD_EARG
    # a subsystem of 33 sites of a full basis has 34 values: the range says so, the device call refuses it
    big = pkg.XXZChain(40, nup=None, ctx=None)
    assert counting_range(pkg, big, (1 << 33) - 1) == (0, 0, 34)


def test_magnetization_cumulants_and_snapshot_spins(pkg):
    """host arithmetic: a binomial distribution of n fair spins has cumulants 0, n/4, 0, -n/8 of sum S^z"""
    from math import comb
    n = 10
    P = np.zeros(17)
    P[:n + 1] = [comb(n, k) for k in range(n + 1)]
    k = pkg.magnetization_cumulants(P, list(range(1, n + 1)), order=4)
    assert np.abs(k - np.array([0.0, n / 4, 0.0, -n / 8])).max() <= 1e-12
    assert np.abs(pkg.magnetization_cumulants(P / 7.0, n, order=2) - np.array([0.0, n / 4])).max() <= 1e-12
    onehot = np.zeros(5)
    onehot[3] = 2.0
    assert np.array_equal(pkg.magnetization_cumulants(onehot, 4, order=3), np.array([1.0, 0.0, 0.0]))
    sp = pkg.snapshot_spins(np.array([0b0101, 0b1000], dtype=np.uint64), 4)
    assert np.array_equal(sp, np.array([[0.5, -0.5, 0.5, -0.5], [-0.5, -0.5, -0.5, 0.5]]))
    with pytest.raises(pkg.ArgumentError):
        pkg.magnetization_cumulants(np.zeros(4), 3)
