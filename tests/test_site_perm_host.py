"""The host side of the site permutations, no GPU: sd_site_permute_sources -- the byte table of csrc/site_perm.hpp, the
same code the kernel builds its LDS tables with, and the host rank of basis.cpp -- against the per-bit loops of tests/subsystem_ref.py
for EVERY row; sd_subsystem_permutation's layout and refusals; the compose / inverse helpers."""
import ctypes as C

import numpy as np
import pytest

import subsystem_ref as SR

_ip = C.POINTER(C.c_int)
_i64p = C.POINTER(C.c_int64)

# L = 17: a third table byte with one bit in use
SHAPES = [(10, 4), (12, 6), (17, 8), (9, None)]


def perms_of(L):
    rng = np.random.default_rng(20261020 + L)
    out = {"T": SR.translation(L), "R": SR.reflection(L), "identity": list(range(1, L + 1))}
    for k in range(10):
        out[f"random{k}"] = [int(x) for x in rng.permutation(L) + 1]
    out["middle block"] = SR.stable_partition(L, list(range(L // 2 - 1, L // 2 + 3)))
    out["two end blocks"] = SR.stable_partition(L, [1, 2, L - 1, L])
    out["every other site"] = SR.stable_partition(L, list(range(1, L + 1, 2)))
    return out


def sources(pkg, m, perm, start=0, count=None):
    count = m.N - start if count is None else count
    out = np.full(max(count, 0), -7, dtype=np.int64)
    p = np.ascontiguousarray(perm, dtype=np.intc)
    rc = pkg.lib().sd_site_permute_sources(m.h, p.ctypes.data_as(_ip), start, count, out.ctypes.data_as(_i64p))
    return rc, out


@pytest.mark.parametrize("L,nup", SHAPES)
def test_sources_equal_the_restatement_for_every_row(pkg, L, nup):
    m = pkg.XXZChain(L, nup=nup, ctx=None)
    for name, perm in perms_of(L).items():
        want = SR.source_rows(L, nup, perm)
        rc, got = sources(pkg, m, perm)
        assert rc == 0, name
        assert np.array_equal(got, want), name
        assert np.array_equal(np.sort(got), np.arange(m.N)), name                 # a permutation of the rows
        # a window of the rows is the same window
        rc, part = sources(pkg, m, perm, 5, 37)
        assert rc == 0 and np.array_equal(part, want[5:42]), name
    rc, ident = sources(pkg, m, list(range(1, L + 1)))
    assert np.array_equal(ident, np.arange(m.N))


def test_sources_refusals(pkg):
    E = pkg._lib
    L = 10
    m = pkg.XXZChain(L, nup=4, ctx=None)
    good = list(range(1, L + 1))
    for bad in ([1] * L, [0] + good[1:], good[:-1] + [L + 1], good[:-2] + [L, L], [-1] + good[1:]):
        assert sources(pkg, m, bad)[0] == E.SD_EARG
    assert sources(pkg, m, good, -1, 3)[0] == E.SD_EARG
    assert sources(pkg, m, good, 0, m.N + 1)[0] == E.SD_EARG
    assert sources(pkg, m, good, m.N, 1)[0] == E.SD_EARG
    assert sources(pkg, m, good, 3, -1)[0] == E.SD_EARG
    assert sources(pkg, m, good, m.N, 0)[0] == 0
    l = pkg.lib()
    p = np.ascontiguousarray(good, dtype=np.intc)
    out = np.zeros(4, dtype=np.int64)
    assert l.sd_site_permute_sources(None, p.ctypes.data_as(_ip), 0, 4, out.ctypes.data_as(_i64p)) == E.SD_EARG
    assert l.sd_site_permute_sources(m.h, None, 0, 4, out.ctypes.data_as(_i64p)) == E.SD_EARG
    assert l.sd_site_permute_sources(m.h, p.ctypes.data_as(_ip), 0, 4, None) == E.SD_EARG


def raw_subsystem_permutation(pkg, L, sites):
    s = np.ascontiguousarray(sites, dtype=np.intc)
    out = np.zeros(max(L, 1), dtype=np.intc)
    rc = pkg.lib().sd_subsystem_permutation(L, s.ctypes.data_as(_ip), len(s), out.ctypes.data_as(_ip))
    return rc, out[:L].tolist()


def test_subsystem_permutation_layout_and_refusals(pkg):
    E = pkg._lib
    for L, sites in ((6, [3, 4]), (6, [6, 2]), (5, [1, 2, 3]), (12, [12, 1, 7]), (9, [2, 4, 6, 8]), (8, [8, 7, 6, 5, 4, 3, 2]), (63, [63, 1])):
        rc, perm = raw_subsystem_permutation(pkg, L, sites)
        assert rc == 0 and perm == SR.stable_partition(L, sites)
        assert pkg.subsystem_permutation(L, sites).tolist() == perm
        assert [perm[s - 1] for s in sites] == list(range(1, len(sites) + 1))      # sites[j] -> j + 1, in the order given
        rest = [perm[i] for i in range(L) if i + 1 not in sites]
        assert rest == list(range(len(sites) + 1, L + 1))                          # the others keep their order
    assert pkg.subsystem_permutation(5, [1, 2, 3]).tolist() == [1, 2, 3, 4, 5]     # a prefix in order: the identity
    for L, sites in ((6, []), (6, [1, 2, 3, 4, 5, 6]), (6, [1, 1]), (6, [0]), (6, [7]), (6, [-2]), (1, [1]), (0, [1]), (64, [1])):
        assert raw_subsystem_permutation(pkg, L, sites)[0] == E.SD_EARG, (L, sites)
        with pytest.raises(pkg.ArgumentError):
            pkg.subsystem_permutation(L, sites)
    l = pkg.lib()
    one = np.ones(1, dtype=np.intc)
    out = np.zeros(6, dtype=np.intc)
    assert l.sd_subsystem_permutation(6, None, 1, out.ctypes.data_as(_ip)) == E.SD_EARG
    assert l.sd_subsystem_permutation(6, one.ctypes.data_as(_ip), 1, None) == E.SD_EARG
    with pytest.raises(pkg.ArgumentError):
        pkg.subsystem_permutation(6, [1.5])


def test_compose_and_inverse(pkg):
    rng = np.random.default_rng(9)
    L, nup = 9, 4
    psi = rng.standard_normal(len(SR.basis(L, nup)))
    for _ in range(5):
        p, q = [int(x) for x in rng.permutation(L) + 1], [int(x) for x in rng.permutation(L) + 1]
        pi, r = pkg.permutation_inverse(p), pkg.permutation_compose(p, q)
        ident = list(range(1, L + 1))
        assert pkg.permutation_compose(p, pi).tolist() == ident and pkg.permutation_compose(pi, p).tolist() == ident
        assert pkg.permutation_inverse(pi).tolist() == p
        assert pkg.permutation_inverse(r).tolist() == pkg.permutation_compose(pkg.permutation_inverse(q), pi).tolist()
        # U_r = U_p U_q, q acting first; U_{p^-1} U_p = 1
        assert np.array_equal(SR.permute(psi, L, nup, r.tolist()), SR.permute(SR.permute(psi, L, nup, q), L, nup, p))
        assert np.array_equal(SR.permute(SR.permute(psi, L, nup, p), L, nup, pi.tolist()), psi)
    T = SR.translation(L)
    assert pkg.permutation_compose(T, T).tolist() == [(i + 2) % L + 1 for i in range(L)]
    assert pkg.permutation_inverse(SR.reflection(L)).tolist() == SR.reflection(L)
    for bad in ([1, 1, 2], [0, 1, 2], [], [2, 3, 4]):
        with pytest.raises(pkg.ArgumentError):
            pkg.permutation_inverse(bad)
    with pytest.raises(pkg.ArgumentError):
        pkg.permutation_compose([1, 2, 3], [1, 2])
