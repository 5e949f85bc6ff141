"""sd_model_symmetric through the C ABI and its Python mirror is_symmetric, on models created without a context: which of T^r, R
and Z leave the hop, zz and field lists invariant, and the argument errors.  CPU only."""
import ctypes as C

import numpy as np
import pytest

REFLECT, FLIP = 256, 512
SD_EARG = 1


def raw(pkg, m, code):
    yes = C.c_int(-7)
    rc = pkg.lib().sd_model_symmetric(m.h, int(code), C.byref(yes))
    return rc, yes.value


def table(pkg, m):
    """(T, R, Z) with Z None where it is undefined"""
    z = pkg.is_symmetric(m, flip=True) if (m.nup is None or 2 * m.nup == m.L) else None
    return pkg.is_symmetric(m, shift=1), pkg.is_symmetric(m, reflect=True), z


def ring(L, J):
    return [(i, i % L + 1, J) for i in range(1, L + 1)]


@pytest.mark.parametrize("nup", [4, 3, None])
def test_xxz_ring(pkg, nup):
    L = 8
    m = pkg.XXZChain(L, Jxy=0.8, Jz=0.7, hz=0.0, nup=nup, boundary="periodic", ctx=None)
    assert table(pkg, m) == (True, True, None if nup == 3 else True)
    for r in range(L):                                   # every element of the dihedral group, with and without Z
        for refl in (False, True):
            assert pkg.is_symmetric(m, r, refl)
            assert raw(pkg, m, r | (REFLECT if refl else 0)) == (0, 1)
    h = pkg.XXZChain(L, Jxy=0.8, Jz=0.7, hz=0.3, nup=nup, boundary="periodic", ctx=None)
    assert table(pkg, h) == (True, True, None if nup == 3 else False)        # a uniform field breaks Z only


def test_open_chain(pkg):
    m = pkg.XXZChain(8, Jxy=0.8, Jz=0.7, nup=3, boundary="open", ctx=None)
    assert table(pkg, m) == (False, True, None)
    assert not any(pkg.is_symmetric(m, r) for r in range(1, 8)) and pkg.is_symmetric(m, 0)
    assert not pkg.is_symmetric(m, 1, True)              # the reflection about another centre is none of the open chain's


def test_j1j2_ring_with_uniform_field(pkg):
    L = 10
    hop = ring(L, 0.5) + [(i, (i + 1) % L + 1, 0.2) for i in range(1, L + 1)]
    zz = ring(L, 1.0) + [(i, (i + 1) % L + 1, 0.4) for i in range(1, L + 1)]
    m = pkg.build_model(L, nup=5, hopping=hop, zz=zz, onsite_field=np.full(L, 0.1), ctx=None)
    assert table(pkg, m) == (True, True, False)
    # a bond given twice, reversed, with a zero entry and a self-bond in between: the tables are summed per unordered pair
    hop2 = [(j, i, 0.25) for i, j, _ in ring(L, 0.5)] + [(3, 3, 9.0), (1, 5, 0.0)] + [(i, j, 0.25) for i, j, _ in ring(L, 0.5)]
    m2 = pkg.build_model(L, nup=5, hopping=hop2, zz=ring(L, 1.0), ctx=None)
    assert table(pkg, m2) == (True, True, True)
    # one second-neighbour bond missing: only the reflection through that bond's centre survives
    m3 = pkg.build_model(L, nup=5, hopping=hop[:-1], zz=zz, ctx=None)
    assert table(pkg, m3)[0] is False and pkg.is_symmetric(m3, flip=True)
    # hops invariant but the zz list not
    m4 = pkg.build_model(L, nup=5, hopping=ring(L, 0.5), zz=ring(L, 1.0)[:-1], ctx=None)
    assert table(pkg, m4) == (False, True, True)


def test_random_field(pkg):
    L = 8
    f = np.random.default_rng(3).standard_normal(L)
    m = pkg.build_model(L, nup=4, hopping=ring(L, 0.5), zz=ring(L, 1.0), onsite_field=f, ctx=None)
    assert table(pkg, m) == (False, False, False)
    stag = pkg.build_model(L, nup=4, hopping=ring(L, 0.5), zz=ring(L, 1.0), onsite_field=[0.2, -0.2] * 4, ctx=None)
    assert table(pkg, stag) == (False, False, False)     # R maps odd sites onto even ones for even L
    assert pkg.is_symmetric(stag, 2) and pkg.is_symmetric(stag, 1, True)


def test_small_rings(pkg):
    m2 = pkg.XXZChain(2, nup=1, boundary="periodic", ctx=None)       # one bond: T and R are the same exchange
    assert table(pkg, m2) == (True, True, True)
    m3 = pkg.XXZChain(3, nup=1, boundary="periodic", ctx=None)
    assert table(pkg, m3) == (True, True, None) and pkg.is_symmetric(m3, 2, True)
    o3 = pkg.XXZChain(3, nup=1, boundary="open", ctx=None)
    assert table(pkg, o3) == (False, True, None)
    full3 = pkg.XXZChain(3, boundary="periodic", ctx=None)
    assert table(pkg, full3) == (True, True, True)                   # Z is defined on the full basis for odd L too


def test_argument_errors(pkg):
    L = 8
    m = pkg.XXZChain(L, nup=3, boundary="periodic", ctx=None)
    half = pkg.XXZChain(L, nup=4, boundary="periodic", ctx=None)
    for bad in (L, 255, -1, 1 << 10, (1 << 10) | 1):
        assert raw(pkg, m, bad) == (SD_EARG, -7)                     # the result is left alone
    assert raw(pkg, m, FLIP) == (SD_EARG, -7)                        # Z outside a half-filled sector
    assert raw(pkg, half, FLIP | REFLECT | (L - 1)) == (0, 1)
    assert pkg.lib().sd_model_symmetric(None, 0, C.byref(C.c_int())) == SD_EARG
    assert pkg.lib().sd_model_symmetric(m.h, 0, None) == SD_EARG
    with pytest.raises(pkg.ArgumentError):
        pkg.is_symmetric(m, flip=True)
    assert pkg.is_symmetric(m, shift=-1) and pkg.is_symmetric(m, shift=L + 1)      # the mirror takes the shift mod L
