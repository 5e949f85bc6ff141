"""sd_energy_current_terms (host only, models created without a context) against the builder of tests/ecurrent_ref.py: the same
(i, j, k) list in the same order, coefficients within 1e-15 max|c|, the term counts of DESIGN.md 17, and the refusals.

The minimum image of a bond is needed only where the bond enters a contributing pair: the two-site "ring" (one bond, delta = 1 =
L/2) therefore has an empty list at zero field -- nothing shares a site with the bond -- and is refused with a field, whose k = 0
term needs delta.  Both builders must agree on that."""
import ctypes as C

import numpy as np
import pytest

import ecurrent_ref as ER
from test_ecurrent_ref_host import j1j2, xxz


def all_to_all(L):
    hop = [(i, j, 1.0 / (j - i)) for i in range(1, L + 1) for j in range(i + 1, L + 1)]
    zz = [(i, j, 0.7 / (j - i) ** 2) for i, j, _ in hop]
    return hop, zz, np.linspace(0.1, 0.5, L)


def host_model(pkg, L, lists, nup=None):
    hop, zz, field = lists
    return pkg.build_model(L, nup=min(2, L) if nup is None else nup, hopping=hop, zz=zz, onsite_field=field, ctx=None)


def compare(pkg, L, lists, boundary):
    m = host_model(pkg, L, lists)
    got = pkg.energy_current_terms(m, boundary)
    ref = ER.energy_current_terms(L, *lists, periodic=boundary == "periodic")
    assert got.dtype == ER.DTERM
    assert [tuple(int(x) for x in (t["i"], t["j"], t["k"])) for t in got] == [tuple(int(x) for x in (t["i"], t["j"], t["k"])) for t in ref]
    if len(ref):
        assert np.abs(got["c"] - ref["c"]).max() <= 1e-15 * np.abs(ref["c"]).max()
    return got


@pytest.mark.parametrize("hz", [0.0, 0.3])
@pytest.mark.parametrize("L", [2, 3, 8, 25])
@pytest.mark.parametrize("boundary", ["open", "periodic"])
def test_xxz_lists(pkg, boundary, L, hz):
    lists = xxz(L, boundary, hz=hz)
    if boundary == "periodic" and L == 2 and hz != 0.0:      # delta = L/2 and the field term needs it: both refuse
        with pytest.raises(ER.Ambiguous):
            ER.energy_current_terms(L, *lists, periodic=True)
        with pytest.raises(pkg.ArgumentError):
            pkg.energy_current_terms(host_model(pkg, L, lists), "periodic")
        return
    got = compare(pkg, L, lists, boundary)
    if boundary == "periodic" and L >= 8:
        assert len(got) == (4 * L if hz else 3 * L)
    if L == 2:
        assert len(got) == (1 if hz else 0)


def test_j1j2_ring_and_all_to_all(pkg):
    got = compare(pkg, 39, j1j2(39), "periodic")
    assert len(got) == 546 and len(ER.groups(got)) == 156
    compare(pkg, 12, all_to_all(12), "open")
    assert len(pkg.energy_current_terms(host_model(pkg, 20, all_to_all(20)), "open")) == 3610


def test_refusals(pkg):
    lib, EARG = pkg.lib(), pkg._lib.SD_EARG
    n = C.c_int(-1)
    # the +-L/2 ambiguity: a ring of 8 with the bond (1, 5) next to a nearest-neighbour bond
    m = host_model(pkg, 8, ([(1, 5, 0.5), (5, 6, 0.5)], [], np.zeros(8)))
    assert lib.sd_energy_current_terms(m.h, 1, None, 0, C.byref(n)) == EARG
    assert lib.sd_energy_current_terms(m.h, 0, None, 0, C.byref(n)) == 0 and n.value == 1
    with pytest.raises(pkg.ArgumentError):
        pkg.energy_current_terms(m, "periodic")
    # more than 4096 terms
    m = host_model(pkg, 24, all_to_all(24))
    assert lib.sd_energy_current_terms(m.h, 0, None, 0, C.byref(n)) == EARG
    # a cap that is too small; the count comes back all the same
    m = host_model(pkg, 8, xxz(8, "periodic"))
    buf = np.zeros(32, dtype=ER.DTERM)
    assert lib.sd_energy_current_terms(m.h, 1, buf.ctypes.data, 31, C.byref(n)) == EARG and n.value == 32
    assert lib.sd_energy_current_terms(m.h, 1, buf.ctypes.data, 32, C.byref(n)) == 0 and n.value == 32
    assert lib.sd_energy_current_terms(m.h, 2, None, 0, C.byref(n)) == EARG
    with pytest.raises(pkg.ArgumentError):
        pkg.energy_current_terms(m, "ring")
