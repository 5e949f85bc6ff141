"""sd_opstring_check and sd_hamiltonian_terms (host only, models created without a context) against the builders of
tests/opstring_ref.py: the same terms in the same order, the operator count, the Hermiticity flag and every refusal.  Also the
Python builders of the package (op_string, operator_adjoint, ...) against the restatement's.  CPU only."""
import ctypes as C

import numpy as np
import pytest

import opstring_ref as OR
from test_ecurrent_ref_host import j1j2, xxz


def host_model(pkg, L, lists, nup):
    hop, zz, field = lists
    return pkg.build_model(L, nup=nup, hopping=hop, zz=zz, onsite_field=field, ctx=None)


def as_tuples(pkg, terms):
    return [(int(t.plus), int(t.minus), int(t.z), complex(t.c), int(t.op)) for t in terms]


def check(pkg, m, terms):
    tl = pkg.pack_terms(terms)
    k, h = C.c_int(-7), C.c_int(-7)
    rc = pkg.lib().sd_opstring_check(m.h, tl.ctypes.data, len(tl), C.byref(k), C.byref(h))
    return rc, k.value, h.value


@pytest.mark.parametrize("name,L,nup,lists", [
    ("xxz-open", 8, 4, xxz(8, "open")), ("xxz-periodic", 8, 3, xxz(8, "periodic")), ("xxz-field-full", 7, None, xxz(7, "periodic", hz=0.3)),
    ("j1j2-field", 10, 5, j1j2(10)), ("L2", 2, 1, xxz(2, "open", hz=0.5)), ("L3", 3, 1, xxz(3, "periodic")), ("L3-full", 3, None, xxz(3, "open", hz=-1.0)),
])
def test_hamiltonian_terms_match_the_restatement(pkg, name, L, nup, lists):
    hop, zz, field = lists
    m = host_model(pkg, L, lists, nup)
    got = as_tuples(pkg, pkg.hamiltonian_terms(m))
    want = OR.hamiltonian_terms(hop, zz, field)
    assert got == want                                        # the same terms, coefficients bit for bit, in list order
    n_hop = sum(1 for i, j, _t in hop if i != j)
    assert len(got) == 2 * n_hop + len(zz) + L
    rc, k, h = check(pkg, m, pkg.hamiltonian_terms(m))
    assert (rc, k, h) == (0, 1, 1)                            # one operator, Hermitian
    # cap = 0 sets the count alone; a short cap is refused and still reports it
    lib, n = pkg.lib(), C.c_int(-1)
    assert lib.sd_hamiltonian_terms(m.h, None, 0, C.byref(n)) == 0 and n.value == len(want)
    buf = np.zeros(len(want), dtype=pkg.operators.OPTERM)
    n = C.c_int(-1)
    assert lib.sd_hamiltonian_terms(m.h, buf.ctypes.data, len(want) - 1, C.byref(n)) == pkg._lib.SD_EARG and n.value == len(want)
    assert lib.sd_hamiltonian_terms(m.h, buf.ctypes.data, len(want), C.byref(n)) == 0
    assert lib.sd_hamiltonian_terms(m.h, None, 3, C.byref(n)) == pkg._lib.SD_EARG
    assert lib.sd_hamiltonian_terms(m.h, None, -1, C.byref(n)) == pkg._lib.SD_EARG


def test_self_bonds_of_the_lists(pkg):
    """a hop (i, i) never flips and gives no term; a zz term (i, i) is (S^z_i)^2 = 1/4"""
    lists = ([(1, 2, 0.5), (3, 3, 9.0)], [(2, 2, 0.8), (1, 3, -0.2)], np.array([0.0, 0.1, 0.0]))
    m = host_model(pkg, 3, lists, None)
    assert as_tuples(pkg, pkg.hamiltonian_terms(m)) == OR.hamiltonian_terms(*lists)
    assert (0, 0, 0, complex(0.25 * 0.8), 0) in as_tuples(pkg, pkg.hamiltonian_terms(m))


def test_hermiticity_flag(pkg):
    m = host_model(pkg, 6, xxz(6, "periodic"), 3)
    hop = pkg.op_string(0.7, ("+", 2), ("-", 5))
    assert check(pkg, m, hop) == (0, 1, 0)                                     # a lone S^+_i S^-_j
    assert check(pkg, m, hop + pkg.operator_adjoint(hop)) == (0, 1, 1)
    D = 0.37
    dm = pkg.op_string(0.5j * D, ("+", 1), ("-", 2)) + pkg.op_string(-0.5j * D, ("-", 1), ("+", 2))      # i D (S^+S^- - S^-S^+)/2
    assert check(pkg, m, dm) == (0, 1, 1)
    assert check(pkg, m, pkg.op_string(0.5j * D, ("+", 1), ("-", 2)) + pkg.op_string(0.5j * D, ("-", 1), ("+", 2))) == (0, 1, 0)
    # coefficients of equal (P, M, Z) are summed first: two halves of a Hermitian pair
    split = pkg.op_string(0.25, ("+", 1), ("-", 3)) + pkg.op_string(0.5, ("-", 1), ("+", 3)) + pkg.op_string(0.25, ("+", 1), ("-", 3))
    assert check(pkg, m, split) == (0, 1, 1)
    # per operator: op 1 Hermitian, op 3 not -> 0; K = 1 + max op, unused indices in between are allowed
    two = pkg.op_string(1.0, ("z", 1), ("z", 2), op=1) + pkg.op_string(1.0, ("+", 1), ("-", 2), op=3)
    assert check(pkg, m, two) == (0, 4, 0)
    assert check(pkg, m, pkg.op_string(1.0, ("z", 1), ("z", 2), op=1) + pkg.op_string(2.0, ("z", 4), op=3)) == (0, 4, 1)
    assert check(pkg, m, []) == (0, 0, 1)
    # a diagonal string is Hermitian only with a real coefficient
    assert check(pkg, m, pkg.op_string(1j, ("z", 1)))[2] == 0
    assert pkg.operator_check(m, dm) == (1, True)
    # the Python rule agrees
    for tl in (hop, dm, split, two):
        assert pkg.operator_is_hermitian(tl) == bool(check(pkg, m, tl)[2]) == OR.is_hermitian(as_tuples(pkg, tl))


def test_every_refusal_of_the_check(pkg):
    EARG = pkg._lib.SD_EARG
    T = pkg.Term
    sector = host_model(pkg, 6, xxz(6, "open"), 3)
    full = host_model(pkg, 6, xxz(6, "open"), None)
    ok = [T(1, 2, 4, 1.0 + 0j, 0)]
    assert check(pkg, sector, ok)[0] == 0
    bad = {
        "plus and minus overlap": [T(3, 2, 0, 1.0 + 0j, 0)],
        "plus and z overlap": [T(1, 2, 1, 1.0 + 0j, 0)],
        "minus and z overlap": [T(1, 2, 6, 1.0 + 0j, 0)],
        "a bit at L": [T(1, 1 << 6, 0, 1.0 + 0j, 0)],
        "a z bit far above L": [T(0, 0, 1 << 63, 1.0 + 0j, 0)],
        "non-finite real part": [T(1, 2, 0, complex(np.inf, 0.0), 0)],
        "non-finite imaginary part": [T(1, 2, 0, complex(0.0, np.nan), 0)],
        "negative op": [T(1, 2, 0, 1.0 + 0j, -1)],
        "op at the limit": [T(1, 2, 0, 1.0 + 0j, 256)],
    }
    for why, tl in bad.items():
        for m in (sector, full):
            assert check(pkg, m, ok + tl)[0] == EARG, why
            with pytest.raises(pkg.ArgumentError):
                pkg.operator_check(m, ok + tl)
    assert check(pkg, sector, [T(0, 0, 7, 1.0 + 0j, 255)]) == (0, 256, 1)
    # |P| != |M|: refused in a sector, allowed on the full basis
    for tl in ([T(1, 0, 0, 1.0 + 0j, 0)], [T(3, 4, 0, 1.0 + 0j, 0)], pkg.op_string(1.0, ("x", 2))):
        assert check(pkg, sector, tl)[0] == EARG
        assert check(pkg, full, tl)[0] == 0
    # the number of terms
    lib, k, h = pkg.lib(), C.c_int(), C.c_int()
    many = pkg.pack_terms([T(0, 0, 1, 1.0 + 0j, 0)] * 4097)
    assert lib.sd_opstring_check(full.h, many.ctypes.data, 4097, C.byref(k), C.byref(h)) == EARG
    assert lib.sd_opstring_check(full.h, many.ctypes.data, 4096, C.byref(k), C.byref(h)) == 0 and k.value == 1
    assert lib.sd_opstring_check(full.h, many.ctypes.data, -1, C.byref(k), C.byref(h)) == EARG
    assert lib.sd_opstring_check(full.h, None, 2, C.byref(k), C.byref(h)) == EARG
    assert lib.sd_opstring_check(full.h, None, 0, C.byref(k), C.byref(h)) == 0 and k.value == 0
    assert lib.sd_opstring_check(None, many.ctypes.data, 1, C.byref(k), C.byref(h)) == EARG
    assert lib.sd_opstring_check(full.h, many.ctypes.data, 1, None, C.byref(h)) == EARG


def test_python_builders_match_the_restatement(pkg):
    rng = np.random.default_rng(4)
    for _ in range(30):
        k = int(rng.integers(1, 7))
        sites = [int(s) for s in rng.choice(np.arange(1, 13), size=k, replace=False)]
        f = [(str(rng.choice(["+", "-", "z", "x", "y"])), s) for s in sites]
        c = complex(rng.standard_normal(), rng.standard_normal())
        got = as_tuples(pkg, pkg.op_string(c, *f, op=3))
        want = OR.expand(c, f, op=3)
        assert [t[:3] + t[4:] for t in got] == [t[:3] + t[4:] for t in want]
        assert got == want                                    # halving and multiplying by +-i are exact
        assert as_tuples(pkg, pkg.operator_adjoint(pkg.op_string(c, *f))) == OR.adjoint(OR.expand(c, f))
        assert as_tuples(pkg, pkg.operator_simplify(pkg.op_string(c, *f) * 2)) == OR.simplify(OR.expand(c, f) * 2)
    assert len(pkg.op_string(1.0, ("x", 1), ("y", 2), ("x", 3), ("z", 4))) == 8
    with pytest.raises(pkg.ArgumentError):
        pkg.op_string(1.0, ("z", 2), ("+", 2))
    with pytest.raises(pkg.ArgumentError):
        pkg.op_string(1.0, ("w", 2))
    with pytest.raises(pkg.ArgumentError):
        pkg.op_string(1.0, ("z", 0))
    assert as_tuples(pkg, pkg.chirality_terms(2, 5, 3, coeff=0.7)) == OR.chirality(2, 5, 3, coeff=0.7)
    assert as_tuples(pkg, pkg.string_order_terms(2, 6)) == OR.string_order(2, 6)
    # the packed array round-trips
    tl = pkg.chirality_terms(1, 2, 3) + pkg.op_string(2.0 - 1j, ("z", 60), op=7)
    arr = pkg.pack_terms(tl)
    assert arr.dtype.itemsize == 48 and as_tuples(pkg, pkg.operators._as_terms(arr)) == as_tuples(pkg, tl)
    with pytest.raises(pkg.ArgumentError):
        pkg.chirality_correlations(np.zeros(4), None, [(1, 2, 3), (3, 4, 5)])
