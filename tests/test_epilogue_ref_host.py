"""The yardstick of tests/test_gpu_apply_epilogues.py, proven without a GPU: every operation of tests/epilogue_ref.py against exact
rational arithmetic rounded once (fractions.Fraction is exact, float(Fraction) is correctly rounded), element by element, for the
eight epilogues in both element types; and CHEB2 against a deferred c0 accumulation followed by one CHEB, bit for bit."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import epilogue_ref as ER

N = 300
A, B, C1, C0 = 4.3, -0.7, 0.3 - 0.2j, -0.11 + 0.23j


def mul(x, y):
    return float(Fr(x) * Fr(y))


def add(x, y):
    return float(Fr(x) + Fr(y))


def sub(x, y):
    return float(Fr(x) - Fr(y))


def div(x, y):
    return float(Fr(x) / Fr(y))


def vectors(cplx, seed):
    rng = np.random.default_rng(seed)

    def one():
        v = rng.standard_normal(N) * 10.0 ** rng.integers(-3, 4, N)       # a spread of exponents: roundings of every size
        v[:4] = [0.0, 1.0, -2.5, 3.0]                                     # ... and a few exact cases
        return v + 1j * (rng.standard_normal(N) * 10.0 ** rng.integers(-3, 4, N)) if cplx else v
    return {k: one() for k in ("h", "own", "prev", "phi", "psi_t")}


def comp(v, i):
    """the components of element i: (x, y) of a complex vector, (x,) of a real one"""
    return (float(v[i].real), float(v[i].imag)) if np.iscomplexobj(v) else (float(v[i]),)


def scalar_epilogue(epi, i, v, phi, negate):
    """element i by rational arithmetic rounded after every operation, in the order of csrc/device_common.hpp:
    -> (out components, psi_t components or None, (term 0, term 1))"""
    h, own = comp(v["h"], i), comp(v["own"], i)
    cplx = len(h) == 2
    if epi in (ER.PLAIN, ER.DOT):
        o = tuple(-x if negate else x for x in h)
    else:
        o = tuple(div(sub(hh, mul(B, oo)), A) for hh, oo in zip(h, own))
        if epi in ER.WITH_PREV:
            o = tuple(sub(mul(2.0, x), p) for x, p in zip(o, comp(v["prev"], i)))
    t = None
    if epi in ER.WITH_PSI_T:
        t = list(comp(v["psi_t"], i))
        terms = ([(C0, own)] if epi == ER.CHEB2 else []) + [(C1, o)]
        for cc, x in terms:
            if cplx:
                t[0] = add(t[0], sub(mul(cc.real, x[0]), mul(cc.imag, x[1])))
                t[1] = add(t[1], add(mul(cc.real, x[1]), mul(cc.imag, x[0])))
            else:
                t[0] = add(t[0], mul(cc.real, x[0]))
    s = (None, None)
    if epi == ER.DOT:
        s = (add(mul(own[0], o[0]), mul(own[1], o[1])), sub(mul(own[0], o[1]), mul(own[1], o[0]))) if cplx else (mul(own[0], o[0]), None)
    elif epi in (ER.RESCALE_DOT, ER.KPM):
        ph = own if phi is None else comp(phi, i)
        s = (add(mul(ph[0], o[0]), mul(ph[1], o[1])), add(mul(o[0], o[0]), mul(o[1], o[1]))) if cplx else (mul(ph[0], o[0]), mul(o[0], o[0]))
    return o, t, s


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("epi", ER.EPILOGUES)
def test_every_operation_is_the_exact_result_rounded_once(epi, cplx):
    v = vectors(cplx, 7 + ER.EPILOGUES.index(epi))
    frozen = {k: x.copy() for k, x in v.items()}
    cases = [(v["phi"], False)]
    if epi in (ER.RESCALE_DOT, ER.KPM):
        cases.append((None, False))                                       # phi = None: ph = own
    if epi in (ER.PLAIN, ER.DOT):
        cases.append((v["phi"], True))                                    # negate
    for phi, negate in cases:
        out, new_t, s0, s1 = ER.epilogue(epi, v["h"], v["own"], a=A, b=B, c=C1, c0=C0, prev=v["prev"], phi=phi, psi_t=v["psi_t"],
                                         negate=negate)
        assert out.dtype == (np.complex128 if cplx else np.float64) and out.shape == (N,)
        assert (new_t is not None) == (epi in ER.WITH_PSI_T) and (s0 is not None) == (epi in ER.WITH_SUMS)
        assert (s1 is not None) == (epi in (ER.RESCALE_DOT, ER.KPM) or (epi == ER.DOT and cplx))
        for i in range(N):
            o, t, s = scalar_epilogue(epi, i, v, phi, negate)
            assert comp(out, i) == o, (epi, cplx, i)
            if t is not None:
                assert comp(new_t, i) == tuple(t), (epi, cplx, i)
            if s[0] is not None:
                assert float(s0[i]) == s[0], (epi, cplx, i)
            if s[1] is not None:
                assert float(s1[i]) == s[1], (epi, cplx, i)
        for k in v:                                                       # the inputs are the caller's: untouched
            assert np.array_equal(v[k], frozen[k])
    if epi not in (ER.PLAIN, ER.DOT):                                     # a comparison of rounded results, not of copies
        assert not np.array_equal(out, v["h"])


def test_negate_leaves_the_other_epilogues_alone():
    v = vectors(True, 3)
    for epi in (ER.RESCALE, ER.RECUR, ER.KPM):
        x = ER.epilogue(epi, v["h"], v["own"], a=A, b=B, prev=v["prev"], phi=v["phi"], negate=True)
        y = ER.epilogue(epi, v["h"], v["own"], a=A, b=B, prev=v["prev"], phi=v["phi"], negate=False)
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[2], y[2])


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
def test_cheb2_is_a_deferred_c0_accumulation_followed_by_one_cheb(cplx):
    v = vectors(cplx, 11)
    out2, t2, _, _ = ER.epilogue(ER.CHEB2, v["h"], v["own"], a=A, b=B, c=C1, c0=C0, prev=v["prev"], psi_t=v["psi_t"])
    # the deferred term of the pass before: psi_t += c0 * own, component-wise
    tx, ty = ER.parts(v["psi_t"])
    ox, oy = ER.parts(v["own"])
    if cplx:
        t_def = ER.join(tx + (C0.real * ox - C0.imag * oy), ty + (C0.real * oy + C0.imag * ox))
    else:
        t_def = tx + C0.real * ox
    out1, t1, _, _ = ER.epilogue(ER.CHEB, v["h"], v["own"], a=A, b=B, c=C1, prev=v["prev"], psi_t=t_def)
    assert np.array_equal(out1, out2) and np.array_equal(t1, t2)
    assert not np.array_equal(t2, v["psi_t"])
