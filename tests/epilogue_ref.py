"""Plain numpy restatements of the fused apply epilogues (csrc/device_common.hpp, epilogue<1> and epilogue<2>): what is stored for
every row given h = H psi, own = psi, the side vectors and the scalars.  The yardstick of tests/test_gpu_apply_epilogues.py, proven
against exact rational arithmetic by tests/test_epilogue_ref_host.py.  Nothing here is shared with the library.

One numpy ufunc call is one correctly rounded IEEE operation per element, and numpy never contracts two of them, so every
expression below is written as the sequence of operations the header spells out (the library is built with -ffp-contract=off):
  rescale      (h - b*own) / a          a multiply, a subtract, a true division
  recurrence   2.0*x - prev             a multiply (exact) and a subtract
  accumulate   t.x += cr*o.x - ci*o.y ; t.y += cr*o.y + ci*o.x       (CHEB2: the c0 term with `own` first, then the c term with o)
  sums         RESCALE_DOT / KPM: ph.x*o.x + ph.y*o.y and o.x*o.x + o.y*o.y, ph = phi or (phi=None) own
               DOT:               own.x*o.x + own.y*o.y and own.x*o.y - own.y*o.x
Real vectors: the .x lines alone (a real coefficient, one sum for DOT).  `negate` applies to PLAIN and DOT.

Complex vectors are handled as two float64 arrays, never through numpy's complex arithmetic."""
import numpy as np

PLAIN, DOT, RESCALE, RESCALE_DOT, KPM, RECUR, CHEB2, CHEB = "PLAIN", "DOT", "RESCALE", "RESCALE_DOT", "KPM", "RECUR", "CHEB2", "CHEB"
EPILOGUES = (PLAIN, DOT, RESCALE, RESCALE_DOT, KPM, RECUR, CHEB2, CHEB)
WITH_SUMS = (DOT, RESCALE_DOT, KPM)
WITH_PREV = (KPM, RECUR, CHEB2, CHEB)
WITH_PSI_T = (CHEB2, CHEB)


def parts(v):
    """(re, im) of a complex vector as float64 arrays, (v, None) of a real one"""
    v = np.asarray(v)
    if np.iscomplexobj(v):
        return np.ascontiguousarray(v.real, dtype=np.float64), np.ascontiguousarray(v.imag, dtype=np.float64)
    return np.ascontiguousarray(v, dtype=np.float64), None


def join(x, y):
    if y is None:
        return x
    out = np.empty(len(x), dtype=np.complex128)
    out.real, out.imag = x, y
    return out


def epilogue(epi, h, own, a=1.0, b=0.0, c=0.0, c0=0.0, prev=None, phi=None, psi_t=None, negate=False):
    """-> (out, new psi_t or None, terms of sum 0 or None, terms of sum 1 or None); the terms are PER ROW, in row order.
    h and own decide the element type (both real or both complex); c and c0 are complex numbers (real vectors use their real
    parts, as the kernel does)."""
    assert epi in EPILOGUES
    hx, hy = parts(h)
    ox, oy = parts(own)
    cplx = hy is not None
    assert cplx == (oy is not None)
    a, b = np.float64(a), np.float64(b)
    cr, ci = np.float64(complex(c).real), np.float64(complex(c).imag)
    c0r, c0i = np.float64(complex(c0).real), np.float64(complex(c0).imag)
    comps = ((hx, ox), (hy, oy)) if cplx else ((hx, ox),)
    if epi in (PLAIN, DOT):
        o = [(-hh if negate else hh.copy()) for hh, _ in comps]
    else:
        o = [(hh - b * oo) / a for hh, oo in comps]
        if epi in WITH_PREV:
            pv = parts(prev)
            assert (pv[1] is not None) == cplx
            o = [np.float64(2.0) * x - p for x, p in zip(o, pv)]
    new_t = s0 = s1 = None
    if epi in WITH_PSI_T:
        t = [x.copy() for x in parts(psi_t) if x is not None]
        assert len(t) == len(o)
        if cplx:
            if epi == CHEB2:
                t[0] = t[0] + (c0r * ox - c0i * oy)
                t[1] = t[1] + (c0r * oy + c0i * ox)
            t[0] = t[0] + (cr * o[0] - ci * o[1])
            t[1] = t[1] + (cr * o[1] + ci * o[0])
        else:
            if epi == CHEB2:
                t[0] = t[0] + c0r * ox
            t[0] = t[0] + cr * o[0]
        new_t = join(t[0], t[1] if cplx else None)
    if epi == DOT:
        if cplx:
            s0 = ox * o[0] + oy * o[1]
            s1 = ox * o[1] - oy * o[0]
        else:
            s0 = ox * o[0]
    elif epi in (RESCALE_DOT, KPM):
        px, py = (ox, oy) if phi is None else parts(phi)
        if cplx:
            s0 = px * o[0] + py * o[1]
            s1 = o[0] * o[0] + o[1] * o[1]
        else:
            s0 = px * o[0]
            s1 = o[0] * o[0]
    return join(o[0], o[1] if cplx else None), new_t, s0, s1
