"""Plain restatements of the lattice symmetry operators.  They share nothing with the library.

Site i is bit i - 1 of a configuration; L-bit words.  T moves the spin of site i to site i + 1 (mod L): a rotation to the left by
one bit.  R exchanges site i with site L + 1 - i: bit reversal.  Z flips every spin.  A group element is g = (r, refl, flip),
U_g = T^r R^refl Z^flip, U_g |s> = |T^r R^refl Z^flip s>, hence (U_g psi)[idx(s)] = psi[idx(Z^flip R^refl T^-r s)].  Rows are ordered
as tests/rows_ref.py states (proven there): combinadic in a sector, the configuration itself in the full basis (nup None).

numpy functions work on uint64 configurations, the `*_t` functions are their torch ports on int64 tensors of any device (L <= 62).
tests/test_symmetry_ref_host.py proves them against Kronecker-product operators."""
import functools
import math

import numpy as np

import rows_ref as RR


# ---- the three transforms on configurations: numpy -------------------------------------------------------------------------
def rot_right(s, L, r):
    """T^-r s: the low r bits go to the top (no intermediate exceeds L bits)"""
    r %= L
    if r == 0:
        return s.copy()
    lo = s & np.uint64((1 << r) - 1)
    return (s >> np.uint64(r)) | (lo << np.uint64(L - r))


def T(s, L, r=1):
    """T^r s"""
    return rot_right(s, L, (-r) % L)


def R(s, L):
    out = np.zeros_like(s)
    for b in range(L):
        out |= ((s >> np.uint64(b)) & np.uint64(1)) << np.uint64(L - 1 - b)
    return out


def Z(s, L):
    return s ^ np.uint64((1 << L) - 1)


def transform(s, L, g):
    """T^r R^refl Z^flip s: where U_g sends the configuration s"""
    r, refl, flip = g
    if flip:
        s = Z(s, L)
    if refl:
        s = R(s, L)
    return T(s, L, r)


def source(s, L, g):
    """Z^flip R^refl T^-r s: the configuration whose amplitude row s of U_g psi receives"""
    r, refl, flip = g
    s = rot_right(s, L, r)
    if refl:
        s = R(s, L)
    if flip:
        s = Z(s, L)
    return s


def configurations(L, nup):
    N = (1 << L) if nup is None else math.comb(L, nup)
    rows = np.arange(N, dtype=np.int64)
    return rows.astype(np.uint64) if nup is None else RR.unrank(rows, L, nup)


def rows_of(s, L, nup):
    return s.astype(np.int64) if nup is None else RR.rank(s, L, nup)


def flip_defined(L, nup):
    return nup is None or 2 * nup == L


@functools.lru_cache(maxsize=256)
def _source_rows(L, nup, g):
    out = rows_of(source(configurations(L, nup), L, g), L, nup)
    out.setflags(write=False)
    return out


def source_rows(L, nup, g):
    """row -> the row U_g psi takes its value from (kept per (L, nup, g); read-only)"""
    assert not g[2] or flip_defined(L, nup)
    return _source_rows(L, nup, (int(g[0]) % L, int(bool(g[1])), int(bool(g[2]))))


def apply(psi, L, nup, g):
    return psi[source_rows(L, nup, g)]


def overlaps(bra, ket, L, nup, elements):
    """<bra|U_g|ket> for every element"""
    return np.array([np.vdot(bra, apply(ket, L, nup, g)) for g in elements])


def combine(psi, L, nup, elements, coef):
    """sum_g c_g U_g psi in the kernel's order: (re, im) from (0, 0), elements in list order, the term t = c_g psi[src] with
    t_re = c_re v_re - c_im v_im and t_im = c_re v_im + c_im v_re formed first, then added.  complex128."""
    re, im = np.zeros(len(psi)), np.zeros(len(psi))
    for g, c in zip(elements, coef):
        v = apply(psi, L, nup, g)
        c = complex(c)
        if np.iscomplexobj(v):
            re = re + (c.real * v.real - c.imag * v.imag)
            im = im + (c.real * v.imag + c.imag * v.real)
        else:
            re = re + c.real * v
            im = im + c.imag * v
    return re + 1j * im


def phase(n, r, L):
    """e^{+i k_n r}, k_n = 2 pi n / L; exactly +-1 at k = 0 and k = pi"""
    if (n * r) % L == 0:
        return 1.0 + 0.0j
    if (2 * n * r) % L == 0:
        return -1.0 + 0.0j
    a = 2.0 * math.pi * ((n * r) % L) / L
    return complex(math.cos(a), math.sin(a))


def projector_list(L, momentum=None, parity=None, spin_flip=None):
    """elements and coefficients of P_n (1 + parity R)/2 (1 + spin_flip Z)/2, P_n = (1/L) sum_r e^{+i k_n r} T^r"""
    el, co = [], []
    for r in (range(L) if momentum is not None else (0,)):
        for refl in ((0, 1) if parity is not None else (0,)):
            for fl in ((0, 1) if spin_flip is not None else (0,)):
                c = phase(momentum, r, L) / L if momentum is not None else 1.0 + 0.0j
                if parity is not None:
                    c = c * (0.5 * (parity if refl else 1))
                if spin_flip is not None:
                    c = c * (0.5 * (spin_flip if fl else 1))
                el.append((r, refl, fl))
                co.append(c)
    return el, co


def project(psi, L, nup, momentum=None, parity=None, spin_flip=None):
    return combine(psi, L, nup, *projector_list(L, momentum, parity, spin_flip))


def momentum_weights(psi, L, nup):
    """w_n = <psi|P_n|psi> = (1/L) sum_r e^{i k_n r} <psi|T^r|psi>"""
    ov = overlaps(psi, psi, L, nup, [(r, 0, 0) for r in range(L)])
    return np.array([sum(phase(n, r, L) * ov[r] for r in range(L)).real / L for n in range(L)])


def labels(psi, L, nup, tol=1e-8):
    """(momentum, parity, spin_flip) of psi, None where it has none (or Z is undefined), by the definitions of the issue"""
    n2 = float(np.vdot(psi, psi).real)
    w = momentum_weights(psi, L, nup)
    hit = np.nonzero(w >= (1 - tol) * n2)[0]

    def sign(g):
        v = np.vdot(psi, apply(psi, L, nup, g)) / n2
        return 1 if abs(v - 1) <= tol else -1 if abs(v + 1) <= tol else None

    return (int(hit[0]) if len(hit) else None, sign((0, 1, 0)), sign((0, 0, 1)) if flip_defined(L, nup) else None)


# ---- torch ports: all rows of a sector of several million rows, formed where the vector lives ----------------------------------
def rot_right_t(s, L, r):
    r %= L
    if r == 0:
        return s.clone()
    return (s >> r) | ((s & ((1 << r) - 1)) << (L - r))


def R_t(s, L):
    import torch
    out = torch.zeros_like(s)
    for b in range(L):
        out = out | (((s >> b) & 1) << (L - 1 - b))
    return out


def source_t(s, L, g):
    r, refl, flip = g
    s = rot_right_t(s, L, r)
    if refl:
        s = R_t(s, L)
    if flip:
        s = s ^ ((1 << L) - 1)
    return s


def source_rows_t(s, L, nup, g):
    """s: the configurations of all rows (int64 tensor) -> the source row of every row"""
    assert not g[2] or flip_defined(L, nup)
    t = source_t(s, L, g)
    return t if nup is None else RR.rank_t(t, L, nup)


def apply_t(psi, s, L, nup, g):
    return psi[source_rows_t(s, L, nup, g)]


def overlaps_t(bra, ket, s, L, nup, elements):
    import torch
    out = []
    for g in elements:
        v = apply_t(ket, s, L, nup, g)
        out.append(complex((torch.conj(bra) * v).sum().item()) if bra.is_complex() else complex((bra * v).sum().item()))
    return np.array(out)


def combine_t(psi, s, L, nup, elements, coef):
    """the torch port of `combine`, same order -> complex128 tensor"""
    import torch
    re = torch.zeros(len(psi), dtype=torch.float64, device=psi.device)
    im = torch.zeros_like(re)
    for g, c in zip(elements, coef):
        v = apply_t(psi, s, L, nup, g)
        c = complex(c)
        if v.is_complex():
            vr, vi = v.real, v.imag
            re = re + (c.real * vr - c.imag * vi)
            im = im + (c.real * vi + c.imag * vr)
        else:
            re = re + c.real * v
            im = im + c.imag * v
    return torch.complex(re, im)
