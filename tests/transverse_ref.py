"""numpy reference of S^-_q / S^+_q between adjacent sectors for the transverse tests (shares nothing with the library).

Combinadic rank of the basis order (site i <-> bit i-1, sites in order, "site up" first) and the gather loop of the
operator in the order the library fixes: per target row r = 0..L-1 ascending, acc.re += c_r x.re - s_r x.im,
acc.im += c_r x.im + s_r x.re, then out = acc / sqrt(L) componentwise -- every product and sum rounded on its own.
"""
import math

import numpy as np


def binom_table(L):
    C = np.zeros((L + 1, L + 2), dtype=np.int64)
    for n in range(L + 1):
        for k in range(n + 1):
            C[n, k] = math.comb(n, k)
    return C


def rank(states, L, nup):
    """0-based position of each configuration in sector (L, nup): sum over down sites k (1-based) while ups remain of
    C(L - k, r_k - 1), r_k = ups not yet placed."""
    s = np.asarray(states, dtype=np.int64)
    C = binom_table(L)
    idx = np.zeros(s.shape, dtype=np.int64)
    r = np.full(s.shape, nup, dtype=np.int64)
    for k in range(1, L + 1):
        bit = (s >> (k - 1)) & 1
        add = (bit == 0) & (r > 0)
        idx[add] += C[L - k, r[add] - 1]
        r -= bit
    return idx


def unrank(idx, L, nup):
    idx = np.array(idx, dtype=np.int64)
    C = binom_table(L)
    s = np.zeros(idx.shape, dtype=np.int64)
    r = np.full(idx.shape, nup, dtype=np.int64)
    for k in range(1, L + 1):
        live = r > 0
        c = np.where(live, C[L - k, np.maximum(r - 1, 0)], 0)
        up = live & (idx < c)
        s[up] |= np.int64(1) << (k - 1)
        r[up] -= 1
        dn = live & ~up
        idx[dn] -= c[dn]
    return s


def sector_states(L, nup):
    """All configurations of sector (L, nup) in basis order (small L)."""
    allst = np.arange(1 << L, dtype=np.int64)
    pc = np.zeros(allst.shape, dtype=np.int64)
    for k in range(L):
        pc += (allst >> k) & 1
    st = allst[pc == nup]
    out = np.empty_like(st)
    out[rank(st, L, nup)] = st
    return out


def spm_rows(L, nup_src, psi_at, states, q, op):
    """(S^-_q psi) (op "minus") or (S^+_q psi) (op "plus") at the target configurations `states`; psi_at(j) returns psi at
    source rows j (complex or real).  nup_src None: full basis (row = configuration)."""
    want = 0 if op == "minus" else 1
    ar = np.zeros(len(states))
    ai = np.zeros(len(states))
    for r in range(L):
        m = ((states >> r) & 1) == want
        if not m.any():
            continue
        part = states[m] ^ (np.int64(1) << r)
        j = part if nup_src is None else rank(part, L, nup_src)
        x = np.asarray(psi_at(j))
        xr = np.ascontiguousarray(x.real, dtype=np.float64)
        xi = np.ascontiguousarray(x.imag, dtype=np.float64) if np.iscomplexobj(x) else np.zeros(len(j))
        c, s = math.cos(q * r), math.sin(q * r)
        ar[m] = ar[m] + (c * xr - s * xi)
        ai[m] = ai[m] + (c * xi + s * xr)
    nf = 1.0 / math.sqrt(L)
    out = np.empty(len(states), dtype=np.complex128)
    out.real = nf * ar
    out.imag = nf * ai
    return out


def spm(L, nup_src, psi, q, op):
    """The whole target vector: sector nup_src -+ 1 (or the full basis when nup_src is None)."""
    if nup_src is None:
        states = np.arange(1 << L, dtype=np.int64)
    else:
        states = sector_states(L, nup_src + (-1 if op == "minus" else 1))
    return spm_rows(L, nup_src, lambda j: psi[j], states, q, op)
