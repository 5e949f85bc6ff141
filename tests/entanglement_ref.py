"""Numpy restatement of the reduced density matrix across a chain cut, sharing nothing with the library: the basis comes from
itertools.combinations (or range(2**L)), psi is scattered into M[s & mask, s >> k] and rho_A = M M^dagger, rho_B = M^T conj(M) are
formed in extended precision (np.longdouble / np.clongdouble).  Blocks are cut out by the popcount of the prefix and ordered by first
appearance in the basis."""
import functools
import itertools
import math

import numpy as np


@functools.lru_cache(maxsize=8)
def basis(L, nup):
    """the configurations in basis order as an int64 array: sorted site lists in lexicographic order (site i is bit i - 1), or
    0 .. 2^L - 1"""
    if nup is None:
        return np.arange(1 << L, dtype=np.int64)
    if nup == 0:
        return np.zeros(1, dtype=np.int64)
    sites = np.array(list(itertools.combinations(range(L), nup)), dtype=np.int64)
    return (np.int64(1) << sites).sum(axis=1)


def popcount(x):
    x = np.asarray(x, dtype=np.int64)
    n = np.zeros(x.shape, dtype=np.int64)
    for b in range(63):
        n += (x >> b) & 1
    return n


def matrix(psi, L, nup, cut):
    """M[P, S] = psi_s for s = P | S << cut, in extended precision; zero where (P, S) is not in the basis"""
    cplx = np.iscomplexobj(psi)
    M = np.zeros((1 << cut, 1 << (L - cut)), dtype=np.clongdouble if cplx else np.longdouble)
    s = basis(L, nup)
    M[s & ((1 << cut) - 1), s >> cut] = np.asarray(psi)
    return M


def _in_order_of_first_appearance(v):
    u, idx = np.unique(v, return_index=True)
    return u[np.argsort(idx, kind="stable")]


def first_appearance(L, nup, cut):
    """({m: prefixes in order of first appearance}, {m: suffixes in order of first appearance}); the full basis has the one key -1"""
    s = basis(L, nup)
    P, S = s & ((1 << cut) - 1), s >> cut
    m = np.full(len(s), -1) if nup is None else popcount(P)
    pre, suf = {}, {}
    for mm in np.unique(m):
        pre[int(mm)] = _in_order_of_first_appearance(P[m == mm])
        suf[int(mm)] = _in_order_of_first_appearance(S[m == mm])
    return pre, suf


def gram_blocks(psi, L, nup, cut, side):
    """{m: (G_m in extended precision, K_m)}: side 'A' G = M_m M_m^dagger over the prefixes, side 'B' G = M_m^T conj(M_m) over the
    suffixes, M_m the rows / columns of the block in order of first appearance; K_m the summation length.  side 'auto': the smaller
    side per block, a tie goes to A."""
    M = matrix(psi, L, nup, cut)
    pre, suf = first_appearance(L, nup, cut)
    out = {}
    for m in sorted(pre):
        Mm = M[np.ix_(pre[m], suf[m])]
        sd = side if side != "auto" else ("A" if len(pre[m]) <= len(suf[m]) else "B")
        if sd == "A":
            out[m] = (Mm @ Mm.conj().T, len(suf[m]))
        else:
            out[m] = (Mm.T @ Mm.conj(), len(pre[m]))
    return out


def spectrum(psi, L, nup, cut, side="auto"):
    """{m: eigenvalues of rho_m, descending, clipped at 0}, normalised by the total trace (double precision eigensolver)"""
    G = gram_blocks(psi, L, nup, cut, side)
    tr = sum(float(np.trace(g).real) for g, _ in G.values())
    return {m: np.clip(np.linalg.eigvalsh(np.asarray(g, dtype=np.complex128 if np.iscomplexobj(g) else np.float64))[::-1] / tr, 0.0, None)
            for m, (g, _) in G.items()}


def entropy(lams, q=1):
    lam = np.concatenate([np.asarray(v, dtype=np.float64) for v in lams.values()]) if isinstance(lams, dict) else np.asarray(lams)
    lam = lam[lam > 0.0]
    if q == 1:
        return float(-(lam * np.log(lam)).sum())
    if math.isinf(q):
        return -math.log(lam.max())
    return math.log(float((lam ** q).sum())) / (1.0 - q)


def entry_bound(G, K):
    """4 (K + 4) 2^-53 sqrt(G_aa G_bb): the forward bound of a K-term complex dot product in any order, with Cauchy-Schwarz"""
    dg = np.sqrt(np.abs(np.asarray(np.diag(G).real, dtype=np.float64)))
    return 4.0 * (K + 4) * 2.0 ** -53 * np.outer(dg, dg)
