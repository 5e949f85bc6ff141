"""Numpy restatement of site permutations and of the reduced density matrix of any set of sites, sharing nothing with the library.
The basis comes from itertools.combinations (or range(2**L)), as in tests/entanglement_ref.py.

A permutation is perm[0..L-1], perm[i] the 1-based site to which the spin of site i + 1 moves: U|s> = |pi s>, so
(U psi)[idx(s)] = psi[idx(src(s))] with bit i of src(s) = bit perm[i] - 1 of s.  `source_rows` finds the rows with per-bit loops and
a dict from configuration to row.  `rho` scatters psi into a dense 2^L array, reshapes it to L axes of 2, moves the axes of the
listed sites to the front and forms rho = M M^dagger in np.clongdouble; blocks are cut out by popcount."""
import itertools
import math

import numpy as np


def basis(L, nup):
    """the configurations in basis order as a list of Python ints: sorted site lists in lexicographic order (site i is bit i - 1), or
    0 .. 2^L - 1"""
    if nup is None:
        return list(range(1 << L))
    return [sum(1 << b for b in c) for c in itertools.combinations(range(L), nup)]


def source_config(s, L, perm):
    t = 0
    for i in range(L):
        if (s >> (perm[i] - 1)) & 1:
            t |= 1 << i
    return t


def source_rows(L, nup, perm):
    """row of psi that every row of U psi copies, as an int64 array"""
    st = basis(L, nup)
    row = {s: k for k, s in enumerate(st)}
    return np.array([row[source_config(s, L, perm)] for s in st], dtype=np.int64)


def permute(psi, L, nup, perm):
    return np.asarray(psi)[source_rows(L, nup, perm)]


def translation(L):
    return [(i + 1) % L + 1 for i in range(L)]


def reflection(L):
    return [L - i for i in range(L)]


def stable_partition(L, sites):
    """sites[j] -> site j + 1 in the order given, the other sites -> len(sites) + 1 .. L in ascending order"""
    perm = [0] * L
    for j, s in enumerate(sites):
        perm[s - 1] = j + 1
    nxt = len(sites) + 1
    for i in range(L):
        if perm[i] == 0:
            perm[i] = nxt
            nxt += 1
    return perm


def matrix(psi, L, nup, sites):
    """M[r, e] in np.clongdouble, r = sum_j bit(sites[j]) << j the configuration of the listed sites, e the environment: psi scattered
    into 2^L entries, L axes of 2 (axis a = site L - a in C order), the listed sites' axes moved to the front"""
    s = len(sites)
    full = np.zeros(1 << L, dtype=np.clongdouble)
    full[np.array(basis(L, nup), dtype=np.int64)] = np.asarray(psi)
    T = full.reshape((2,) * L)                                    # axis a <-> bit L - 1 - a
    front = [L - 1 - (x - 1) for x in reversed(sites)]            # sites[s-1] slowest ... sites[0] fastest of the row index
    rest = [a for a in range(L) if a not in front]
    return np.transpose(T, front + rest).reshape(1 << s, 1 << (L - s))


def rho(psi, L, nup, sites):
    """rho_S = M M^dagger, un-normalised, as a dense 2^s x 2^s np.clongdouble matrix"""
    M = matrix(psi, L, nup, sites)
    return M @ M.conj().T


def blocks(R, n_sites, nup, L):
    """{m: (block of the dense matrix R over the configurations with m up spins, in the basis order of the sector (n_sites, m); K_m)},
    K_m = C(L - n_sites, nup - m) the environment dimension; the full basis: {-1: (R, 2^(L - n_sites))}"""
    if nup is None:
        return {-1: (R, 1 << (L - n_sites))}
    out = {}
    for m in range(max(0, nup - (L - n_sites)), min(n_sites, nup) + 1):
        idx = np.array(basis(n_sites, m), dtype=np.int64)
        out[m] = (R[np.ix_(idx, idx)], math.comb(L - n_sites, nup - m))
    return out


def rho_blocks(psi, L, nup, sites):
    """blocks(rho(...)) without the dense 2^s x 2^s matrix: rows of M of different popcount have disjoint support in the environment,
    so the block of m is M_m M_m^dagger over the rows of popcount m alone"""
    s = len(sites)
    M = matrix(psi, L, nup, sites)
    if nup is None:
        return {-1: (M @ M.conj().T, 1 << (L - s))}
    out = {}
    for m in range(max(0, nup - (L - s)), min(s, nup) + 1):
        Mm = M[np.array(basis(s, m), dtype=np.int64)]
        out[m] = (Mm @ Mm.conj().T, math.comb(L - s, nup - m))
    return out


def entropy(R):
    """von Neumann entropy of the dense matrix R / tr R (double precision eigensolver)"""
    lam = np.linalg.eigvalsh(np.asarray(R, dtype=np.complex128))
    lam = lam / lam.sum()
    lam = lam[lam > 0.0]
    return float(-(lam * np.log(lam)).sum())


def mutual_information(psi, L, nup, A, B):
    A, B = list(A), list(B)
    s_ab = entropy(rho(psi, L, nup, A + B)) if len(A) + len(B) < L else 0.0
    return entropy(rho(psi, L, nup, A)) + entropy(rho(psi, L, nup, B)) - s_ab


def partial_transpose(R, n_a, n_b):
    dA, dB = 1 << n_a, 1 << n_b
    out = np.empty_like(R)
    for a in range(dA):                                           # explicit loops: <a b|R^T_B|a' b'> = <a b'|R|a' b>
        for b in range(dB):
            for a2 in range(dA):
                for b2 in range(dB):
                    out[a + (b << n_a), a2 + (b2 << n_a)] = R[a + (b2 << n_a), a2 + (b << n_a)]
    return out


def log_negativity(psi, L, nup, A, B):
    A, B = list(A), list(B)
    R = np.asarray(rho(psi, L, nup, A + B), dtype=np.complex128)
    R = R / np.trace(R).real
    return math.log(float(np.abs(np.linalg.eigvalsh(partial_transpose(R, len(A), len(B)))).sum()))


def singlet_product_state(L, nup, pairs):
    """product of singlets (|ud> - |du>)/sqrt 2 on the listed site pairs, the other sites filled up from site order so that the total
    number of up spins is nup: the lowest remaining sites up.  Returns the vector in the sector's basis order."""
    used = {x for p in pairs for x in p}
    rest = [i for i in range(1, L + 1) if i not in used]
    n_up_rest = nup - len(pairs)
    assert 0 <= n_up_rest <= len(rest)
    base = sum(1 << (i - 1) for i in rest[:n_up_rest])
    st = basis(L, nup)
    row = {s: k for k, s in enumerate(st)}
    psi = np.zeros(len(st))
    for choice in itertools.product((0, 1), repeat=len(pairs)):
        s, sign = base, 1.0
        for (i, j), c in zip(pairs, choice):
            s |= 1 << ((i if c == 0 else j) - 1)                  # c = 0: site i up, site j down; c = 1 the other way, with a minus
            sign *= 1.0 if c == 0 else -1.0
        psi[row[s]] = sign / math.sqrt(2.0) ** len(pairs)
    return psi
