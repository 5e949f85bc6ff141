"""Independent numpy restatement of the energy current: the term builder, the row loop of a term list, and dense
Kronecker-product operators.  It shares nothing with the library; tests/test_ecurrent_ref_host.py proves it on the CPU.

Conventions: sites 1-based, site i <-> bit i - 1; j'_ij = i (S+_i S-_j - S-_i S+_j); a term (i, j, k, c) stands for c Sz_k j'_ij,
k = 0: no Sz factor.  H = sum_a h_a with hops t (S+_i S-_j + h.c.), zz terms v Sz_i Sz_j and field terms B_i Sz_i.  A bond (i, j)
sits at x = i + delta / 2, delta = j - i, a field term at x = i; with `periodic`, delta and every position difference are minimum
images on a ring of L sites.  J_E = (i/2) sum_{a,b} d(a, b) [h_a, h_b], d(a, b) = x_b - x_a."""
import numpy as np

from typicality_ref import SM, SP, SZ, basis, bit, kron_site

DTERM = np.dtype([("i", np.int32), ("j", np.int32), ("k", np.int32), ("c", np.float64)], align=True)
DTERM_MAX = 4096


class Ambiguous(ValueError):
    """a position difference of exactly +-L/2 on a ring"""


def min_image(d, L, periodic):
    """d, or its representative in (-L/2, L/2) on a ring of L sites; exactly +-L/2 has two and is refused"""
    if not periodic:
        return d
    d = d - L * np.floor(d / L + 0.5)
    if 2 * abs(d) == L:
        raise Ambiguous(f"a position difference of +-L/2 = {L / 2} has no minimum image")
    return d


def bond_delta(i, j, L, periodic):
    return min_image(float(j - i), L, periodic)


def bond_x(i, j, L, periodic):
    return i + bond_delta(i, j, L, periodic) / 2


def energy_current_terms(L, hop, zz, field, periodic=False):
    """the term list of J_E: terms of equal (i, j, k) merged after orienting each to i < j (swapping i and j flips the sign),
    exact zeros dropped, sorted by (i, j, k) -> structured array (i, j, k, c)"""
    acc = {}

    def add(i, j, k, c):
        if i > j:
            i, j, c = j, i, -c
        acc[(i, j, k)] = acc.get((i, j, k), 0.0) + c

    hop = [(int(i), int(j), float(t)) for i, j, t in hop if i != j]
    zz = [(int(i), int(j), float(v)) for i, j, v in zz if i != j]
    field = np.zeros(L) if field is None else np.asarray(field, dtype=float)
    # hop with hop: i [F_pm, F_mq] = -2 Sz_m j'_pq, each unordered pair once
    for a, (ai, aj, ta) in enumerate(hop):
        for bi, bj, tb in hop[a + 1:]:
            shared = {ai, aj} & {bi, bj}
            if len(shared) != 1:
                continue
            m = shared.pop()
            p, q = (ai if aj == m else aj), (bi if bj == m else bj)
            d = min_image(bond_x(bi, bj, L, periodic) - bond_x(ai, aj, L, periodic), L, periodic)
            add(p, q, m, -2.0 * ta * tb * d)
    # hop with zz: i [F_pm, Z_mq] = j'_pm Sz_q
    for ai, aj, ta in hop:
        for bi, bj, vb in zz:
            shared = {ai, aj} & {bi, bj}
            if len(shared) != 1:
                continue
            m = shared.pop()
            p, q = (ai if aj == m else aj), (bi if bj == m else bj)
            d = min_image(bond_x(bi, bj, L, periodic) - bond_x(ai, aj, L, periodic), L, periodic)
            add(p, m, q, ta * vb * d)
    # hop with the fields of its two sites
    for ai, aj, ta in hop:
        bsum = field[ai - 1] + field[aj - 1]
        if bsum != 0.0:
            add(ai, aj, 0, 0.5 * bsum * bond_delta(ai, aj, L, periodic) * ta)
    keys = sorted(k for k, c in acc.items() if c != 0.0)
    if len(keys) > DTERM_MAX:
        raise ValueError("more than 4096 terms")
    out = np.zeros(len(keys), dtype=DTERM)
    for n, key in enumerate(keys):
        out[n] = (*key, acc[key])
    return out


def groups(terms):
    """[(i, j, [(k, c), ...])]: consecutive terms with the same ordered (i, j)"""
    out = []
    for t in terms:
        i, j, k, c = int(t[0]), int(t[1]), int(t[2]), float(t[3])
        if out and out[-1][0] == i and out[-1][1] == j:
            out[-1][2].append((k, c))
        else:
            out.append((i, j, [(k, c)]))
    return out


def apply_rows(terms, psi, L, nup):
    """(J psi)[s] = i sum_groups [s_i != s_j] (sigma co) psi[s with i, j exchanged]; co the sum over the group's terms, in list
    order from 0.0, of (k == 0 ? c : +-0.5 c by site k of s); sigma = +1 when site i is up; real and imaginary parts summed
    separately in group order from zero; the factor i as the swap (re, im) -> (-im, re).  Partner rows by the full rank of the
    exchanged configuration (the dictionary of the basis)."""
    states, index = basis(L, nup)
    N = len(states)
    psi = np.asarray(psi)
    pr = np.ascontiguousarray(psi.real, dtype=float)
    pi = np.ascontiguousarray(psi.imag, dtype=float) if np.iscomplexobj(psi) else None
    re, im = np.zeros(N), np.zeros(N)
    for i, j, tl in groups(terms):
        ui, uj = bit(states, i), bit(states, j)
        rows = np.nonzero(ui != uj)[0]
        if len(rows) == 0:
            continue
        mask = np.uint64((1 << (i - 1)) | (1 << (j - 1)))
        part = np.array([index[int(s)] for s in states[rows] ^ mask], dtype=np.int64)
        co = np.zeros(len(rows))
        for k, c in tl:
            co = co + (c if k == 0 else np.where(bit(states[rows], k), 0.5 * c, -(0.5 * c)))
        f = np.where(ui[rows], co, -co)
        re[rows] = re[rows] + f * pr[part]
        if pi is not None:
            im[rows] = im[rows] + f * pi[part]
    out = np.empty(N, dtype=np.complex128)
    out.real, out.imag = -im, re
    return out


def row_sum_bound(terms):
    """an upper bound of the largest absolute row sum of J: sum over groups of |sum of (|c| or |c|/2)|"""
    return float(sum(sum(abs(c) if k == 0 else 0.5 * abs(c) for k, c in tl) for _i, _j, tl in groups(terms)))


# ---- dense Kronecker-product operators ---------------------------------------------------------------------------------
def kron_bond_current(L, i, j):
    return 1j * (kron_site(L, i, SP) @ kron_site(L, j, SM) - kron_site(L, i, SM) @ kron_site(L, j, SP))


def kron_terms(L, terms):
    """sum of c Sz_k j'_ij in the full basis"""
    J = np.zeros((1 << L, 1 << L), dtype=np.complex128)
    for t in terms:
        i, j, k, c = int(t[0]), int(t[1]), int(t[2]), float(t[3])
        M = kron_bond_current(L, i, j)
        J += c * (M if k == 0 else kron_site(L, k, SZ) @ M)
    return J


def local_terms(L, hop, zz, field, periodic):
    """[(position, dense h_a, sites)] of the local terms of H"""
    out = []
    for i, j, t in hop:
        if i != j:
            F = kron_site(L, i, SP) @ kron_site(L, j, SM) + kron_site(L, i, SM) @ kron_site(L, j, SP)
            out.append(((i, j), t * F, {i, j}))
    for i, j, v in zz:
        if i != j:
            out.append(((i, j), v * kron_site(L, i, SZ) @ kron_site(L, j, SZ), {i, j}))
    if field is not None:
        for i in range(1, L + 1):
            if field[i - 1] != 0.0:
                out.append(((i, i), field[i - 1] * kron_site(L, i, SZ), {i}))
    return out


def dense_energy_current(L, hop, zz, field, periodic=False):
    """(i/2) sum_{a,b} d(a, b) [h_a, h_b] formed densely; terms without a common site commute and are skipped"""
    loc = local_terms(L, hop, zz, field, periodic)
    J = np.zeros((1 << L, 1 << L), dtype=np.complex128)
    for a, (sa, ha, ta) in enumerate(loc):
        for b, (sb, hb, tb) in enumerate(loc):
            if a == b or not (ta & tb):
                continue
            comm = ha @ hb - hb @ ha
            if not comm.any():
                continue
            xa = sa[0] if sa[0] == sa[1] else bond_x(sa[0], sa[1], L, periodic)
            xb = sb[0] if sb[0] == sb[1] else bond_x(sb[0], sb[1], L, periodic)
            J += 0.5j * min_image(xb - xa, L, periodic) * comm
    return J


def dense_boost_current(L, hop, zz, field):
    """i [H, sum_a x_a h_a] on a line"""
    loc = local_terms(L, hop, zz, field, False)
    H = sum(h for _s, h, _t in loc)
    K = sum((s[0] if s[0] == s[1] else bond_x(s[0], s[1], L, False)) * h for s, h, _t in loc)
    return 1j * (H @ K - K @ H)


# ---- the row loop with torch, where the vectors live -------------------------------------------------------------------
def apply_rows_t(terms, psis, s, idx, L, nup):
    """`apply_rows` for every vector of `psis` (float64 or complex128 tensors of the whole basis) on the device of the int64
    tensors s (configurations) and idx (rows) -> [(re, im)] float64 tensors.  One torch call per multiply and per add, so nothing
    is contracted; the partner row is rows_ref.rank_t of the exchanged configuration, or idx ^ mask in the full basis, found once
    per group for all vectors."""
    import torch

    import rows_ref as RR
    parts = [(p.real.contiguous(), p.imag.contiguous()) if p.is_complex() else (p, None) for p in psis]
    zeros = lambda: torch.zeros(len(idx), dtype=torch.float64, device=idx.device)      # noqa: E731
    acc = [[zeros(), zeros() if pi is not None else None] for _pr, pi in parts]
    for i, j, tl in groups(terms):
        up_i = ((s >> (i - 1)) & 1).to(torch.bool)
        up_j = ((s >> (j - 1)) & 1).to(torch.bool)
        fl = up_i != up_j
        mask = (1 << (i - 1)) | (1 << (j - 1))
        if nup is None:
            partner = torch.where(fl, idx ^ mask, idx)
        else:
            partner = RR.rank_t(torch.where(fl, s ^ mask, s), L, nup)
        co = zeros()
        for k, c in tl:
            if k == 0:
                co = co + c
            else:
                h = 0.5 * c
                co = co + torch.where(((s >> (k - 1)) & 1).to(torch.bool), torch.full_like(co, h), torch.full_like(co, -h))
        f = torch.where(up_i, co, -co)
        for a, (pr, pi) in zip(acc, parts):
            a[0] = torch.where(fl, a[0] + f * pr[partner], a[0])
            if pi is not None:
                a[1] = torch.where(fl, a[1] + f * pi[partner], a[1])
    return [(torch.zeros_like(re) if im is None else -im, re) for re, im in acc]
