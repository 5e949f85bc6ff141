"""Plain numpy restatement of the operator strings, vectorised over all rows.  Site i is bit i - 1.  A term is the
tuple (plus P, minus M, z Z, c, op): three pairwise disjoint site masks (Python ints), a complex coefficient, the operator's index;

    O_k = sum_{t: op_t = k} c_t prod_{i in P_t} S^+_i prod_{j in M_t} S^-_j prod_{l in Z_t} S^z_l.

Consecutive terms with equal (P, M, op) form a group, and the row form, as the kernel computes it, is

    (O psi)[s] = sum_groups [(s & P) == P and (s & M) == 0] co_g(s) psi[row(s ^ (P | M))]
    co_g(s)    = sum over the group's terms, in list order from (0.0, 0.0), of sigma_t(s) ch_t,
                 sigma_t(s) = +1 when popcount(~s & Z_t) is even, else -1;  ch_t = c_t 2^-|Z_t|
    product      t_re = co_re v_re - co_im v_im, t_im = co_re v_im + co_im v_re, both products first, then the add or subtract
                 (a real psi: t_re = co_re v, t_im = co_im v)
    (re, im) accumulated from (0.0, 0.0) in group order.

One numpy call per multiply and per add, so nothing is contracted.  Rows and configurations by rows_ref.rank / unrank (the row index
itself in the full basis).  Shares nothing with the library; tests/test_opstring_ref_host.py proves it against Kronecker products."""
import itertools
import math

import numpy as np

import rows_ref as RR


def bit(site):
    return 1 << (site - 1)


def popcount(x):
    return bin(x).count("1")


def configurations(L, nup):
    N = (1 << L) if nup is None else math.comb(L, nup)
    rows = np.arange(N, dtype=np.int64)
    return rows.astype(np.uint64) if nup is None else RR.unrank(rows, L, nup)


def rows_of(s, L, nup):
    return s.astype(np.int64) if nup is None else RR.rank(s, L, nup)


# ---- builders ----
def expand(coeff, factors, op=0):
    """coeff * prod of ("+", i), ("-", j), ("z", k), ("x", a), ("y", b): S^x = (S^+ + S^-)/2, S^y = (S^+ - S^-)/(2i); the S^+
    choice of every x / y factor first -> list of terms"""
    P = M = Z = 0
    xy = []
    for kind, site in factors:
        assert not (P | M | Z | sum(b for _k, b in xy)) & bit(site), "repeated site"
        if kind == "+":
            P |= bit(site)
        elif kind == "-":
            M |= bit(site)
        elif kind == "z":
            Z |= bit(site)
        else:
            assert kind in ("x", "y")
            xy.append((kind, bit(site)))
    out = []
    for choice in itertools.product((0, 1), repeat=len(xy)):
        p, m, c = P, M, complex(coeff)
        for (kind, b), lower in zip(xy, choice):
            if lower:
                m |= b
                c = c * (0.5 if kind == "x" else 0.5j)
            else:
                p |= b
                c = c * (0.5 if kind == "x" else -0.5j)
        out.append((p, m, Z, c, op))
    return out


def simplify(terms):
    """coefficients of equal (op, P, M, Z) added, exact zeros dropped, sorted by (op, P, M, Z)"""
    acc = {}
    for P, M, Z, c, op in terms:
        acc[(op, P, M, Z)] = acc.get((op, P, M, Z), 0j) + complex(c)
    return [(P, M, Z, c, op) for (op, P, M, Z), c in sorted(acc.items()) if c != 0]


def adjoint(terms):
    return [(M, P, Z, complex(c).conjugate(), op) for P, M, Z, c, op in terms]


def is_hermitian(terms):
    key = lambda tl: {(op, P, M, Z): c for P, M, Z, c, op in simplify(tl)}      # noqa: E731
    return key(terms) == key(adjoint(terms))


def sector_terms(terms):
    """the terms that conserve S^z: all that acts inside a fixed-nup sector"""
    return [t for t in terms if popcount(t[0]) == popcount(t[1])]


def hamiltonian_terms(hop, zz, field):
    """the lists of a model as strings of op 0, in list order: t S^+_i S^-_j then t S^-_i S^+_j per hop, v S^z_i S^z_j, B_i S^z_i"""
    out = []
    for i, j, t in hop:
        if i != j:
            out += [(bit(i), bit(j), 0, complex(t), 0), (bit(j), bit(i), 0, complex(t), 0)]
    for i, j, v in zz:
        out.append((0, 0, 0, complex(0.25 * v), 0) if i == j else (0, 0, bit(i) | bit(j), complex(v), 0))
    for i, h in enumerate(field, start=1):
        out.append((0, 0, bit(i), complex(h), 0))
    return out


EPS = (((0, 1, 2), 1.0), ((1, 2, 0), 1.0), ((2, 0, 1), 1.0), ((0, 2, 1), -1.0), ((2, 1, 0), -1.0), ((1, 0, 2), -1.0))


def chirality(i, j, k, coeff=1.0, op=0):
    """coeff S_i . (S_j x S_k) = coeff sum_abc eps_abc S^a_i S^b_j S^c_k, expanded and added up per (P, M, Z)"""
    out = []
    for perm, sign in EPS:
        out += expand(sign * coeff, [("xyz"[a], s) for a, s in zip(perm, (i, j, k))], op)
    return simplify(out)


def product(a, b, op=0):
    """the product of two operators on disjoint sites"""
    return simplify([(P1 | P2, M1 | M2, Z1 | Z2, complex(c1) * complex(c2), op)
                     for P1, M1, Z1, c1, _o1 in a for P2, M2, Z2, c2, _o2 in b])


def string_order(i, j, op=0):
    """-S^z_i exp(i pi sum_{i<l<j} S^z_l) S^z_j with exp(i pi S^z) = 2i S^z: one diagonal term"""
    return [(0, 0, sum(bit(l) for l in range(i, j + 1)), -((2j) ** (j - i - 1)), op)]


def from_ecurrent(terms, op=0):
    """(i, j, k, c) = c S^z_k i (S^+_i S^-_j - S^-_i S^+_j) (tests/ecurrent_ref.py) as strings, one (P, M) at a time"""
    fwd, bwd = [], []
    for t in terms:
        i, j, k, c = int(t[0]), int(t[1]), int(t[2]), float(t[3])
        Z = bit(k) if k else 0
        fwd.append((bit(i), bit(j), Z, complex(0.0, c), op))
        bwd.append((bit(j), bit(i), Z, complex(0.0, -c), op))
    key = lambda t: (t[0], t[1])      # noqa: E731
    return sorted(fwd + bwd, key=key)          # stable: every (P, M) becomes one group, its terms in list order


def from_bond(i, j, xy=1.0, zz=1.0, op=0):
    """D_b = xy/2 (S^+_i S^-_j + S^-_i S^+_j) + zz S^z_i S^z_j (tests/dimer_ref.py)"""
    return [(0, 0, bit(i) | bit(j), complex(zz), op), (bit(i), bit(j), 0, complex(0.5 * xy), op),
            (bit(j), bit(i), 0, complex(0.5 * xy), op)]


# ---- the row form ----
def groups(terms):
    """[(P, M, op, [(Z, ch_re, ch_im), ...])]: consecutive terms with equal (P, M, op); ch = c 2^-|Z|"""
    out = []
    for P, M, Z, c, op in terms:
        c = complex(c)
        sc = 2.0 ** -popcount(Z)
        if not out or out[-1][:3] != (P, M, op):
            out.append((P, M, op, []))
        out[-1][3].append((Z, c.real * sc, c.imag * sc))
    return out


def n_ops(terms):
    return 1 + max((t[4] for t in terms), default=-1)


def _group_rows(s, P, M, tl):
    """rows the group contributes to, and (co_re, co_im) there"""
    u = np.uint64
    rows = np.nonzero((s & u(P | M)) == u(P))[0]              # every S^+ site up and every S^- site down
    ss = s[rows]
    co_re, co_im = np.zeros(len(rows)), np.zeros(len(rows))
    for Z, ch_re, ch_im in tl:
        odd = np.zeros(len(rows), dtype=bool)
        for b in range(64):
            if (Z >> b) & 1:
                odd ^= ((ss >> u(b)) & u(1)) == u(0)          # a down spin among the S^z sites flips the sign
        sign = np.where(odd, -1.0, 1.0)
        co_re = co_re + sign * ch_re
        co_im = co_im + sign * ch_im
    return rows, ss, co_re, co_im


def _split(psi):
    """(real parts, imaginary parts or None) as contiguous float64 arrays"""
    psi = np.asarray(psi)
    return (np.ascontiguousarray(psi.real, dtype=np.float64),
            np.ascontiguousarray(psi.imag, dtype=np.float64) if np.iscomplexobj(psi) else None)


def _contributions(terms, parts, L, nup, op, s):
    """per group of operator `op`, in list order: (rows, t_re, t_im, number of terms, sum |ch_t| |v|); parts = _split(psi)"""
    pr, pi = parts
    cplx = pi is not None
    assert len(pr) == len(s)
    for P, M, o, tl in groups(terms):
        if o != op:
            continue
        assert nup is None or popcount(P) == popcount(M), "a sector needs |P| = |M|"
        rows, ss, co_re, co_im = _group_rows(s, P, M, tl)
        if len(rows) == 0:
            continue
        src = rows if (P | M) == 0 else rows_of(ss ^ np.uint64(P | M), L, nup)
        if cplx:
            vr, vi = pr[src], pi[src]
            a, b = co_re * vr, co_im * vi
            c, d = co_re * vi, co_im * vr
            t_re, t_im, absv = a - b, c + d, np.hypot(vr, vi)
        else:
            v = pr[src]
            t_re, t_im, absv = co_re * v, co_im * v, np.abs(v)
        yield rows, t_re, t_im, len(tl), sum(math.hypot(ch_re, ch_im) for _Z, ch_re, ch_im in tl) * absv


def apply_rows(terms, psi, L, nup, op=0, s=None, contributions=False):
    """(O_op psi) on all rows -> complex128 (the real part is what a float64 output holds).  contributions=True: also, per row, the
    number of contributing terms and the sum of |ch_t| |v| over them (what a rounding bar of the row is made of)."""
    s = configurations(L, nup) if s is None else s
    N = len(s)
    re, im = np.zeros(N), np.zeros(N)
    cnt, mag = np.zeros(N, dtype=np.int64), np.zeros(N)
    for rows, t_re, t_im, nt, m in _contributions(terms, _split(psi), L, nup, op, s):
        re[rows] = re[rows] + t_re
        im[rows] = im[rows] + t_im
        if contributions:
            cnt[rows] += nt
            mag[rows] += m
    out = np.empty(N, dtype=np.complex128)
    out.real, out.imag = re, im
    return (out, cnt, mag) if contributions else out


def fused(o, y, b, real=False):
    """o + b y as the kernel forms it: t = b y with both products first, then the add or subtract; then one add per component"""
    b = complex(b)
    if real:
        return o.real + b.real * np.asarray(y, dtype=np.float64)
    y = np.asarray(y, dtype=np.complex128)
    tr = b.real * y.real - b.imag * y.imag
    ti = b.real * y.imag + b.imag * y.real
    out = np.empty(len(o), dtype=np.complex128)
    out.real, out.imag = o.real + tr, o.imag + ti
    return out


def expectations(terms, bra, ket, L, nup, s=None):
    """[(value, scale)] per operator: value = sum_s conj(bra[s]) (O_k ket)[s] with math.fsum over the products' parts,
    scale = sum_s |bra[s] (O_k ket)[s]|.  bra may be a list of vectors: then one such list per bra.  Only the rows an operator
    reaches are formed: their values are the row form's, accumulated in group order (np.add.at adds in index order)."""
    s = configurations(L, nup) if s is None else s
    many = isinstance(bra, (list, tuple))
    bras = [np.asarray(b) for b in (bra if many else [bra])]
    out = [[] for _ in bras]
    kparts = _split(ket)
    for k in range(n_ops(terms)):
        parts = list(_contributions(terms, kparts, L, nup, k, s))
        if not parts:
            for o in out:
                o.append((0j, 0.0))
            continue
        rows, inv = np.unique(np.concatenate([p[0] for p in parts]), return_inverse=True)
        re, im = np.zeros(len(rows)), np.zeros(len(rows))
        np.add.at(re, inv, np.concatenate([p[1] for p in parts]))
        np.add.at(im, inv, np.concatenate([p[2] for p in parts]))
        val = np.empty(len(rows), dtype=np.complex128)
        val.real, val.imag = re, im
        for b, o in zip(bras, out):
            prod = np.conj(b[rows]) * val
            o.append((complex(math.fsum(prod.real.tolist()), math.fsum(prod.imag.tolist())), float(np.abs(prod).sum())))
    return out if many else out[0]
