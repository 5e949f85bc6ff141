"""Independent numpy restatement of the finite-temperature typicality functions: the row-loop spin current, the
Chebyshev and Krylov imaginary-time steps with their truncation rules, the real-time steps and the per-sample loop

    psi_beta = exp(-beta H / 2) r / |.|,  num(t) = <psi_beta(t)| A |phi(t)>,  phi(t) = exp(-iHt) B psi_beta,  den = |exp(-beta H/2) r|^2.

Written from the definitions; it shares nothing with the library or the oracle.  Sites are 1-based, site i <-> bit i - 1; a
sector's basis is ordered lexicographically over the sorted lists of up sites (site 1 first)."""
import itertools

import numpy as np
import scipy.sparse as sp
import scipy.special as ss

EPS53 = 2.0 ** -53


# ---- basis -------------------------------------------------------------------------------------------------------------
def basis(L, nup):
    """(states, index) -- states[k] the configuration of row k, index[state] = k"""
    if nup is None:
        states = np.arange(1 << L, dtype=np.uint64)
    else:
        states = np.array([sum(1 << s for s in c) for c in itertools.combinations(range(L), nup)], dtype=np.uint64).reshape(-1)
    index = {int(s): k for k, s in enumerate(states)}
    return states, index


def bit(states, site):
    return ((states >> np.uint64(site - 1)) & np.uint64(1)).astype(bool)


def partners(states, index, i, j):
    """rows whose sites i, j differ, and the row each maps to when both are flipped"""
    bi, bj = bit(states, i), bit(states, j)
    rows = np.nonzero(bi != bj)[0]
    mask = np.uint64((1 << (i - 1)) | (1 << (j - 1)))
    part = np.array([index[int(s)] for s in states[rows] ^ mask], dtype=np.int64)
    return rows, part, bi[rows]


# ---- operators ---------------------------------------------------------------------------------------------------------
def hamiltonian(L, nup, hop, zz, field, states=None, index=None):
    """H = sum_hop t (S+_i S-_j + S-_i S+_j) + sum_zz J Sz_i Sz_j + sum_i h_i Sz_i as a sparse matrix on the basis"""
    if states is None:
        states, index = basis(L, nup)
    N = len(states)
    d = np.zeros(N)
    field = np.zeros(L) if field is None else np.asarray(field, dtype=float)
    for i in range(1, L + 1):
        d += field[i - 1] * np.where(bit(states, i), 0.5, -0.5)
    for i, j, J in zz:
        d += J * np.where(bit(states, i), 0.5, -0.5) * np.where(bit(states, j), 0.5, -0.5)
    H = sp.diags(d).tocsr()
    for i, j, t in hop:
        if i == j:
            continue
        rows, part, _ = partners(states, index, i, j)
        H = H + sp.csr_matrix((np.full(len(rows), float(t)), (rows, part)), shape=(N, N))
    return H.tocsr()


class CurrentPlan:
    """partner rows and signs of every hop, computed once: the row loop of J_w then is pure arithmetic"""

    def __init__(self, L, nup, hop, states=None, index=None):
        if states is None:
            states, index = basis(L, nup)
        self.N, self.hop = len(states), list(hop)
        self.bonds = [partners(states, index, i, j) if i != j else (np.zeros(0, int), np.zeros(0, int), np.zeros(0, bool))
                      for i, j, _ in self.hop]

    def apply(self, psi, weights=None):
        """(J_w psi)[s] = i sum_b (w_b t_b sigma_b) psi[partner]: hop-list order, zero start, the product (w_b t_b sigma_b) formed
        first, real and imaginary parts summed separately, the factor i as the swap (re, im) -> (-im, re)"""
        psi = np.asarray(psi)
        re, im = np.zeros(self.N), np.zeros(self.N)
        pr = np.ascontiguousarray(psi.real, dtype=float)
        pi = np.ascontiguousarray(psi.imag, dtype=float) if np.iscomplexobj(psi) else None
        for b, (i, j, t) in enumerate(self.hop):
            rows, part, up_i = self.bonds[b]
            wt = (1.0 if weights is None else float(weights[b])) * float(t)
            c = np.where(up_i, wt, -wt)
            re[rows] += c * pr[part]
            if pi is not None:
                im[rows] += c * pi[part]
        out = np.empty(self.N, dtype=np.complex128)
        out.real, out.imag = -im, re
        return out

    def matrix(self, weights=None):
        eye = np.eye(self.N)
        return np.array([self.apply(eye[k], weights) for k in range(self.N)]).T


def sz_site(states, site):
    return np.where(bit(states, site), 0.5, -0.5)


def sz_q(states, L, q):
    """diagonal of S^z_q = L^(-1/2) sum_r exp(iqr) S^z_{r+1}"""
    d = np.zeros(len(states), dtype=np.complex128)
    for r in range(L):
        d += np.exp(1j * q * r) * sz_site(states, r + 1)
    return d / np.sqrt(L)


# ---- Kronecker-product matrices (the independent check of the row forms) ------------------------------------------------
SP = np.array([[0.0, 1.0], [0.0, 0.0]])      # basis (up, down): S+ |down> = |up>
SM = SP.T
SZ = np.diag([0.5, -0.5])


def kron_site(L, site, op):
    """op on `site`, identity elsewhere, in the full basis indexed by the configuration integer (site i <-> bit i - 1, up = 1):
    index = sum_i bit_i 2^(i-1), so site L is the slowest Kronecker factor; local index 0 = down, 1 = up"""
    flip = np.array([[0, 1], [1, 0]])
    loc = flip @ op @ flip                     # reorder (up, down) -> (down, up) = bit value 0, 1
    M = np.ones((1, 1))
    for s in range(L, 0, -1):
        M = np.kron(M, loc if s == site else np.eye(2))
    return M


def kron_current(L, hop, weights=None):
    J = np.zeros((1 << L, 1 << L), dtype=np.complex128)
    for b, (i, j, t) in enumerate(hop):
        if i == j:
            continue
        w = 1.0 if weights is None else weights[b]
        J += 1j * w * t * (kron_site(L, i, SP) @ kron_site(L, j, SM) - kron_site(L, i, SM) @ kron_site(L, j, SP))
    return J


def kron_hamiltonian(L, hop, zz, field):
    H = np.zeros((1 << L, 1 << L))
    for i, j, t in hop:
        if i != j:
            H += t * (kron_site(L, i, SP) @ kron_site(L, j, SM) + kron_site(L, i, SM) @ kron_site(L, j, SP))
    for i, j, J in zz:
        H += J * kron_site(L, i, SZ) @ kron_site(L, j, SZ)
    if field is not None:
        for i in range(1, L + 1):
            H += field[i - 1] * kron_site(L, i, SZ)
    return H


def project(M, states):
    idx = states.astype(np.int64)
    return M[np.ix_(idx, idx)]


# ---- imaginary time ----------------------------------------------------------------------------------------------------
def rescaling(Emin, Emax):
    return (Emax - Emin) / (2 * 0.9999), (Emax + Emin) / 2


def imag_coeffs(z):
    """c_k = (2 - delta_k0) (-1)^k exp(-z) I_k(z), k < n_used; n_used = first k with k > z and ive(k, z) < 2^-53 ive(0, z)"""
    e0 = ss.ive(0, z)
    k = int(np.floor(z)) + 1
    while not ss.ive(k, z) < EPS53 * e0:
        k += 1
    ks = np.arange(k)
    c = ss.ive(ks, z) * np.where(ks % 2 == 1, -1.0, 1.0) * np.where(ks == 0, 1.0, 2.0)
    return c


def cheb_sum(H, psi, a, b, c):
    """sum_k c_k T_k((H - b)/a) psi"""
    def Ht(v):
        return (H @ v - b * v) / a
    t0 = psi.astype(np.complex128)
    out = c[0] * t0
    if len(c) == 1:
        return out
    t1 = Ht(t0)
    out = out + c[1] * t1
    for k in range(2, len(c)):
        t0, t1 = t1, 2.0 * Ht(t1) - t0
        out = out + c[k] * t1
    return out


def imag_chebyshev(H, r, tau, Ebounds, zmax=600.0):
    """(exp(-tau H) r / |.|, ln |exp(-tau H) r|): equal sub-steps with z = a tau_sub <= zmax, renormalised after each"""
    a, b = rescaling(*Ebounds)
    v = np.asarray(r, dtype=np.complex128)
    if tau == 0:
        n = np.linalg.norm(v)
        return v / n, np.log(n)
    z = a * tau
    nsub = int(np.ceil(z / zmax)) if z > zmax else 1
    tsub = tau / nsub
    c = imag_coeffs(a * tsub)
    ln = 0.0
    for _ in range(nsub):
        v = cheb_sum(H, v, a, b, c)
        n = np.linalg.norm(v)
        v = v / n
        ln += np.log(n) - tsub * (b - a)
    return v, ln


def lanczos(H, psi, m):
    n0 = np.linalg.norm(psi)
    V = [psi / n0]
    al, be = [], []
    for j in range(m):
        w = H @ V[j]
        al.append(np.vdot(V[j], w).real)
        w = w - al[j] * V[j]
        if j > 0:
            w = w - be[j - 1] * V[j - 1]
        if j < m - 1:
            bj = np.linalg.norm(w)
            if bj < 1e-14:
                break
            be.append(bj)
            V.append(w / bj)
    k = len(al)
    T = np.diag(al) + np.diag(be[: k - 1], 1) + np.diag(be[: k - 1], -1)
    return n0, np.array(V[:k]).T, T


def imag_krylov(H, r, tau, m=30):
    """one projection on m Lanczos vectors: V exp(-tau T) e_1 |r|, normalised, with the logarithm of its norm"""
    n0, V, T = lanczos(H, np.asarray(r, dtype=np.complex128), min(m, len(r)))
    th, Q = np.linalg.eigh(T)
    y = Q @ (np.exp(-tau * (th - th[0])) * Q[0]) * n0
    v = V @ y
    n = np.linalg.norm(v)
    return v / n, np.log(n) - tau * th[0]


# ---- real time ---------------------------------------------------------------------------------------------------------
def real_coeffs(a, b, dt, cheb_n=0):
    """c_k = (2 - delta_k0) (-i)^k J_k(a dt) exp(-i b dt); cheb_n = 0: first k with k > a dt and |J_k(a dt)| < 2^-53 terms"""
    z = a * dt
    if cheb_n == 0:
        k = int(np.floor(z)) + 1
        while not abs(ss.jv(k, z)) < EPS53:
            k += 1
        cheb_n = max(k, 1)
    ks = np.arange(cheb_n)
    return np.where(ks == 0, 1.0, 2.0) * (-1j) ** ks * ss.jv(ks, z) * np.exp(-1j * b * dt)


def real_krylov(H, psi, dt, m=30):
    """krylov_time_evolve: normalised result"""
    n0 = np.linalg.norm(psi)
    if n0 == 0:
        return psi.astype(np.complex128)
    _, V, T = lanczos(H, psi.astype(np.complex128), min(m, len(psi)))
    th, Q = np.linalg.eigh(T)
    v = V @ (Q @ (np.exp(-1j * dt * th) * Q[0]))
    return v / np.linalg.norm(v)


# ---- the per-sample loop -----------------------------------------------------------------------------------------------
class Operator:
    """kind: "Sz" (site), "Szq" (q), "Sz_all", "current" (weights or None)"""

    def __init__(self, kind, param, L, states, plan=None):
        self.kind, self.L = kind, L
        if kind == "Sz":
            self.d = sz_site(states, param)
        elif kind == "Szq":
            self.d = sz_q(states, L, param)
        elif kind == "Sz_all":
            self.d = np.array([sz_site(states, i) for i in range(1, L + 1)])
        else:
            self.plan, self.w = plan, param

    def apply(self, psi):                       # B psi
        return self.plan.apply(psi, self.w) if self.kind == "current" else self.d * psi

    def bracket(self, bra, ket):                # <bra| A |ket>; "Szq": the adjoint <S^z_q bra|ket>
        if self.kind == "current":
            return np.array([np.vdot(bra, self.plan.apply(ket, self.w))])
        if self.kind == "Sz_all":
            return (self.d * (bra.conj() * ket)).sum(axis=1)
        return np.array([np.vdot(self.d * bra, ket)])


def dqt_sample(H, A, B, beta, r, times, method="chebyshev", Ebounds=None, cheb_n=0, kry_m=30):
    """-> (num[nt, nA] for the normalised psi_beta, log_norm, energy)"""
    r = np.asarray(r, dtype=np.complex128)
    r = r / np.linalg.norm(r)
    if beta == 0:
        psi, ln = r, 0.0
    elif method == "chebyshev":
        psi, ln = imag_chebyshev(H, r, beta / 2, Ebounds)
    else:
        psi, ln = imag_krylov(H, r, beta / 2, kry_m)
    energy = np.vdot(psi, H @ psi).real / np.vdot(psi, psi).real
    phi = B.apply(psi)
    nphi = np.linalg.norm(phi)
    out, t_prev = [], 0.0
    a, b = rescaling(*Ebounds) if method == "chebyshev" else (1.0, 0.0)
    for t in times:
        dt = t - t_prev
        t_prev = t
        if dt > 0:
            if method == "chebyshev":
                c = real_coeffs(a, b, dt, cheb_n)
                psi, phi = cheb_sum(H, psi, a, b, c), cheb_sum(H, phi, a, b, c)
            else:
                psi = real_krylov(H, psi, dt, kry_m)
                phi = real_krylov(H, phi, dt, kry_m) * nphi
        out.append(A.bracket(psi, phi))
    return np.array(out), ln, energy


def dqt_dense(Hd, A, B, beta, r, times):
    """the same quantities from the eigen-decomposition of the dense H (exact propagators)"""
    w, U = np.linalg.eigh(Hd)
    r = np.asarray(r, dtype=np.complex128)
    r = r / np.linalg.norm(r)
    v = U @ (np.exp(-0.5 * beta * (w - w[0])) * (U.conj().T @ r))
    n = np.linalg.norm(v)
    ln = np.log(n) - 0.5 * beta * w[0]
    psi = v / n
    energy = np.vdot(psi, Hd @ psi).real
    phi = B.apply(psi)
    out = []
    for t in times:
        ph = np.exp(-1j * w * t)
        out.append(A.bracket(U @ (ph * (U.conj().T @ psi)), U @ (ph * (U.conj().T @ phi))))
    return np.array(out), ln, energy
