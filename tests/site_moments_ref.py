"""numpy restatement of the site-resolved KPM moments for the site-moment tests (shares nothing with the library; uses only
oracle/oracle.py for H~ v and oracle/dense.py for the dense H).

    mu_n^{ij} = <psi0| S^z_i T_n(H~) S^z_j |psi0>,  H~ = (H - b)/a,  sites 1-based, r_i = i - 1.

Arrays are indexed mu[s, n, i-1] with j = sources[s].
"""
import numpy as np


def site_sz(states, L):
    """sz[i-1, row] = +-1/2, the S^z value of site i in configuration states[row] (site i <-> bit i-1, bit 1 = up)."""
    st = np.asarray(states).astype(np.uint64)
    return np.array([((st >> np.uint64(i)) & np.uint64(1)).astype(np.float64) - 0.5 for i in range(L)])


def project(sz, bra, ket):
    """out[i-1] = sum_rows conj(bra) s_i ket"""
    return sz @ (np.conj(bra) * ket)


def site_moments(O, model, psi0, sources, M, a, b):
    """The recursion on the oracle's rescaled apply: v_0 = S^z_j psi0, v_1 = H~ v_0, v_n = 2 H~ v_{n-1} - v_{n-2}; a
    projection onto every S^z_i psi0 after each."""
    L = model.L
    sz = site_sz(model.states, L)
    psi0 = np.asarray(psi0)
    mu = np.zeros((len(sources), M, L), dtype=np.complex128)
    for s, j in enumerate(sources):
        v_prev = (sz[j - 1] * psi0).astype(np.complex128)
        mu[s, 0] = project(sz, psi0, v_prev)
        v_curr = O.apply_rescaled_H(model, v_prev, a, b)
        mu[s, 1] = project(sz, psi0, v_curr)
        for n in range(2, M):
            v_next = 2.0 * O.apply_rescaled_H(model, v_curr, a, b) - v_prev
            mu[s, n] = project(sz, psi0, v_next)
            v_prev, v_curr = v_curr, v_next
    return mu


def dense_spectral_moments(H, states, L, psi0, sources, M, a, b):
    """sum_k <psi0|S_i|k><k|S_j|psi0> T_n(x_k), x_k = (E_k - b)/a, from the eigen-decomposition of the dense H."""
    w, V = np.linalg.eigh(H)
    sz = site_sz(states, L)
    x = (w - b) / a
    amp = V.conj().T @ (sz * np.asarray(psi0)[None, :]).T          # amp[k, i] = <k|S_i psi0>
    T = np.empty((M, len(x)))
    T[0] = 1.0
    T[1] = x
    for n in range(2, M):
        T[n] = 2.0 * x * T[n - 1] - T[n - 2]
    mu = np.zeros((len(sources), M, L), dtype=np.complex128)
    for s, j in enumerate(sources):
        wgt = np.conj(amp) * amp[:, j - 1][:, None]                # [k, i] = conj(<k|S_i psi0>) <k|S_j psi0>
        mu[s] = T @ wgt
    return mu


def moments_q_all(mu, sources, q):
    """mu_n(q) = (1/L) sum_ij e^{-iq(r_i - r_j)} mu_n^{ij} (complex; its real part is the moment) from ALL sources."""
    L = mu.shape[2]
    ri = np.arange(L)
    rj = np.asarray(sources) - 1
    return np.einsum("i,sni,s->n", np.exp(-1j * q * ri), mu, np.exp(1j * q * rj)) / L


def moments_q_one(mu_j, j, q):
    """mu_n(q) = sum_i e^{-iq(r_i - r_j)} mu_n^{ij} from the ONE source j (translation-invariant psi0 and H); complex."""
    L = mu_j.shape[1]
    return (mu_j @ np.exp(-1j * q * np.arange(L))) * np.exp(1j * q * (j - 1))


def reconstruct_signed(mu_damped, omega, a, b, E0):
    """(mu_0 + 2 sum_{n>=1} mu_n T_n(x)) / (a pi sqrt(1 - x^2)), x = (omega + E0 - b)/a, 0 for |x| >= 1; NOT clamped."""
    mu = np.asarray(mu_damped)
    om = np.asarray(omega, dtype=np.float64)
    x = (om + E0 - b) / a
    ok = np.abs(x) < 1.0
    xs = np.where(ok, x, 0.0)
    n = np.arange(len(mu))
    T = np.cos(n[:, None] * np.arccos(xs)[None, :])
    coef = np.where(n == 0, 1.0, 2.0)[:, None] * mu[:, None]
    out = (coef * T).sum(axis=0) / (a * np.pi * np.sqrt(1.0 - xs * xs))
    return np.where(ok, out, 0.0)
