"""numpy / torch restatement of the diagonal drives and the stage schedules, for the tests.

A drive is written here as a tuple (site_w or None, [(i, j), ...] 1-based, [v, ...]).

1. effective_weights: the table of one stage, as the library's host code forms it -- W_i = sum_k c_k w_{k,i} from 0.0 in ascending k,
   one multiply then one add per term; the concatenated bond list with weights c_k v_{k,b}; the halves W_i / 2 and quarters V_b / 4.
2. diag_values: d(s) in the contract's order, bit for bit -- from 0.0 the site terms i = 0..L-1, each +-W_i/2 selected, then the bond
   terms in list order, each +-V_b/4 with + for parallel spins; the site loop skipped when no drive has site weights.
   drive_rows: h + d psi per component, one multiply and one add.  Both run on numpy arrays or on torch tensors (eager torch does
   not contract a * b + c), so the large shapes are restated on the device.
3. magnus_schedule / piecewise_schedule and the dense stage propagator by eigh."""
import math

import numpy as np


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def effective_weights(L, drives, coefs):
    """(has_sites, wh[L], bits [(bi, bj) 0-based], vq) of sum_k coefs[k] D_k"""
    has_sites = any(d[0] is not None for d in drives)
    wh = np.zeros(L)
    for i in range(L):
        W = 0.0
        for k, d in enumerate(drives):
            if d[0] is not None:
                t = float(coefs[k]) * float(d[0][i])
                W = W + t
        wh[i] = W * 0.5
    bits, vq = [], []
    for k, d in enumerate(drives):
        for (i, j), v in zip(d[1], d[2]):
            bits.append((i - 1, j - 1))
            vq.append((float(coefs[k]) * float(v)) * 0.25)
    return has_sites, wh, bits, np.array(vq, dtype=np.float64)


def diag_values(s, L, table):
    """d(s) for the configurations s (numpy uint64 / int64 array or torch int64 tensor), in the contract's order"""
    has_sites, wh, bits, vq = table
    if _is_torch(s):
        import torch
        d = torch.zeros(len(s), dtype=torch.float64, device=s.device)
        where = lambda c, v: torch.where(c, torch.full_like(d, v), torch.full_like(d, -v))     # noqa: E731
        bit = lambda k: ((s >> k) & 1) == 1                                                    # noqa: E731
    else:
        s = np.asarray(s).astype(np.int64)
        d = np.zeros(len(s))
        where = lambda c, v: np.where(c, v, -v)                                                # noqa: E731
        bit = lambda k: ((s >> k) & 1) == 1                                                    # noqa: E731
    if has_sites:
        for i in range(L):
            d = d + where(bit(i), float(wh[i]))
    for (bi, bj), q in zip(bits, vq):
        d = d + where(bit(bi) == bit(bj), float(q))
    return d


def drive_rows(h, psi, d):
    """h + d psi per component (h None: zeros): the kernel's one multiply and one add; complex vectors part by part"""
    if _is_torch(psi):
        import torch
        if psi.is_complex():
            hr = h.real if h is not None else torch.zeros_like(d)
            hi = h.imag if h is not None else torch.zeros_like(d)
            return torch.complex(hr + d * psi.real, hi + d * psi.imag)
        return (h if h is not None else torch.zeros_like(d)) + d * psi
    if np.iscomplexobj(psi):
        hr = h.real if h is not None else np.zeros_like(d)
        hi = h.imag if h is not None else np.zeros_like(d)
        out = np.empty(len(psi), dtype=np.complex128)
        out.real = hr + d * psi.real
        out.imag = hi + d * psi.imag
        return out
    return (h if h is not None else np.zeros_like(d)) + d * psi


# ---- schedules ----
S3 = math.sqrt(3.0)
A1, A2 = (3.0 - 2.0 * S3) / 12.0, (3.0 + 2.0 * S3) / 12.0


def magnus_schedule(functions, t0, dt, n_steps, order=4, swap=False):
    """(tau, coef[stage, k]); swap=True exchanges the two stages of every fourth-order step (a second-order method: the order test's
    negative control)"""
    K = len(functions)
    if order == 2:
        tau = np.full(n_steps, dt)
        coef = np.array([[f(t0 + (s + 0.5) * dt) for f in functions] for s in range(n_steps)]).reshape(n_steps, K)
        return tau, coef
    tau = np.full(2 * n_steps, dt / 2)
    coef = np.zeros((2 * n_steps, K))
    for s in range(n_steps):
        t = t0 + s * dt
        f1 = np.array([f(t + (0.5 - S3 / 6) * dt) for f in functions])
        f2 = np.array([f(t + (0.5 + S3 / 6) * dt) for f in functions])
        first, second = 2 * (A2 * f1 + A1 * f2), 2 * (A1 * f1 + A2 * f2)
        if swap:
            first, second = second, first
        coef[2 * s], coef[2 * s + 1] = first, second
    return tau, coef


def piecewise_schedule(segments):
    return np.array([float(d) for d, _ in segments]), np.array([np.atleast_1d(c) for _, c in segments], dtype=np.float64)


def dense_diag(states, L, drive):
    """the diagonal of D on the given states, by the plain definition (not the contract's order)"""
    s = np.asarray(states).astype(np.int64)
    sz = [((s >> i) & 1) - 0.5 for i in range(L)]
    d = np.zeros(len(s))
    if drive[0] is not None:
        for i in range(L):
            d += drive[0][i] * sz[i]
    for (i, j), v in zip(drive[1], drive[2]):
        d += v * sz[i - 1] * sz[j - 1]
    return d


def dense_stages(H0, diags, tau, coef, psi0):
    """psi after the stages exp(-i tau_s (H0 + sum_k coef[s, k] diag(diags[k]))), each by eigh; psi0 normalised first"""
    psi = np.asarray(psi0, dtype=np.complex128)
    psi = psi / np.linalg.norm(psi)
    for s in range(len(tau)):
        H = np.array(H0, dtype=np.float64)
        for k, dg in enumerate(diags):
            H = H + np.diag(coef[s][k] * dg)
        w, v = np.linalg.eigh(H)
        psi = v @ (np.exp(-1j * w * tau[s]) * (v.conj().T @ psi))
    return psi
