"""Plain restatement of the S^z-basis statistics with numpy / torch; shares nothing with the library.

    w_s = |psi_s|^2 (re * re + im * im), nothing divided by <psi|psi>
    moments   : sum w, sum w ln w (0 where w = 0), max w and the lowest row that attains it, sum w^q
    counting  : P[k, m] = sum_s w_s [popcount(s & mask_k) = m], m = 0..L, by bincount with weights
    snapshots : the INTERVAL RULE.  With C the cumulative sum of w over all rows in row order and t_k = u_k C[N-1], u_k the hashed
                uniform of shot k, the row r returned for shot k must satisfy C[r-1] - delta <= t_k <= C[r] + delta, delta = 1e-12 C[N-1],
                and w[r] > 0.  (C[-1] = 0.)

The rows' configurations come from rows_ref.configurations_t (the combinadic order, proven on the CPU by tests/test_rows_ref_host.py).
torch tensors of any device (numpy arrays are wrapped), so the sums over all rows of a sector of several million rows are formed where
the vector lives.  tests/test_basis_stats_ref_host.py proves it against explicit loops over the basis and on exact states."""
import math

import numpy as np

import rows_ref as RR

SALT = 0x5AD5B1A5C0F1E2D3
_M = np.uint64


def _tensor(psi):
    import torch
    return psi if isinstance(psi, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(psi))


def weights(psi):
    psi = _tensor(psi)
    return psi.real * psi.real + psi.imag * psi.imag if psi.is_complex() else psi * psi


def configurations(N, L, nup, device):
    import torch
    return RR.configurations_t(torch.arange(N, dtype=torch.int64, device=device), L, nup)


# ---- moments ----
def moments(psi, qs=()):
    """{"W", "wlnw", "wmax", "argmax", "sums": [sum w^q for q in qs]} as Python floats / ints.  Whole-vector operations only (no
    index lists), so a sector past 2^31 rows goes through; the lowest row of the maximum is looked for slab by slab."""
    import torch
    w = weights(psi)
    one = torch.ones((), dtype=w.dtype, device=w.device)
    wlnw = torch.where(w > 0, w * torch.log(torch.where(w > 0, w, one)), torch.zeros((), dtype=w.dtype, device=w.device))
    wmax = w.max()
    argmax = -1
    for a in range(0, len(w), 1 << 30):
        hit = (w[a:a + (1 << 30)] == wmax).nonzero().flatten()
        if len(hit):
            argmax = a + int(hit[0].item())
            break
    return {"W": float(w.sum().item()), "wlnw": float(wlnw.sum().item()), "wmax": float(wmax.item()), "argmax": argmax,
            "sums": [float(torch.pow(w, float(q)).sum().item()) for q in qs]}       # 0^q = 0 for q > 0


def entropy(mom, q, k=None):
    """S_q from a `moments` result: q = 1 Shannon, math.inf -ln max p, else ln(sum p^q) / (1 - q) with sum w^q = mom["sums"][k]"""
    W = mom["W"]
    if q == 1:
        return math.log(W) - mom["wlnw"] / W
    if math.isinf(q):
        return -math.log(mom["wmax"] / W)
    return math.log(mom["sums"][k] / W ** q) / (1.0 - q)


# ---- counting ----
def site_mask(sites):
    m = 0
    for i in sites:
        m |= 1 << (i - 1)
    return m


def counting(psi, L, nup, masks, s=None, slab=1 << 26):
    """(K, L + 1) float64 numpy array of the raw sums for the K masks (Python ints).  s: the rows' configurations when the caller
    has them; otherwise they are formed slab by slab (`slab` rows at a time), so that a sector past 2^31 rows needs no second vector
    of its size; the slabs' bins are added in row order."""
    import torch
    psi = _tensor(psi)
    w = weights(psi)
    N = len(psi)
    out = np.zeros((len(masks), L + 1))
    for a in range(0, N, slab):
        b = min(N, a + slab)
        sl = s[a:b] if s is not None else RR.configurations_t(torch.arange(a, b, dtype=torch.int64, device=psi.device), L, nup)
        for k, mask in enumerate(masks):
            m = RR.popcount_t(sl & int(mask))
            out[k] += torch.bincount(m, weights=w[a:b], minlength=L + 1).cpu().numpy()
    return out


def reachable(L, nup, mask):
    """(m_min, m_max) of popcount(s & mask) over the basis, from the definition's two extremes"""
    a = bin(mask).count("1")
    if nup is None:
        return 0, a
    return max(0, nup - (L - a)), min(a, nup)


# ---- snapshots ----
def _mix(z):
    z = z + _M(0x9E3779B97F4A7C15)
    z = (z ^ (z >> _M(30))) * _M(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _M(27))) * _M(0x94D049BB133111EB)
    return z ^ (z >> _M(31))


def uniforms(seed, first, n):
    """u_k = (mix64((seed ^ SALT) ^ mix64(k)) >> 11) 2^-53 for k = first .. first + n - 1, in numpy uint64 arithmetic"""
    with np.errstate(over="ignore"):                         # the hash wraps modulo 2^64
        k = np.arange(n, dtype=_M) + _M(first)
        h = _mix((_M(seed) ^ _M(SALT)) ^ _mix(k))
    return (h >> _M(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def cumulative(psi):
    import torch
    return torch.cumsum(weights(psi), 0)


def snapshot_violation(rows, psi, seed, cum=None, w=None):
    """The interval rule for rows[k] = the row returned for shot k (all shots): (worst excess over the interval in units of
    delta = 1e-12 C[N-1] -- at most 1 passes --, number of returned rows with w = 0 or outside [0, N))"""
    import torch
    psi = _tensor(psi)
    w = weights(psi) if w is None else w
    C = torch.cumsum(w, 0) if cum is None else cum
    N = len(w)
    rows = np.asarray(rows, dtype=np.int64)
    bad = int(((rows < 0) | (rows >= N)).sum())
    r = torch.from_numpy(np.clip(rows, 0, N - 1)).to(w.device)
    total = float(C[N - 1].item())
    t = torch.from_numpy(uniforms(seed, 0, len(rows)) * total).to(w.device)
    hi = C[r]
    lo = torch.where(r > 0, C[torch.clamp(r - 1, min=0)], torch.zeros_like(hi))
    delta = 1e-12 * total
    excess = torch.maximum(lo - t, t - hi) / delta           # <= 0 inside the interval
    bad += int((w[r] <= 0).sum().item())
    return float(excess.max().item()) if len(rows) else 0.0, bad
