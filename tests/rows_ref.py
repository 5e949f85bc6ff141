"""Plain restatements, row by row, of the operators whose kernels walk the basis: the combinadic order of a sector's rows, the
spin current, S^z_q, S^-_q / S^+_q between adjacent sectors, the site S^z signs and the single-site spin operators.  They share nothing with the library or the oracle.

Sites are 1-based, site i <-> bit i - 1; a sector's rows are ordered lexicographically over the sorted lists of up sites (site 1
first), the full basis by the configuration integer.  `unrank` / `rank` are numpy; the `*_t` functions are their torch ports and
work on tensors of any device, so the expected values of ALL rows of a sector of several million rows are formed where the vector
lives.  Configurations are int64 there (L <= 62).

Every floating-point result is built from single multiplies and adds of float64 tensors -- one torch call per operation, so
nothing is contracted into a fused multiply-add -- in the order the row loop states; tests/test_rows_ref_host.py proves the
current against tests/typicality_ref.py and S^-+_q against tests/transverse_ref.py, bit for bit."""
import math
from math import comb

import numpy as np


def binom_table(L, nup):
    """table[n, k] = C(n, k), n <= L, k <= nup"""
    return np.array([[comb(n, k) for k in range(nup + 1)] for n in range(L + 1)], dtype=np.int64)


# ---- the combinadic order: numpy ---------------------------------------------------------------------------------------
def unrank(rows, L, nup):
    """configurations (uint64, site i = bit i-1) of 0-based rows in the reference order: site 1 up first"""
    idx = rows.astype(np.int64).copy()
    r = np.full(idx.shape, nup, dtype=np.int64)
    s = np.zeros(idx.shape, dtype=np.uint64)
    table = binom_table(L, nup)
    for k in range(1, L + 1):
        c = np.where(r > 0, table[L - k, np.maximum(r - 1, 0)], 0)
        up = (r > 0) & (idx < c)
        s |= np.where(up, np.uint64(1) << np.uint64(k - 1), np.uint64(0))
        idx = np.where(up | (r == 0), idx, idx - c)
        r = r - up
    assert (r == 0).all()
    return s


def rank(s, L, nup):
    idx = np.zeros(s.shape, dtype=np.int64)
    r = np.full(s.shape, nup, dtype=np.int64)
    table = binom_table(L, nup)
    for k in range(1, L + 1):
        bit = ((s >> np.uint64(k - 1)) & np.uint64(1)).astype(bool)
        add = np.where(~bit & (r > 0), table[L - k, np.maximum(r - 1, 0)], 0)
        idx += add
        r = r - bit
    assert (r == 0).all()
    return idx


# ---- the combinadic order: torch ---------------------------------------------------------------------------------------
def unrank_t(rows, L, nup):
    """the torch port of `unrank`: rows an int64 tensor -> configurations as an int64 tensor on the same device"""
    import torch
    idx = rows.clone()
    r = torch.full_like(idx, nup)
    s = torch.zeros_like(idx)
    table = torch.as_tensor(binom_table(L, nup), device=rows.device)
    zero = torch.zeros_like(idx)
    for k in range(1, L + 1):
        c = torch.where(r > 0, table[L - k][torch.clamp(r - 1, min=0)], zero)
        up = (r > 0) & (idx < c)
        s = s | torch.where(up, torch.full_like(idx, 1 << (k - 1)), zero)
        idx = torch.where(up | (r == 0), idx, idx - c)
        r = r - up.to(torch.int64)
    assert bool((r == 0).all())
    return s


def rank_t(s, L, nup):
    """the torch port of `rank`"""
    import torch
    idx = torch.zeros_like(s)
    r = torch.full_like(s, nup)
    table = torch.as_tensor(binom_table(L, nup), device=s.device)
    zero = torch.zeros_like(s)
    for k in range(1, L + 1):
        bit = ((s >> (k - 1)) & 1).to(torch.bool)
        idx = idx + torch.where(~bit & (r > 0), table[L - k][torch.clamp(r - 1, min=0)], zero)
        r = r - bit.to(torch.int64)
    assert bool((r == 0).all())
    return idx


def configurations_t(rows, L, nup):
    """configurations of the given rows: the row index itself in the full basis (nup None)"""
    return rows.clone() if nup is None else unrank_t(rows, L, nup)


# ---- sampled rows of a large sector ---------------------------------------------------------------------------------------------
def sample_rows(model, n_random, seed):
    """rows of a model for a sampled comparison: the first and last 2048, both sides of up to 300 tile boundaries of the device
    plan (the only thing read from the model besides its size), and n_random random ones"""
    N = model.N
    rng = np.random.default_rng(seed)
    parts = [np.arange(0, min(N, 2048)), np.arange(max(0, N - 2048), N), rng.integers(0, N, n_random)]
    gb = []
    if model.device_path == "tiled":                      # tile boundaries of the device plan: rows on both sides of a few hundred of them
        _lb, gb, _ln = model.local_tiles()
    pick = rng.choice(len(gb), size=min(len(gb), 300), replace=False) if len(gb) else []     # (the per-row path has no tiles)
    for t in pick:
        parts.append(np.arange(max(0, gb[t] - 3), min(N, gb[t] + 3)))
    return np.unique(np.concatenate(parts).astype(np.int64))


# ---- the spin current ------------------------------------------------------------------------------------------------
def current_rows(psis, weight_sets, s, idx, L, nup, hop):
    """(J_w psi)[idx] for every vector of `psis` (float64 or complex128 tensors of the whole basis) and every weight list of
    `weight_sets` (None: ones) -> {(k, m): (re, im)} as float64 tensors, for vector k and weight list m.

    The row loop: zero accumulators; hops (i_b, j_b, t_b) in list order; a hop whose two sites are equal is skipped, and so is
    one whose two sites agree in the row; c = +-(w_b t_b), the product formed first, + when site i_b is up; re += c psi_re[partner],
    im += c psi_im[partner], the multiply and the add apart; the result is i (re + i im) = (-im, re).  The partner is the row of
    the configuration with both sites flipped: `rank_t` of it, or idx ^ mask in the full basis.  The partner of a hop is found
    once and serves every vector and weight list."""
    import torch
    parts = []
    for psi in psis:
        if psi.is_complex():
            parts.append((psi.real.contiguous(), psi.imag.contiguous()))
        else:
            parts.append((psi, None))
    zeros = lambda: torch.zeros(len(idx), dtype=torch.float64, device=idx.device)      # noqa: E731
    acc = {(k, m): [zeros(), zeros() if parts[k][1] is not None else None] for k in range(len(psis)) for m in range(len(weight_sets))}
    for b, (i, j, t) in enumerate(hop):
        if i == j:
            continue
        up_i = ((s >> (i - 1)) & 1).to(torch.bool)
        up_j = ((s >> (j - 1)) & 1).to(torch.bool)
        fl = up_i != up_j
        mask = (1 << (i - 1)) | (1 << (j - 1))
        if nup is None:
            partner = torch.where(fl, idx ^ mask, idx)
        else:
            partner = rank_t(torch.where(fl, s ^ mask, s), L, nup)
        gathered = [(pr[partner], None if pi is None else pi[partner]) for pr, pi in parts]
        for m, w in enumerate(weight_sets):
            wt = (1.0 if w is None else float(w[b])) * float(t)
            c = torch.where(up_i, torch.full_like(gathered[0][0], wt), torch.full_like(gathered[0][0], -wt))
            for k, (gr, gi) in enumerate(gathered):
                a = acc[(k, m)]
                a[0] = torch.where(fl, a[0] + c * gr, a[0])
                if gi is not None:
                    a[1] = torch.where(fl, a[1] + c * gi, a[1])
    out = {}
    for key, (re, im) in acc.items():
        out[key] = (torch.zeros_like(re) if im is None else -im, re)       # i (re + i im); a real psi: -0.0 == 0.0 under ==
    return out


# ---- S^z_q -------------------------------------------------------------------------------------------------------------
def szq_rows(psi, s, L, q):
    """(S^z_q psi) at the rows with configurations s: sq = sum_{r=0}^{L-1} exp(iqr) sz(site r+1), in site order, the phases from
    math.cos / math.sin; then (1/sqrt(L)) sq psi.  psi: the vector at those rows (float64 or complex128) -> complex128."""
    import torch
    sr = torch.zeros(len(s), dtype=torch.float64, device=s.device)
    si = torch.zeros_like(sr)
    for r in range(L):
        z = ((s >> r) & 1).to(torch.float64) - 0.5
        sr = sr + math.cos(q * r) * z
        si = si + math.sin(q * r) * z
    nf = 1.0 / math.sqrt(L)
    ar, ai = nf * sr, nf * si
    if psi.is_complex():
        xr, xi = psi.real, psi.imag
        return torch.complex(ar * xr - ai * xi, ar * xi + ai * xr)
    return torch.complex(ar * psi, ai * psi)


# ---- S^-_q / S^+_q between adjacent sectors ------------------------------------------------------------------------------
def spm_rows_t(psi, s_dst, L, nup_src, q, op):
    """(S^-_q psi) (op "minus") or (S^+_q psi) (op "plus") at the TARGET configurations s_dst (int64 tensor) -> (re, im), float64
    tensors on s_dst's device.  psi: the whole source vector (float64 or complex128) of sector nup_src, or of the full basis
    when nup_src is None (row = configuration).

    The row loop: zero accumulators; r = 0 .. L-1 ascending; a row whose bit r is 0 (minus) / 1 (plus) receives psi x at the
    row of the configuration with that bit flipped -- `rank_t` of it in the source sector -- as re += c_r x.re - s_r x.im,
    im += c_r x.im + s_r x.re (a real psi enters with x.im = 0), every product and sum a torch call of its own; then
    (nf re, nf im).  c_r, s_r = math.cos(q r), math.sin(q r) and nf = 1 / math.sqrt(L) are Python floats."""
    import torch
    want = 0 if op == "minus" else 1
    if psi.is_complex():
        pr, pi = psi.real.contiguous(), psi.imag.contiguous()
    else:
        pr, pi = psi, None
    ar = torch.zeros(len(s_dst), dtype=torch.float64, device=s_dst.device)
    ai = torch.zeros_like(ar)
    for r in range(L):
        sel = (((s_dst >> r) & 1) == want).nonzero().flatten()         # the rows this site contributes to
        if len(sel) == 0:
            continue
        part = s_dst[sel] ^ (1 << r)
        j = part if nup_src is None else rank_t(part, L, nup_src)
        xr = pr[j]
        xi = torch.zeros_like(xr) if pi is None else pi[j]
        c, s = math.cos(q * r), math.sin(q * r)
        a, b = c * xr, s * xi
        ar[sel] = ar[sel] + (a - b)
        a, b = c * xi, s * xr
        ai[sel] = ai[sel] + (a + b)
    nf = 1.0 / math.sqrt(L)
    return nf * ar, nf * ai


# ---- site S^z signs ----------------------------------------------------------------------------------------------------
def site_sz(s, site):
    """s_i = +-1/2 of site `site` in the configurations s (float64 tensor)"""
    import torch
    return ((s >> (site - 1)) & 1).to(torch.float64) - 0.5


def lag_sums(s, L):
    """sum_i s_i s_{i+r} (sites cyclic) of ONE configuration s (a Python int), r = 0..L-1: (L - 2 popcount(s ^ rot_r s)) / 4"""
    full = (1 << L) - 1
    out = []
    for r in range(L):
        rot = ((s >> r) | (s << (L - r))) & full
        out.append((L - 2 * bin(s ^ rot).count("1")) / 4)
    return np.array(out)


def popcount_t(x):
    """bits set in every entry of a non-negative int64 tensor: pair, nibble and byte sums, then the bytes added up"""
    x = x - ((x >> 1) & 0x5555555555555555)
    x = (x & 0x3333333333333333) + ((x >> 2) & 0x3333333333333333)
    x = (x + (x >> 4)) & 0x0F0F0F0F0F0F0F0F
    x = x + (x >> 8)
    x = x + (x >> 16)
    x = x + (x >> 32)
    return x & 0x7F


def lag_sums_t(s, L, r):
    """sum_i s_i s_{i+r} of every configuration of the int64 tensor s, as float64"""
    import torch
    full = (1 << L) - 1
    rot = s if r == 0 else ((s >> r) | (s << (L - r))) & full
    return (L - 2 * popcount_t(s ^ rot)).to(torch.float64) / 4


# ---- single-site spin operators of the full basis ------------------------------------------------------------------------
def spin_operator_rows(psi, site, op):
    """create_spin_operator(site, op)(psi) on the whole full basis, in gather form, psi a float64 or complex128 tensor.
    z: +-1/2 psi[row].  A source row with the site down sends psi to the row with it up under "plus" (nothing from an up source),
    the other way round under "minus"; "x" sends half of psi both ways; "y" sends -i/2 psi from a down source and +i/2 psi from
    an up source.  Row `row` therefore receives from row ^ bit only."""
    import torch
    rows = torch.arange(len(psi), dtype=torch.int64, device=psi.device)
    bit = 1 << (site - 1)
    up = (rows & bit) != 0
    if op == "z":
        return torch.where(up, 0.5 * psi, -0.5 * psi)
    src = psi[rows ^ bit]                                # the source row has the opposite bit
    zero = torch.zeros_like(src)
    if op == "plus":
        return torch.where(up, src, zero)
    if op == "minus":
        return torch.where(up, zero, src)
    if op == "x":
        return 0.5 * src
    assert op == "y" and psi.is_complex()
    re, im = src.real, src.imag
    # the destination is up: the source was down, -i/2 (a + ib) = (b/2, -a/2); else +i/2 (a + ib) = (-b/2, a/2)
    return torch.complex(torch.where(up, 0.5 * im, -(0.5 * im)), torch.where(up, -(0.5 * re), 0.5 * re))
