"""Plain restatement of the two equal-time pair correlations, row by row (sites 1-based, site i <-> bit i - 1, nothing divided
by <psi|psi>):

    G_ij = <psi| S^+_i S^-_j |psi> = sum over the rows s with site j up and site i down of conj(psi[s']) psi[s],
           s' = s with the up spin moved from j to i;      G_ii = sum_s |psi[s]|^2 [site i up]
    Z_ij = <psi| S^z_i S^z_j |psi> = sum_s |psi[s]|^2 s_i(s) s_j(s),   s_i = +-1/2.

The partner row is the FULL rank of the flipped configuration (rows_ref.rank_t, proven on the CPU), or s' itself in the full
basis.  Every ordered pair is summed on its own: nothing here knows that G is Hermitian or Z symmetric.  torch tensors of any
device (numpy arrays are wrapped), so the sums over all rows of a sector of several million rows are formed where the vector
lives.  Shares nothing with the library or the oracle; tests/test_pair_ref_host.py proves it against Kronecker-product operators."""
import numpy as np

import rows_ref as RR


def _tensor(psi):
    import torch
    return psi if isinstance(psi, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(psi))


def configurations(N, L, nup, device):
    """configurations (int64) of rows 0..N-1: the reference order of the sector, or the row itself in the full basis"""
    import torch
    return RR.configurations_t(torch.arange(N, dtype=torch.int64, device=device), L, nup)


def g_pm(psi, s, L, nup, i, j):
    """G_ij of the vector psi (all rows) whose rows have the configurations s -> complex"""
    import torch
    up_i = ((s >> (i - 1)) & 1).to(torch.bool)
    up_j = ((s >> (j - 1)) & 1).to(torch.bool)
    if i == j:
        prob = psi.real * psi.real + psi.imag * psi.imag if psi.is_complex() else psi * psi
        return complex(prob[up_i].sum().item())
    rows = (up_j & ~up_i).nonzero().flatten()
    if len(rows) == 0:
        return 0j
    flipped = s[rows] ^ ((1 << (i - 1)) | (1 << (j - 1)))
    partner = flipped if nup is None else RR.rank_t(flipped, L, nup)
    return complex((torch.conj(psi[partner]) * psi[rows]).sum().item())


def z_zz(psi, s, i, j):
    """Z_ij -> float"""
    prob = psi.real * psi.real + psi.imag * psi.imag if psi.is_complex() else psi * psi
    return float((prob * RR.site_sz(s, i) * RR.site_sz(s, j)).sum().item())


def correlations(psi, L, nup, component, pairs=None, s=None):
    """component "+-" or "zz".  pairs None: the L x L complex128 matrix M[i-1, j-1], every ordered pair summed on its own;
    pairs a list of 1-based (i, j): {(i, j): complex}.  s: the rows' configurations when the caller has them already."""
    psi = _tensor(psi)
    if s is None:
        s = configurations(len(psi), L, nup, psi.device)
    one = (lambda i, j: g_pm(psi, s, L, nup, i, j)) if component == "+-" else (lambda i, j: complex(z_zz(psi, s, i, j)))
    assert component in ("+-", "zz")
    if pairs is not None:
        return {(i, j): one(i, j) for (i, j) in pairs}
    M = np.zeros((L, L), dtype=np.complex128)
    for i in range(1, L + 1):
        for j in range(1, L + 1):
            M[i - 1, j - 1] = one(i, j)
    return M
