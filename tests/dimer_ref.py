"""Plain restatement of the bond operators and the dimer correlations, row by row (sites 1-based, site i <-> bit i - 1, nothing
divided by <psi|psi>).  For a bond b = (i, j), i != j, and two real weights

    D_b = xy/2 (S^+_i S^-_j + S^-_i S^+_j) + zz S^z_i S^z_j                (xy = zz = 1: S_i . S_j)
    (D_b psi)(s) = +-(zz/4) psi(s), + when the two sites agree in s, plus (xy/2) psi(s') when they differ,
                   s' = s with the two sites exchanged
    D_ab = <psi| D_a D_b |psi> = sum_s conj((D_a psi)(s)) (D_b psi)(s),    e_b = <psi| D_b |psi> = Re sum_s conj(psi(s)) (D_b psi)(s).

The partner row is the FULL rank of the exchanged configuration (rows_ref.rank_t, proven on the CPU), or s' itself in the full
basis.  Every vector D_b psi is formed and every ordered pair (a, b) is summed on its own with torch.vdot: nothing here knows that D
is Hermitian.  Each row of D_b psi is one multiply, and one multiply and one add, per component -- one torch call per operation, so
nothing is contracted.  torch tensors of any device (numpy arrays are wrapped).  Shares nothing with the library or the oracle;
tests/test_dimer_ref_host.py proves it against Kronecker-product operators."""
import numpy as np

import rows_ref as RR
from pair_ref import _tensor, configurations


def bond_rows(psi, s, L, nup, i, j, xy, zz):
    """D_b psi on all rows, b = (i, j); psi the whole vector, s its rows' configurations -> a tensor of psi's dtype"""
    import torch
    assert i != j and 1 <= i <= L and 1 <= j <= L
    cz, cx = float(zz) * 0.25, float(xy) * 0.5
    up_i = ((s >> (i - 1)) & 1).to(torch.bool)
    up_j = ((s >> (j - 1)) & 1).to(torch.bool)
    differ = up_i != up_j
    mask = (1 << (i - 1)) | (1 << (j - 1))
    exchanged = torch.where(differ, s ^ mask, s)
    partner = exchanged if nup is None else RR.rank_t(exchanged, L, nup)

    def part(x):
        c = torch.where(differ, torch.full_like(x, -cz), torch.full_like(x, cz))
        d = c * x
        return torch.where(differ, d + cx * x[partner], d)

    if psi.is_complex():
        return torch.complex(part(psi.real.contiguous()), part(psi.imag.contiguous()))
    return part(psi)


def gram(psi, L, nup, bonds, xy, zz, s=None, pairs=None):
    """(D, e) for the list of bonds (1-based site pairs).  pairs None: D the B x B complex128 matrix, every ordered pair (a, b) summed
    on its own; pairs a list of 0-based (a, b): D = {(a, b): complex}.  e: the B bond expectation values (float64).
    s: the rows' configurations when the caller has them already."""
    import torch
    psi = _tensor(psi)
    if s is None:
        s = configurations(len(psi), L, nup, psi.device)
    vecs = [bond_rows(psi, s, L, nup, i, j, xy, zz) for (i, j) in bonds]
    B = len(vecs)
    e = np.array([complex(torch.vdot(psi, v).item()).real for v in vecs])
    one = lambda a, b: complex(torch.vdot(vecs[a], vecs[b]).item())      # noqa: E731
    if pairs is not None:
        return {(a, b): one(a, b) for (a, b) in pairs}, e
    D = np.zeros((B, B), dtype=np.complex128)
    for a in range(B):
        for b in range(B):
            D[a, b] = one(a, b)
    return D, e
