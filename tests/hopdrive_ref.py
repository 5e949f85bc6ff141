"""numpy / torch restatement of the hopping drives, for the tests.

A hopping drive is written here as a tuple ([(i, j), ...] 1-based, [z, ...] complex): B = sum_b (z_b S^+_i S^-_j + conj(z_b) S^-_i S^+_j).

1. effective_list: the list of one stage, as the library's host code forms it -- drive order, then list order, nothing merged, the
   bonds of a drive whose coefficient is exactly 0.0 dropped, weights x = c re, y = c im with one multiply each (y = 0.0 for a drive
   without imaginary parts, which the package passes with im = NULL); and the form of the call: complex iff some im of some drive
   passed is non-zero, whatever the coefficients.
2. hop_rows: acc + (B psi) row by row in the contract's order, bit for bit -- for each bond in list order whose two sites differ in s,
   v = psi[partner row]; real form acc.c + x v.c per component; complex form y' = +y (site i up) or -y (site j up), selected,
   t = (x v.re - y' v.im, x v.im + y' v.re), acc + t.  The partner rows are passed in (partner_rows: by a rank function, or idx ^ mask
   in the full basis).  Runs on numpy arrays or on torch tensors (eager torch does not contract a * b + c).
3. dense_hop: B as a dense matrix from oracle.dense.site_op, by the plain definition."""
import numpy as np


def _is_torch(x):
    return type(x).__module__.startswith("torch")


def has_imag(drive):
    return bool(np.any(np.imag(np.asarray(drive[1], dtype=np.complex128)) != 0.0))


def effective_list(drives, coefs):
    """(complex_form, [(bi, bj, x, y), ...]) of sum_k coefs[k] B_k: 0-based bits of sites i and j, in this orientation"""
    complex_form = any(has_imag(d) for d in drives)
    out = []
    for k, d in enumerate(drives):
        c = float(coefs[k])
        if c == 0.0:
            continue
        im = has_imag(d)
        for (i, j), z in zip(d[0], np.asarray(d[1], dtype=np.complex128)):
            out.append((i - 1, j - 1, c * float(z.real), c * float(z.imag) if im else 0.0))
    return complex_form, out


def partner_rows(s, idx, elist, rank=None):
    """per bond of the list the row of s with the bond's two sites exchanged (meaningful where they differ): rank(configurations), or
    idx ^ mask when rank is None (full basis)"""
    out = []
    for (bi, bj, _x, _y) in elist:
        mask = (1 << bi) | (1 << bj)
        if rank is None:
            out.append(idx ^ mask)
        else:                                                # rows whose two sites agree have no partner in the sector: their own row
            flip = (((s >> bi) ^ (s >> bj)) & 1) * mask
            out.append(rank(s ^ flip))
    return out


def hop_rows(acc, psi, s, partners, elist, complex_form):
    """acc + B psi in the contract's order.  acc None: zeros.  s: configurations (int64); partners: partner_rows' list."""
    tor = _is_torch(psi)
    if tor:
        import torch
        cplx = psi.is_complex()
        zeros = lambda: torch.zeros(len(psi), dtype=torch.float64, device=psi.device)         # noqa: E731
        full = lambda v: torch.full((len(psi),), v, dtype=torch.float64, device=psi.device)   # noqa: E731
        where = torch.where
        pr, pi = (psi.real, psi.imag) if cplx else (psi, None)
        ar = (acc.real.clone() if cplx else acc.clone()) if acc is not None else zeros()
        ai = (acc.imag.clone() if acc is not None else zeros()) if cplx else None
    else:
        s = np.asarray(s).astype(np.int64)
        cplx = np.iscomplexobj(psi)
        zeros = lambda: np.zeros(len(psi))                                                    # noqa: E731
        full = lambda v: np.full(len(psi), v)                                                 # noqa: E731
        where = np.where
        pr, pi = (np.ascontiguousarray(psi.real), np.ascontiguousarray(psi.imag)) if cplx else (psi, None)
        ar = (np.array(acc.real if cplx else acc, dtype=np.float64)) if acc is not None else zeros()
        ai = (np.array(acc.imag, dtype=np.float64) if acc is not None else zeros()) if cplx else None
    assert cplx or not complex_form, "a complex-form list needs a complex vector"
    n = len(psi)
    for (bi, bj, x, y), part in zip(elist, partners):
        ui, uj = ((s >> bi) & 1) == 1, ((s >> bj) & 1) == 1
        differ = ui != uj
        p = where(differ, part, part * 0)                    # rows that do not take part read row 0 and are masked out
        assert int(p.min()) >= 0 and int(p.max()) < n
        vr = pr[p]
        if not complex_form:
            ar = where(differ, ar + x * vr, ar)
            if cplx:
                ai = where(differ, ai + x * pi[p], ai)
        else:
            vi = pi[p]
            yp = where(ui, full(y), full(-y))               # selected: +y or -y, never a product
            tr = x * vr - yp * vi
            ti = x * vi + yp * vr
            ar = where(differ, ar + tr, ar)
            ai = where(differ, ai + ti, ai)
    if not cplx:
        return ar
    if tor:
        import torch
        return torch.complex(ar, ai)
    out = np.empty(n, dtype=np.complex128)
    out.real, out.imag = ar, ai
    return out


def dense_hop(D, L, drive, states=None):
    """B of one drive on the full basis (or on the given sector states) by the plain definition"""
    B = np.zeros((1 << L, 1 << L), dtype=np.complex128)
    for (i, j), z in zip(drive[0], np.asarray(drive[1], dtype=np.complex128)):
        pm = D.site_op(D.SP, i, L) @ D.site_op(D.SM, j, L)
        B += z * pm + np.conj(z) * pm.T
    if states is None:
        return B
    st = np.asarray(states).astype(np.int64)
    return B[np.ix_(st, st)]


def sector_hop(L, drive, states):
    """B of one drive on the given sector states, element by element from the configurations: for a sector whose 2^L full basis is
    too large for dense_hop (which the CPU tests hold it against at L = 8)"""
    st = [int(s) for s in np.asarray(states)]
    index = {s: k for k, s in enumerate(st)}
    B = np.zeros((len(st), len(st)), dtype=np.complex128)
    for (i, j), z in zip(drive[0], np.asarray(drive[1], dtype=np.complex128)):
        bi, bj = 1 << (i - 1), 1 << (j - 1)
        for col, s in enumerate(st):
            if (s & bj) and not (s & bi):                    # S^+_i S^-_j |s>: j up, i down
                B[index[s ^ (bi | bj)], col] += z
            if (s & bi) and not (s & bj):                    # S^-_i S^+_j |s>
                B[index[s ^ (bi | bj)], col] += np.conj(z)
    return B


def dense_stages_general(H0, ops, tau, coef, psi0):
    """psi after the stages exp(-i tau_s (H0 + sum_k coef[s, k] ops[k])) with dense Hermitian ops, each by eigh; psi0 normalised first"""
    psi = np.asarray(psi0, dtype=np.complex128)
    psi = psi / np.linalg.norm(psi)
    for s in range(len(tau)):
        H = np.array(H0, dtype=np.complex128)
        for k, op in enumerate(ops):
            if coef[s][k] != 0.0:
                H = H + coef[s][k] * op
        w, v = np.linalg.eigh(H)
        psi = v @ (np.exp(-1j * w * tau[s]) * (v.conj().T @ psi))
    return psi
