"""Entanglement across a chain cut.  The cut k separates sites 1..k (part A) from sites k+1..L (part B).  In a
fixed-nup sector the reduced density matrix is block diagonal in the number m of up spins in A, and every block is the Gram matrix
of a dense matrix that psi already is -- one batched Hermitian Gram kernel over row pointers, no copy of psi (sd_cut_gram).  The
library divides nothing by <psi|psi>; the functions here normalise by tr rho.  Eigenvalues are numpy's (`eigvalsh` per block).
psi may be a numpy array (host) or a torch CUDA tensor (stays on the device).  Blocks are keyed by m; the full basis has one block
with the key -1."""
import ctypes as C
import math
from collections import namedtuple

import numpy as np

from ._lib import ArgumentError, check, lib
from .hamiltonian import _bind_torch_stream, _dtype_code, _is_torch

_ip = C.POINTER(C.c_int)
_i64p = C.POINTER(C.c_int64)
SIDES = {"A": 0, "B": 1, "auto": 2}          # SD_CUT_A, SD_CUT_B, SD_CUT_AUTO
CUT_MAX_DIM = 16384                          # SD_CUT_MAX_DIM
CUT_BLOCK = np.dtype([("m", "<i4"), ("side", "<i4"), ("dA", "<i8"), ("dB", "<i8"), ("d", "<i8"), ("offset", "<i8")])      # sd_cut_block
CUT_ITEM = np.dtype([("block", "<i4"), ("ti", "<i4"), ("tj", "<i4"), ("tile", "<i4"), ("form", "<i4"), ("piece", "<i4"), ("ns", "<i4"),
                     ("reserved", "<i4"), ("k0", "<i8"), ("k1", "<i8"), ("slot", "<i8")])                                 # sd_cut_item

CutBlock = namedtuple("CutBlock", "m side dA dB d offset")


def _side_code(side, what):
    if side not in SIDES:
        raise ArgumentError(f"{what}: side must be 'A', 'B' or 'auto', got {side!r}")
    return SIDES[side]


def _cut_arg(model, cut, what):
    if isinstance(cut, bool) or int(cut) != cut or not 1 <= int(cut) <= model.L - 1:
        raise ArgumentError(f"{what}: the cut must be an integer in 1..L-1 = 1..{model.L - 1}, got {cut!r}")
    return int(cut)


def _blocks_raw(model, cut, side_code):
    ch = model.ctx.h if model.ctx is not None else None
    nb, ne = C.c_int(0), C.c_int64(0)
    check(lib().sd_cut_blocks(model.h, cut, side_code, None, 0, C.byref(nb), C.byref(ne)), ch)
    rec = np.zeros(nb.value, dtype=CUT_BLOCK)
    check(lib().sd_cut_blocks(model.h, cut, side_code, rec.ctypes.data, nb.value, C.byref(nb), C.byref(ne)), ch)
    return rec, ne.value


def cut_blocks(model, cut, side="auto"):
    """The blocks of the reduced density matrix across the cut (host only): a list of CutBlock(m, side, dA, dB, d, offset) in ascending
    m -- dA = C(k, m) and dB = C(L-k, nup-m) the dimensions of the two parts, side the one in effect ('A' or 'B'; 'auto' takes the
    smaller per block, a tie goes to A), d its dimension and offset the block's first matrix element in the packed output of
    sd_cut_gram.  The full basis has one block, m = -1."""
    cut = _cut_arg(model, cut, "cut_blocks")
    rec, _ = _blocks_raw(model, cut, _side_code(side, "cut_blocks"))
    return [CutBlock(int(r["m"]), "AB"[int(r["side"])], int(r["dA"]), int(r["dB"]), int(r["d"]), int(r["offset"])) for r in rec]


def cut_plan_info(model, cut, side="auto", dtype=np.complex128):
    """(work items, largest number of pieces of a summation range, workspace bytes) of the launch plan (host only)"""
    cut = _cut_arg(model, cut, "cut_plan_info")
    ch = model.ctx.h if model.ctx is not None else None
    ni, ns, wb = C.c_int64(0), C.c_int(0), C.c_int64(0)
    code = _dtype_code(np.empty(0, dtype=dtype))
    check(lib().sd_cut_plan_info(model.h, cut, _side_code(side, "cut_plan_info"), code, C.byref(ni), C.byref(ns), C.byref(wb)), ch)
    return ni.value, ns.value, wb.value


def cut_gram(psi, model, cut, side="auto"):
    """The un-normalised blocks {m: G_m} of sd_cut_gram: G_m = Psi_m Psi_m^dagger (side A, rows = the prefixes of popcount m in basis
    order) or Psi_m^T conj(Psi_m) (side B, rows = the suffix configurations in basis order).  A Float64 psi gives real symmetric
    blocks, a ComplexF64 psi Hermitian ones with an exactly real diagonal."""
    cut = _cut_arg(model, cut, "cut_gram")
    code = _side_code(side, "cut_gram")
    rec, n_el = _blocks_raw(model, cut, code)                    # every argument is refused here, before any launch
    if len(psi) != model.N:
        from ._lib import DimensionMismatch
        raise DimensionMismatch("length(psi) != the basis dimension")
    if _is_torch(psi):
        _bind_torch_stream(model, psi)
        dt = _dtype_code(psi)
        out = np.empty(n_el, dtype=np.complex128 if dt == 2 else np.float64)
        check(lib().sd_cut_gram_dev(model.ctx.h, model.h, dt, psi.data_ptr(), len(psi), cut, code, out.ctypes.data), model.ctx.h)
    else:
        x = np.ascontiguousarray(psi)
        if x.dtype not in (np.float64, np.complex128):
            x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
        out = np.empty(n_el, dtype=x.dtype)
        check(lib().sd_cut_gram(model.ctx.h, model.h, _dtype_code(x), x.ctypes.data, len(x), cut, code, out.ctypes.data), model.ctx.h)
    return {int(r["m"]): out[int(r["offset"]):int(r["offset"]) + int(r["d"]) ** 2].reshape(int(r["d"]), int(r["d"])) for r in rec}


def _sites_arg(model, sites, what):
    try:
        s = [int(x) for x in sites]
        ok = all(not isinstance(x, bool) and int(x) == x for x in sites)
    except (TypeError, ValueError):
        s, ok = [], False
    if not ok or not 1 <= len(s) <= model.L - 1 or len(set(s)) != len(s) or min(s) < 1 or max(s) > model.L:
        raise ArgumentError(f"{what}: the sites must be distinct integers in 1..L = 1..{model.L}, at least 1 and at most L - 1 of them, "
                            f"got {sites!r}")
    return np.ascontiguousarray(s, dtype=np.intc)


def subsystem_gram(psi, model, sites, side="auto"):
    """The un-normalised blocks {m: G_m} of the reduced density matrix of the listed sites (side 'A'), of the other sites ('B'), or
    block by block of the smaller of the two ('auto') -- sd_subsystem_gram: psi is permuted so that sites[j] becomes
    site j + 1 (one copy of psi from the context's pool) and goes through the Gram kernel of cut_gram at cut = len(sites).  Blocks,
    keys and row order are those of cut_gram(., ., len(sites), side) with sites[j] playing site j + 1; sites = 1..k in order is
    cut_gram(psi, model, k, side) bit for bit."""
    s = _sites_arg(model, sites, "subsystem_gram")
    code = _side_code(side, "subsystem_gram")
    rec, n_el = _blocks_raw(model, len(s), code)                 # every argument is refused here, before any launch
    if len(psi) != model.N:
        from ._lib import DimensionMismatch
        raise DimensionMismatch("length(psi) != the basis dimension")
    sp = s.ctypes.data_as(_ip)
    if _is_torch(psi):
        _bind_torch_stream(model, psi)
        dt = _dtype_code(psi)
        out = np.empty(n_el, dtype=np.complex128 if dt == 2 else np.float64)
        check(lib().sd_subsystem_gram_dev(model.ctx.h, model.h, dt, psi.data_ptr(), len(psi), sp, len(s), code, out.ctypes.data),
              model.ctx.h)
    else:
        x = np.ascontiguousarray(psi)
        if x.dtype not in (np.float64, np.complex128):
            x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
        out = np.empty(n_el, dtype=x.dtype)
        check(lib().sd_subsystem_gram(model.ctx.h, model.h, _dtype_code(x), x.ctypes.data, len(x), sp, len(s), code, out.ctypes.data),
              model.ctx.h)
    return {int(r["m"]): out[int(r["offset"]):int(r["offset"]) + int(r["d"]) ** 2].reshape(int(r["d"]), int(r["d"])) for r in rec}


def subsystem_density_matrix(psi, model, sites):
    """rho_S of the listed sites as its blocks {m: ndarray}, normalised so that the traces of all blocks sum to 1.  The rows of block
    m are the configurations of the listed sites with m up spins, in the basis order of the sector (len(sites), m) with sites[j]
    playing site j + 1 (the full basis: one block, key -1, rows by the integer value, sites[j] = bit j)."""
    G = subsystem_gram(psi, model, sites, "A")
    tr = _total_trace(G)
    return {m: g / tr for m, g in G.items()}


def dense_density_matrix(blocks, n_sites):
    """The blocks of subsystem_density_matrix (or of reduced_density_matrix(.., side='A')) as the 2^s x 2^s matrix in the
    computational basis of the s = n_sites listed sites: index = the configuration, sites[j] = bit j.  s <= 12."""
    import itertools
    s = int(n_sites)
    if not 1 <= s <= 12:
        raise ArgumentError(f"dense_density_matrix: n_sites must be in 1..12, got {n_sites!r}")
    first = next(iter(blocks.values()))
    rho = np.zeros((1 << s, 1 << s), dtype=np.asarray(first).dtype)
    for m, g in blocks.items():
        if m == -1:
            idx = np.arange(1 << s)
        else:
            idx = np.array([sum(1 << b for b in c) for c in itertools.combinations(range(s), m)], dtype=np.int64)
        if np.shape(g) != (len(idx), len(idx)):
            raise ArgumentError(f"dense_density_matrix: block {m} is not the side-A block of {s} sites")
        rho[np.ix_(idx, idx)] = g
    return rho


def subsystem_spectrum(psi, model, sites):
    """The eigenvalues of rho_S of the listed sites, per block: {m: descending float64 array}; they sum to 1 over all blocks.  Each
    block is taken on its smaller side (the listed sites or the rest: both have the same non-zero eigenvalues)."""
    return spectrum_from_blocks(subsystem_gram(psi, model, sites, "auto"))


def subsystem_entropy(psi, model, sites, q=1):
    """The entropy S_q of the listed sites with the rest of the system (see entropy_from_spectrum for q)"""
    _q_list(q, "subsystem_entropy")
    return entropy_from_spectrum(subsystem_spectrum(psi, model, sites), q)


def _disjoint(model, A, B, what):
    a, b = [int(x) for x in _sites_arg(model, A, what)], [int(x) for x in _sites_arg(model, B, what)]
    if set(a) & set(b):
        raise ArgumentError(f"{what}: A and B must be disjoint, both hold {sorted(set(a) & set(b))}")
    return a, b


def mutual_information(psi, model, A, B, q=1):
    """I_q(A:B) = S_q(A) + S_q(B) - S_q(A u B) of two disjoint site lists (q = 1: the von Neumann mutual information; psi is a
    pure state, so S(A u B) = 0 when the two lists cover the system)"""
    a, b = _disjoint(model, A, B, "mutual_information")
    _q_list(q, "mutual_information")
    S_ab = subsystem_entropy(psi, model, a + b, q) if len(a) + len(b) < model.L else 0.0
    return subsystem_entropy(psi, model, a, q) + subsystem_entropy(psi, model, b, q) - S_ab


def partial_transpose(rho, n_a, n_b):
    """rho^{T_B} of a dense 2^(n_a + n_b) matrix whose index is a + (b << n_a): the indices of B exchanged between bra and ket"""
    dA, dB = 1 << n_a, 1 << n_b
    return np.asarray(rho).reshape(dB, dA, dB, dA).transpose(2, 1, 0, 3).reshape(dA * dB, dA * dB)


def logarithmic_negativity(psi, model, A, B):
    """E_N = ln || rho_{A u B}^{T_B} ||_1 of two disjoint site lists.  rho_{A u B} comes from the device (subsystem_density_matrix);
    the partial transpose and `eigvalsh` run on the host on the dense matrix, so len(A) + len(B) <= 12."""
    a, b = _disjoint(model, A, B, "logarithmic_negativity")
    if len(a) + len(b) > 12:
        raise ArgumentError("logarithmic_negativity: len(A) + len(B) must be at most 12")
    if len(a) + len(b) > model.L - 1:
        raise ArgumentError("logarithmic_negativity: A and B together must leave at least one site out")
    rho = dense_density_matrix(subsystem_density_matrix(psi, model, a + b), len(a) + len(b))
    lam = np.linalg.eigvalsh(partial_transpose(rho, len(a), len(b)))
    return math.log(float(np.abs(lam).sum())) + 0.0


def two_site_density_matrix(psi, model, i, j):
    """The 4 x 4 density matrix of sites i and j in the computational basis: index = bit(i) + 2 bit(j) (1 = up)"""
    return dense_density_matrix(subsystem_density_matrix(psi, model, [i, j]), 2)


def _total_trace(G):
    tr = sum(float(np.trace(g).real) for g in G.values())
    if not tr > 0.0:
        raise ArgumentError("entanglement: the state has zero norm")
    return tr


def reduced_density_matrix(psi, model, cut, side="A"):
    """rho_A (side='A') or rho_B (side='B') across the cut as its blocks {m: ndarray}, normalised so that the traces of all blocks
    sum to 1"""
    G = cut_gram(psi, model, cut, side)
    tr = _total_trace(G)
    return {m: g / tr for m, g in G.items()}


def spectrum_from_blocks(G):
    """{m: Gram block, un-normalised} -> {m: eigenvalues of rho, descending, clipped at 0}, rho = (+)_m G_m / sum_m tr G_m"""
    tr = _total_trace(G)
    return {m: np.clip(np.linalg.eigvalsh(g)[::-1] / tr, 0.0, None) for m, g in G.items()}


def entanglement_spectrum(psi, model, cut):
    """The eigenvalues of the reduced density matrix across the cut, per block: {m: descending float64 array}; they sum to 1 over all
    blocks.  Each block is taken on its smaller side (both sides have the same non-zero eigenvalues)."""
    return spectrum_from_blocks(cut_gram(psi, model, cut, "auto"))


def _xlogx(p):
    p = p[p > 0.0]
    return float(-(p * np.log(p)).sum()) + 0.0


def _q_list(q, what):
    scalar = np.ndim(q) == 0
    qs = [float(x) for x in np.atleast_1d(np.asarray(q, dtype=np.float64))]
    for x in qs:
        if not x > 0.0:
            raise ArgumentError(f"{what}: q must be positive, got {x}")
    return scalar, qs


def entropy_from_spectrum(spectrum, q=1):
    """The Renyi entropy S_q = ln(sum lambda^q) / (1 - q) of a spectrum {m: eigenvalues} (or one array); q = 1 the von Neumann entropy
    -sum lambda ln lambda, q = math.inf the min-entropy -ln max lambda.  q: a positive scalar -> a float, a sequence -> an array."""
    scalar, qs = _q_list(q, "entropy_from_spectrum")
    lam = np.concatenate([np.asarray(v, dtype=np.float64).ravel() for v in spectrum.values()]) if isinstance(spectrum, dict) \
        else np.asarray(spectrum, dtype=np.float64).ravel()
    lam = lam[lam > 0.0]
    out = []
    for x in qs:
        if x == 1.0:
            out.append(_xlogx(lam))
        elif math.isinf(x):
            out.append(-math.log(lam.max()) + 0.0)
        else:
            out.append(math.log(float((lam ** x).sum())) / (1.0 - x) + 0.0)
    return out[0] if scalar else np.array(out)


def entanglement_entropy(psi, model, cut, q=1):
    """The entanglement entropy S_q between sites 1..cut and the rest (see entropy_from_spectrum for q)"""
    _q_list(q, "entanglement_entropy")
    return entropy_from_spectrum(entanglement_spectrum(psi, model, cut), q)


def entanglement_profile(psi, model, q=1):
    """S_q at every cut 1..L-1 -> a float64 array of L - 1 entries (q a scalar)"""
    if np.ndim(q) != 0:
        raise ArgumentError("entanglement_profile: q must be a scalar")
    if model.L < 2:
        raise ArgumentError("entanglement_profile: the chain has no cut")
    _q_list(q, "entanglement_profile")
    return np.array([entanglement_entropy(psi, model, k, q) for k in range(1, model.L)])


def schmidt_gap(psi, model, cut):
    """The difference of the two largest eigenvalues of the reduced density matrix (the largest itself when there is only one)"""
    lam = np.sort(np.concatenate(list(entanglement_spectrum(psi, model, cut).values())))[::-1]
    return float(lam[0] - (lam[1] if len(lam) > 1 else 0.0))


def symmetry_resolved_from_spectrum(spectrum):
    """{m: eigenvalues} -> dict(p={m: tr rho_m}, S={m: entropy of rho_m / p_m}, S_number, S_config, S_total) with S_number = -sum p ln p,
    S_config = sum p_m S_m and S_total = S_number + S_config, the von Neumann entropy"""
    p = {m: float(np.sum(v)) for m, v in spectrum.items()}
    S = {m: (_xlogx(np.asarray(v) / p[m]) if p[m] > 0.0 else 0.0) for m, v in spectrum.items()}
    S_number = _xlogx(np.array(list(p.values())))
    S_config = float(sum(p[m] * S[m] for m in p)) + 0.0
    return {"p": p, "S": S, "S_number": S_number, "S_config": S_config, "S_total": S_number + S_config}


def symmetry_resolved_entanglement(psi, model, cut):
    """The symmetry-resolved entanglement across the cut: the probabilities p_m = tr rho_m of finding m up spins in A, the entropies S_m
    of the normalised blocks, the number entropy S_number = -sum p ln p, the configurational entropy S_config = sum p_m S_m, and
    S_total = S_number + S_config = S_1 (see symmetry_resolved_from_spectrum)"""
    return symmetry_resolved_from_spectrum(entanglement_spectrum(psi, model, cut))
