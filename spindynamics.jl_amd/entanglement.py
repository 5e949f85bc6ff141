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
