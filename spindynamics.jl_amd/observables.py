"""Mirror of the reference's Observables module (src/Observables.jl): device reductions over |psi|^2, the equal-time pair
correlation matrices <S^+_i S^-_j>, <S^z_i S^z_j> the reference does not return, and the bond operators and dimer
correlations <(S_i . S_j)(S_k . S_l)>.
psi may be a numpy array (host) or a torch CUDA tensor (stays on the device)."""
import ctypes as C

import numpy as np

from ._lib import ArgumentError, DimensionMismatch, check, lib
from .hamiltonian import _bind_torch_stream, _dtype_code, _is_torch

_dp = C.POINTER(C.c_double)


def _call(name, psi, model, nout):
    outs = [np.empty(model.L) for _ in range(nout)]
    ptrs = [o.ctypes.data_as(_dp) for o in outs]
    if _is_torch(psi):
        _bind_torch_stream(model, psi)
        check(getattr(lib(), name + "_dev")(model.ctx.h, model.h, _dtype_code(psi), psi.data_ptr(), len(psi), *ptrs), model.ctx.h)
    else:
        x = np.ascontiguousarray(psi)
        if x.dtype not in (np.float64, np.complex128):
            x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
        check(getattr(lib(), name)(model.ctx.h, model.h, _dtype_code(x), x.ctypes.data, len(x), *ptrs), model.ctx.h)
    return outs


def magnetization_per_site(psi, model):
    """magnetization_per_site(psi, model) -> <S^z_i>, i = 1..L -- src/Observables.jl:14-36"""
    return _call("sd_magnetization", psi, model, 1)[0]


def connected_correlations(psi, model):
    """connected_correlations(psi, model) -> C_r, r = 0..L-1 -- src/Observables.jl:44-94"""
    return _call("sd_connected_correlations", psi, model, 1)[0]


def structure_factor_Sq(psi, model):
    """structure_factor_Sq(psi, model) -> Dict{q => S(q)}, q = 2 pi (n-1)/L -- src/Observables.jl:100-109"""
    q, S = _call("sd_structure_factor", psi, model, 2)
    return {float(a): float(b) for a, b in zip(q, S)}


_PAIR = {"zz": 0, "+-": 1}     # SD_PAIR_ZZ, SD_PAIR_PM


def _pair_matrix(psi, model, component):
    """sd_pair_correlations[_dev]: the L x L complex matrix of SD_PAIR_ZZ / SD_PAIR_PM"""
    L = model.L
    out = np.empty((L, L), dtype=np.complex128)
    ptr = out.ctypes.data_as(_dp)
    if _is_torch(psi):
        _bind_torch_stream(model, psi)
        check(lib().sd_pair_correlations_dev(model.ctx.h, model.h, _dtype_code(psi), psi.data_ptr(), len(psi), _PAIR[component],
                                             ptr), model.ctx.h)
    else:
        x = np.ascontiguousarray(psi)
        if x.dtype not in (np.float64, np.complex128):
            x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
        check(lib().sd_pair_correlations(model.ctx.h, model.h, _dtype_code(x), x.ctypes.data, len(x), _PAIR[component], ptr),
              model.ctx.h)
    return out


def correlation_matrix(psi, model, component="zz", connected=False):
    """The L x L equal-time correlation matrix M[i-1, j-1] of psi, nothing divided by <psi|psi> (as the observables above):
      "zz": <S^z_i S^z_j> (float64);  "+-": <S^+_i S^-_j> (complex128, Hermitian: the one-body density matrix of the chain read
      as hard-core bosons);  "-+": <S^-_i S^+_j> = conj of "+-" off the diagonal, "+-" - 2 <S^z_i> on it (complex128);
      "xx": <S^x_i S^x_j> = <S^y_i S^y_j> = ("+-" + "-+") / 4 (float64).
    One pass of the pair kernel per call ("-+" and "xx" add the magnetisation pass for the diagonal).  "zz", "+-" and "-+" hold in
    a fixed-nup sector and in the full basis; "xx" leaves out <S^+ S^+>, which vanishes only in a sector, and raises ArgumentError
    for a full-basis model.  connected=True subtracts <S^z_i><S^z_j> from "zz" (the transverse one-point functions vanish in a
    sector, so the other components are their own connected parts there)."""
    if component not in ("zz", "+-", "-+", "xx"):
        raise ArgumentError(f"unknown component: {component}; expected \"zz\", \"+-\", \"-+\" or \"xx\"")
    if component == "xx" and model.nup is None:
        raise ArgumentError("component \"xx\" needs a fixed-nup sector: <S^+_i S^+_j> does not vanish in the full basis")
    if component == "zz":
        Z = _pair_matrix(psi, model, "zz").real.copy()
        if connected:
            sz = magnetization_per_site(psi, model)
            Z -= np.outer(sz, sz)
        return Z
    G = _pair_matrix(psi, model, "+-")
    if component == "+-":
        return G
    Gmp = G.conj()
    np.fill_diagonal(Gmp, np.diagonal(G) - 2.0 * magnetization_per_site(psi, model))
    if component == "-+":
        return Gmp
    return 0.25 * (G + Gmp).real


def static_structure_factor(psi, model, q, component="zz"):
    """S^{ab}(q) = (1/L) sum_ij e^{iq(j-i)} M^{ab}_ij for every q of the list, M = correlation_matrix(psi, model, component):
    S^{zz}(q) = |S^z_q psi|^2, S^{+-}(q) = |S^-_q psi|^2, S^{-+}(q) = |S^+_q psi|^2 with the phases and the 1/sqrt(L) of
    Sz_q_vector -- the equal-time sum rules int S^{ab}(q, w) dw of dynamical_structure_factor(..., component=...).  Not the
    connected, lag-periodic quantity of structure_factor_Sq.  Returns a float64 array over q."""
    M = correlation_matrix(psi, model, component)
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    ph = np.exp(1j * np.outer(qs, np.arange(model.L)))          # e^{iq r_j}, r_j = j - 1
    return np.einsum("qi,ij,qj->q", ph.conj(), M, ph).real / model.L


def momentum_distribution(psi, model, k=None):
    """n(k) = (1/L) sum_ij e^{ik(j-i)} <S^+_i S^-_j> of the chain read as hard-core bosons (b^+_i = S^+_i): the "+-" static
    structure factor.  k None: momenta(model)."""
    from .model import momenta
    return static_structure_factor(psi, model, momenta(model) if k is None else k, "+-")


# ---- bond operators and dimer correlations ----
def _host_vec(psi):
    x = np.ascontiguousarray(psi)
    if x.dtype not in (np.float64, np.complex128):
        x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    return x


def bond_operator(psi, model, i, j, xy=1.0, zz=1.0, out=None):
    """D_b psi for the bond b = (i, j) (1-based sites, i != j), D_b = xy/2 (S^+_i S^-_j + S^-_i S^+_j) + zz S^z_i S^z_j
    (xy = zz = 1: S_i . S_j) -> a vector of psi's kind and dtype.  out: where to write it (same kind, dtype and length; a device
    tensor must not be psi itself)."""
    if _is_torch(psi):
        import torch
        code = _dtype_code(psi)
        _bind_torch_stream(model, psi)
        if out is None:
            out = torch.empty_like(psi)
        elif not _is_torch(out) or out.dtype != psi.dtype or out.device != psi.device or not out.is_contiguous():
            raise ArgumentError("out must be a contiguous device tensor of psi's dtype on psi's device")
        elif len(out) != len(psi):
            raise DimensionMismatch("length(out) != length(psi)")
        check(lib().sd_bond_apply_dev(model.ctx.h, model.h, code, psi.data_ptr(), len(psi), int(i), int(j), float(xy), float(zz),
                                      out.data_ptr()), model.ctx.h)
        return out
    x = _host_vec(psi)
    if out is None:
        out = np.empty_like(x)
    elif not isinstance(out, np.ndarray) or out.dtype != x.dtype or not out.flags.c_contiguous:
        raise ArgumentError("out must be a contiguous numpy array of psi's dtype")
    elif len(out) != len(x):
        raise DimensionMismatch("length(out) != length(psi)")
    check(lib().sd_bond_apply(model.ctx.h, model.h, _dtype_code(x), x.ctypes.data, len(x), int(i), int(j), float(xy), float(zz),
                              out.ctypes.data), model.ctx.h)
    return out


def model_bonds(model):
    """the distinct site pairs of model.hopping_list, in list order (a pair and its reverse are one bond; i == j is none)"""
    seen, bonds = set(), []
    for i, j, _t in model.hopping_list:
        key = (min(i, j), max(i, j))
        if i != j and key not in seen:
            seen.add(key)
            bonds.append((int(i), int(j)))
    return bonds


def _dimer_call(psi, model, bonds, xy, zz):
    """sd_dimer_correlations[_dev] -> (D (B, B) complex128, e (B,), whether psi is complex)"""
    bl = model_bonds(model) if bonds is None else [(int(i), int(j)) for i, j in bonds]
    B = len(bl)
    flat = np.ascontiguousarray(np.array(bl, dtype=np.intc).reshape(-1))
    D, e = np.empty((B, B), dtype=np.complex128), np.empty(B)
    bp, Dp, ep = flat.ctypes.data_as(C.POINTER(C.c_int)), D.ctypes.data_as(_dp), e.ctypes.data_as(_dp)
    if _is_torch(psi):
        _bind_torch_stream(model, psi)
        check(lib().sd_dimer_correlations_dev(model.ctx.h, model.h, _dtype_code(psi), psi.data_ptr(), len(psi), bp, B, float(xy),
                                              float(zz), Dp, ep), model.ctx.h)
        return D, e, psi.is_complex()
    x = _host_vec(psi)
    check(lib().sd_dimer_correlations(model.ctx.h, model.h, _dtype_code(x), x.ctypes.data, len(x), bp, B, float(xy), float(zz), Dp,
                                      ep), model.ctx.h)
    return D, e, np.iscomplexobj(x)


def dimer_correlation_matrix(psi, model, bonds=None, connected=False, xy=1.0, zz=1.0):
    """The B x B dimer matrix D[a, b] = <psi| D_a D_b |psi> of a list of bonds (1-based site pairs; None: model_bonds(model)), D_b
    as in bond_operator, nothing divided by <psi|psi>.  One pass of the Gram kernel: no vector D_b psi is stored.  float64 for a
    real psi, complex128 (Hermitian to the bit; complex where bonds overlap) for a complex one.  connected=True subtracts
    e_a e_b, e = bond_energies -- for a normalised psi, like connected=True of correlation_matrix."""
    D, e, cplx = _dimer_call(psi, model, bonds, xy, zz)
    if connected:
        D = D - np.outer(e, e)
    return D if cplx else D.real.copy()


def bond_energies(psi, model, bonds=None, xy=1.0, zz=1.0):
    """e[b] = <psi| D_b |psi> for the bonds of the list (None: model_bonds(model)), from the same call as the dimer matrix."""
    return _dimer_call(psi, model, bonds, xy, zz)[1]


def dimer_structure_factor(psi, model, q, bonds=None, connected=False, xy=1.0, zz=1.0):
    """S_D(q) = (1/B) sum_ab e^{iq(x_b - x_a)} D_ab for every q of the list, x_b the position of bond b in the list and D =
    dimer_correlation_matrix(psi, model, bonds, connected, xy, zz).  Formed on the host.  Returns a float64 array over q."""
    D = dimer_correlation_matrix(psi, model, bonds, connected, xy, zz)
    qs = np.atleast_1d(np.asarray(q, dtype=np.float64))
    ph = np.exp(1j * np.outer(qs, np.arange(len(D))))
    return np.einsum("qa,ab,qb->q", ph.conj(), D, ph).real / len(D)
