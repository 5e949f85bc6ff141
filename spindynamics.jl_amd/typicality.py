"""Finite temperature by dynamical quantum typicality, with the spin current.

The reference's src/TimeEvolution/QuantumTypicality.jl advertises typicality_correlation_function but is never included
and calls undefined names; this is the quantity on this library's own definitions:

    psi_beta = exp(-beta H / 2) r,   num_r(t) = <psi_beta(t)| A |phi(t)>,   phi(t) = exp(-iHt) B psi_beta,
    den_r = |psi_beta|^2,            <A(t) B>_beta ~ sum_r num_r(t) / sum_r den_r.

Every call runs its whole loop on the device through one C-ABI call (include/spindyn.h).
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import ArgumentError, DimensionMismatch, SD_C128, SD_F64, check, lib
from .hamiltonian import _bind_torch_stream, _is_torch
from .model import Model
from .solvers import _c128, _vec

_dp = C.POINTER(C.c_double)
_KINDS = {"Sz": 0, "Szq": 1, "Sz_all": 2, "current": 3, "energy_current": 4}
_BOUNDARY = {"open": 0, "periodic": 1}
# sd_dterm (include/spindyn.h): the term c S^z_k j'_ij of a list of dressed bond currents
DTERM = np.dtype([("i", np.int32), ("j", np.int32), ("k", np.int32), ("c", np.float64)], align=True)


def chebyshev_imag_coeffs(a, tau, n_max=4096):
    """c_k = (2 - delta_k0) (-1)^k exp(-z) I_k(z), z = a tau, k = 0..n_used-1, n_used the first k with k > z and
    exp(-z) I_k(z) < 2^-53 exp(-z) I_0(z) (sd_chebyshev_imag_coeffs).  ArgumentError for z < 0 or z > 600."""
    c = np.empty(int(n_max))
    nu = C.c_int(0)
    check(lib().sd_chebyshev_imag_coeffs(int(n_max), float(a), float(tau), c.ctypes.data_as(_dp), C.byref(nu)))
    return c[: nu.value].copy()


def _method(method):
    if method not in _lib.EVOLVE:
        raise ArgumentError(f"unknown evolution method: {method}; expected \"chebyshev\" or \"krylov\"")
    return _lib.EVOLVE[method]


def _weights(model, weights):
    if weights is None:
        return None, None
    w = np.ascontiguousarray(weights, dtype=np.float64)
    if w.ndim != 1 or len(w) != len(model.hopping_list):
        raise ArgumentError(f"weights must have one entry per hop ({len(model.hopping_list)})")
    return w, w.ctypes.data_as(_dp)


def _torch_code(model, x):
    import torch
    if x.dtype not in (torch.float64, torch.complex128):
        raise ArgumentError("vectors must be float64 or complex128")
    _bind_torch_stream(model, x)
    return SD_C128 if x.is_complex() else SD_F64


def thermal_state(model, beta, r=None, seed=0, method="chebyshev", cheb_n=0, kry_m=30, Ebounds=None):
    """(exp(-beta H / 2) r / |.|, ln |exp(-beta H / 2) r|) for the start vector r as given (None: the counter-based normal
    stream of `seed`, sd_fill_randn_host, normalised).  numpy array in, numpy array out; torch device tensor in, device tensor out.
    method "chebyshev" (cheb_n = 0: automatic term count) or "krylov" -- one projection on kry_m Lanczos vectors, accurate
    only while beta/2 * (bandwidth) is small against kry_m.  Ebounds None: estimated (Chebyshev only)."""
    code = _method(method)
    if not float(beta) >= 0.0:
        raise ArgumentError("beta must be >= 0")
    lo, hi = (0.0, 0.0) if Ebounds is None else (float(Ebounds[0]), float(Ebounds[1]))
    ln = C.c_double(0.0)
    if r is not None and _is_torch(r):
        import torch
        dt = _torch_code(model, r)
        x = r
        out = torch.empty(len(x), dtype=torch.complex128, device=x.device)
        check(lib().sd_imag_evolve_dev(model.ctx.h, model.h, dt, x.data_ptr(), len(x), 0.5 * float(beta), code, int(cheb_n),
                                       int(kry_m), lo, hi, out.data_ptr(), C.byref(ln)), model.ctx.h)
        return out, ln.value
    if r is None:
        x = np.empty(model.N, dtype=np.complex128)
        check(lib().sd_fill_randn_host(x.ctypes.data_as(_dp), 2 * model.N, int(seed), 0))
        x = x / np.linalg.norm(x)
    else:
        x = _c128(r, model.N, "r")
    out = np.empty(model.N, dtype=np.complex128)
    check(lib().sd_imag_evolve(model.ctx.h, model.h, SD_C128, x.ctypes.data, len(x), 0.5 * float(beta), code, int(cheb_n),
                               int(kry_m), lo, hi, out.ctypes.data, C.byref(ln)), model.ctx.h)
    return out, ln.value


def spin_current(psi, model, weights=None):
    """J_w psi, J_w = sum_b w_b i t_b (S^+_i S^-_j - S^-_i S^+_j) over the model's hop list (weights None: ones, the total
    current; a unit vector: one bond's current) -> ComplexF64.  numpy arrays or torch device tensors."""
    w, wp = _weights(model, weights)
    if _is_torch(psi):
        import torch
        code = _torch_code(model, psi)
        out = torch.empty(len(psi), dtype=torch.complex128, device=psi.device)
        check(lib().sd_current_apply_dev(model.ctx.h, model.h, code, psi.data_ptr(), len(psi), wp, out.data_ptr()), model.ctx.h)
        return out
    x, code = _vec(psi)
    out = np.empty(len(x), dtype=np.complex128)
    check(lib().sd_current_apply(model.ctx.h, model.h, code, x.ctypes.data, len(x), wp, out.ctypes.data), model.ctx.h)
    return out


def current_expectation(bra, ket, model, weights=None):
    """<bra| J_w |ket> without forming J_w ket (one pass over both vectors, fixed summation order: the same call gives the same
    bits) -> complex.  bra Float64 or ComplexF64, ket ComplexF64; numpy arrays or torch device tensors (both of one kind)."""
    w, wp = _weights(model, weights)
    out = np.empty(2)
    if _is_torch(bra) or _is_torch(ket):
        import torch
        if not (_is_torch(bra) and _is_torch(ket)):
            raise ArgumentError("bra and ket must both be numpy arrays or both torch device tensors")
        if ket.dtype != torch.complex128:
            raise ArgumentError("ket must be complex128")
        if len(bra) != len(ket):
            raise DimensionMismatch("length(bra) != length(ket)")
        code = _torch_code(model, bra)
        _bind_torch_stream(model, ket)
        check(lib().sd_current_bracket_dev(model.ctx.h, model.h, code, bra.data_ptr(), ket.data_ptr(), len(ket), wp,
                                           out.ctypes.data_as(_dp)), model.ctx.h)
        return complex(out[0], out[1])
    b, code = _vec(bra)
    k = _c128(ket, len(b), "ket")
    check(lib().sd_current_bracket(model.ctx.h, model.h, code, b.ctypes.data, k.ctypes.data, len(k), wp, out.ctypes.data_as(_dp)),
          model.ctx.h)
    return complex(out[0], out[1])


def _boundary(boundary):
    if boundary not in _BOUNDARY:
        raise ArgumentError("boundary must be \"open\" or \"periodic\"")
    return _BOUNDARY[boundary]


def energy_current_terms(model, boundary="open"):
    """The energy current J_E = (i/2) sum_{a,b} (x_b - x_a) [h_a, h_b] of the model's lists as a list of terms c S^z_k j'_ij
    (sd_energy_current_terms): a structured array with fields i, j, k, c, merged, oriented i < j and sorted by (i, j, k); k = 0
    means no S^z factor.  boundary "periodic": positions are minimum images on a ring of L sites.  Host only: works on a model
    built with ctx=None."""
    per = _boundary(boundary)
    ch = model.ctx.h if model.ctx is not None else None
    n = C.c_int(0)
    check(lib().sd_energy_current_terms(model.h, per, None, 0, C.byref(n)), ch)
    out = np.zeros(n.value, dtype=DTERM)
    if n.value:
        check(lib().sd_energy_current_terms(model.h, per, out.ctypes.data, n.value, C.byref(n)), ch)
    return out


def _terms(model, terms, boundary):
    if terms is None:
        return energy_current_terms(model, boundary)
    if isinstance(terms, np.ndarray) and terms.dtype == DTERM:
        return np.ascontiguousarray(terms)
    out = np.zeros(len(terms), dtype=DTERM)
    for n, t in enumerate(terms):
        if len(t) != 4:
            raise ArgumentError("a term is (i, j, k, c)")
        out[n] = (int(t[0]), int(t[1]), int(t[2]), float(t[3]))
    return out


def energy_current(psi, model, terms=None, boundary="open"):
    """J psi for a list of terms (i, j, k, c) = c S^z_k i (S^+_i S^-_j - S^-_i S^+_j) -> ComplexF64; terms None: the model's energy
    current energy_current_terms(model, boundary).  A subset of that list is a local energy current.  numpy arrays or torch
    device tensors."""
    tl = _terms(model, terms, boundary)
    if _is_torch(psi):
        import torch
        code = _torch_code(model, psi)
        out = torch.empty(len(psi), dtype=torch.complex128, device=psi.device)
        check(lib().sd_dcurrent_apply_dev(model.ctx.h, model.h, code, psi.data_ptr(), len(psi), tl.ctypes.data, len(tl),
                                          out.data_ptr()), model.ctx.h)
        return out
    x, code = _vec(psi)
    out = np.empty(len(x), dtype=np.complex128)
    check(lib().sd_dcurrent_apply(model.ctx.h, model.h, code, x.ctypes.data, len(x), tl.ctypes.data, len(tl), out.ctypes.data),
          model.ctx.h)
    return out


def energy_current_expectation(bra, ket, model, terms=None, boundary="open"):
    """<bra| J |ket> for the list of `energy_current` without forming J ket (fixed summation order: the same call gives the same
    bits) -> complex.  bra Float64 or ComplexF64, ket ComplexF64; numpy arrays or torch device tensors (both of one kind)."""
    tl = _terms(model, terms, boundary)
    out = np.empty(2)
    if _is_torch(bra) or _is_torch(ket):
        import torch
        if not (_is_torch(bra) and _is_torch(ket)):
            raise ArgumentError("bra and ket must both be numpy arrays or both torch device tensors")
        if ket.dtype != torch.complex128:
            raise ArgumentError("ket must be complex128")
        if len(bra) != len(ket):
            raise DimensionMismatch("length(bra) != length(ket)")
        code = _torch_code(model, bra)
        _bind_torch_stream(model, ket)
        check(lib().sd_dcurrent_bracket_dev(model.ctx.h, model.h, code, bra.data_ptr(), ket.data_ptr(), len(ket), tl.ctypes.data,
                                            len(tl), out.ctypes.data_as(_dp)), model.ctx.h)
        return complex(out[0], out[1])
    b, code = _vec(bra)
    k = _c128(ket, len(b), "ket")
    check(lib().sd_dcurrent_bracket(model.ctx.h, model.h, code, b.ctypes.data, k.ctypes.data, len(k), tl.ctypes.data, len(tl),
                                    out.ctypes.data_as(_dp)), model.ctx.h)
    return complex(out[0], out[1])


def _operator(model, op, is_A):
    """(kind, param, weights array or None, weights pointer) of an operator descriptor"""
    if isinstance(op, str):
        op = (op,)
    if not isinstance(op, (tuple, list)) or len(op) == 0 or op[0] not in _KINDS:
        raise ArgumentError(f"unknown operator: {op!r}; expected (\"Sz\", site), (\"Szq\", q), \"Sz_all\", (\"current\", weights) "
                            "or (\"energy_current\", boundary)")
    name = op[0]
    if name == "Sz_all":
        if not is_A or len(op) != 1:
            raise ArgumentError("\"Sz_all\" is for operator_i only and takes no parameter")
        return 2, 0.0, None, None
    if name == "current":
        w, wp = _weights(model, op[1] if len(op) > 1 else None)
        return 3, 0.0, w, wp
    if name == "energy_current":
        if len(op) > 2:
            raise ArgumentError("(\"energy_current\", boundary) takes one parameter")
        return 4, float(_boundary(op[1] if len(op) > 1 else "open")), None, None
    if len(op) != 2:
        raise ArgumentError(f"operator {name!r} needs one parameter")
    if name == "Sz":
        if int(op[1]) != op[1] or not 1 <= int(op[1]) <= model.L:
            raise ArgumentError(f"site {op[1]} is outside 1..L = {model.L}")
        return 0, float(int(op[1])), None, None
    try:
        q = float(op[1])
    except (TypeError, ValueError):
        raise ArgumentError("(\"Szq\", q) takes one momentum") from None
    return 1, q, None, None


def dqt_sample(model, beta, operator_i, operator_j, t_range, method="chebyshev", r=None, seed=0, cheb_n=0, kry_m=30,
               Ebounds=None):
    """One sample of <A(t) B>_beta (sd_dqt_correlations) -> dict with `num` (complex, (nt,) or (nt, L) for "Sz_all": the
    numerators <psi_beta(t)| A |phi(t)> of the NORMALISED psi_beta), `log_norm` = ln |exp(-beta H/2) r| for the normalised r,
    `den` = exp(2 log_norm) and `energy` = <H> in psi_beta."""
    code = _method(method)
    Ak, Ap, Aw, Awp = _operator(model, operator_i, True)
    Bk, Bp, Bw, Bwp = _operator(model, operator_j, False)
    t = np.ascontiguousarray(t_range, dtype=np.float64)
    if t.ndim != 1 or len(t) == 0:
        raise ArgumentError("t_range must be a non-empty list of times")
    nA = model.L if Ak == 2 else 1
    num = np.empty((len(t), nA), dtype=np.complex128)
    den, en, ln = C.c_double(), C.c_double(), C.c_double()
    rp = None
    if r is not None:
        if _is_torch(r):
            r = r.detach().cpu().numpy()
        rr = _c128(r, model.N, "r")
        rp = rr.ctypes.data
    lo, hi = (0.0, 0.0) if Ebounds is None else (float(Ebounds[0]), float(Ebounds[1]))
    check(lib().sd_dqt_correlations(model.ctx.h, model.h, float(beta), rp, int(seed), Bk, Bp, Bwp, Ak, Ap, Awp,
                                    t.ctypes.data_as(_dp), len(t), code, int(cheb_n), int(kry_m), lo, hi,
                                    num.ctypes.data_as(_dp), C.byref(den), C.byref(en), C.byref(ln)), model.ctx.h)
    return {"num": num if Ak == 2 else num[:, 0], "den": den.value, "energy": en.value, "log_norm": ln.value}


class TypicalityResult(np.ndarray):
    """The complex array sum num / sum den with the per-sample pieces attached: `num` (n_samples, ...), `den` (n_samples,),
    `energy` (n_samples,), `log_norm` (n_samples,), `stderr` (the standard error of the per-sample ratios over the samples;
    zeros for one sample).  num and den are given relative to exp(2 * `log_shift`) so that nothing overflows."""


def _finish(nums, lns, ens):
    lns = np.asarray(lns, dtype=np.float64)
    shift = float(lns.max())
    den = np.exp(2.0 * (lns - shift))
    num = np.asarray(nums) * den.reshape((-1,) + (1,) * (np.asarray(nums).ndim - 1))
    val = num.sum(axis=0) / den.sum()
    out = np.asarray(val).view(TypicalityResult)
    out.num, out.den, out.energy, out.log_norm, out.log_shift = num, den, np.asarray(ens), lns, shift
    k = len(lns)
    ratios = np.asarray(nums)
    if k > 1:
        out.stderr = (np.std(ratios.real, axis=0, ddof=1) + 1j * np.std(ratios.imag, axis=0, ddof=1)) / math.sqrt(k)
    else:
        out.stderr = np.zeros_like(val)
    return out


def typicality_correlation_function(model, beta, operator_i, operator_j, t_range, method="chebyshev", n_samples=1, seed=0,
                                    r=None, all_sectors=False, **kw):
    """<A(t) B>_beta ~ sum_r num_r(t) / sum_r den_r over n_samples random start vectors (sample k: seed + k, or r[k] when `r` is a
    list of start vectors / one vector) -> complex array (len(t_range),), or (len(t_range), L) for operator_i = "Sz_all", with
    per-sample `num`, `den`, `energy` and the standard error `stderr` attached (TypicalityResult).

    Operators: ("Sz", site), ("Szq", q) (as operator_i: its adjoint), "Sz_all" (operator_i only), ("current", weights | None),
    ("energy_current", "open" | "periodic"): the model's energy current (energy_current_terms).
    method "chebyshev" or "krylov"; further keywords: cheb_n (0: automatic), kry_m, Ebounds.

    The model's basis is the trace: a sector model gives the canonical average at fixed S^z.  all_sectors=True sums the
    sectors nup = 0..L of the model's lists instead (grand-canonical at zero field beyond the model's own): sector s
    contributes N_s num and N_s den for its normalised start vector; r, when given, is then a list of L + 1 vectors (or a
    list of such lists, one per sample).  The typicality_correlation_function of the reference
    (src/TimeEvolution/QuantumTypicality.jl:33-91) is the model, with its defects left behind."""
    _method(method)
    _operator(model, operator_i, True)
    _operator(model, operator_j, False)
    if int(n_samples) < 1:
        raise ArgumentError("n_samples must be >= 1")
    unknown = set(kw) - {"cheb_n", "kry_m", "Ebounds"}
    if unknown:
        raise ArgumentError(f"unknown keyword: {sorted(unknown)}")
    nums, lns, ens = [], [], []
    if not all_sectors:
        rs = None
        if r is not None:
            rs = [r] if (_is_torch(r) or np.ndim(r) == 1) else list(r)
            if len(rs) != int(n_samples):
                raise ArgumentError("r must hold one start vector per sample")
        for k in range(int(n_samples)):
            s = dqt_sample(model, beta, operator_i, operator_j, t_range, method=method, r=None if rs is None else rs[k],
                           seed=int(seed) + k, **kw)
            nums.append(s["num"]); lns.append(s["log_norm"]); ens.append(s["energy"])
        return _finish(nums, lns, ens)
    L = model.L
    sectors = [Model(L, nup=s, hopping=model.hopping_list, onsite_field=model.onsite_field, zz=model.zz_list, ctx=model.ctx)
               for s in range(L + 1)]
    rs = None
    if r is not None:
        rs = [list(r)] if np.ndim(r[0]) == 1 else [list(x) for x in r]
        if len(rs) != int(n_samples) or any(len(x) != L + 1 for x in rs):
            raise ArgumentError("with all_sectors, r must hold L + 1 start vectors per sample")
    for k in range(int(n_samples)):
        parts = [dqt_sample(sec, beta, operator_i, operator_j, t_range, method=method, r=None if rs is None else rs[k][s],
                            seed=int(seed) + k, **kw) for s, sec in enumerate(sectors)]
        # sector s weighs N_s exp(2 ln_s); one common shift in the logarithms so that nothing overflows
        lw = np.array([math.log(sec.N) + 2.0 * p["log_norm"] for sec, p in zip(sectors, parts)])
        sh = lw.max()
        wgt = np.exp(lw - sh)
        nums.append(sum(w * p["num"] for w, p in zip(wgt, parts)) / wgt.sum())
        ens.append(float(sum(w * p["energy"] for w, p in zip(wgt, parts)) / wgt.sum()))
        lns.append(0.5 * (sh + math.log(wgt.sum())))
    return _finish(nums, lns, ens)


def thermal_energy(model, betas, n_samples=1, seed=0, method="chebyshev", Ebounds=None):
    """E(beta) = sum_r den_r E_r / sum_r den_r and ln Z_r(beta) = ln <r|exp(-beta H)|r> per sample, from successive
    imaginary-time steps of the same samples (betas non-decreasing) -> (E[len(betas)], lnZ[n_samples, len(betas)])."""
    import torch
    from .hamiltonian import apply_H
    code = _method(method)
    b = np.ascontiguousarray(betas, dtype=np.float64)
    if b.ndim != 1 or len(b) == 0 or b[0] < 0 or np.any(np.diff(b) < 0):
        raise ArgumentError("betas must be non-decreasing and >= 0")
    lo, hi = (0.0, 0.0) if Ebounds is None else (float(Ebounds[0]), float(Ebounds[1]))
    dev = torch.device("cuda", model.ctx.device)
    lnZ = np.zeros((int(n_samples), len(b)))
    En = np.zeros((int(n_samples), len(b)))
    for k in range(int(n_samples)):
        x = np.empty(model.N, dtype=np.complex128)
        check(lib().sd_fill_randn_host(x.ctypes.data_as(_dp), 2 * model.N, int(seed) + k, 0))
        psi = torch.from_numpy(x / np.linalg.norm(x)).to(dev)
        hpsi = torch.empty_like(psi)
        _bind_torch_stream(model, psi)
        ln_tot, prev = 0.0, 0.0
        for i, beta in enumerate(b):
            ln = C.c_double(0.0)
            check(lib().sd_imag_evolve_dev(model.ctx.h, model.h, SD_C128, psi.data_ptr(), len(psi), 0.5 * (beta - prev), code, 0,
                                           30, lo, hi, psi.data_ptr(), C.byref(ln)), model.ctx.h)
            prev = beta
            ln_tot += ln.value
            apply_H(hpsi, psi, model)
            lnZ[k, i] = 2.0 * ln_tot
            En[k, i] = float(torch.vdot(psi, hpsi).real / torch.vdot(psi, psi).real)
    w = np.exp(lnZ - lnZ.max(axis=0, keepdims=True))
    return (w * En).sum(axis=0) / w.sum(axis=0), lnZ
