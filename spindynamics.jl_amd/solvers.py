"""Mirrors of the reference's solver functions; each runs its whole recursion on
the device through one C-ABI call (include/spindyn.h, "recursion level").

The `applyH` argument of the reference functions is honoured: hamiltonian.apply_H selects the built-in fused
operator; any other callable `applyH(out, psi, model)` on torch device tensors is installed as the operator of the
recursion for the duration of the call (sd_ctx_set_apply_callback: the library calls it for out <- H psi and
applies its fused step as a second pass).
Where the reference draws a start vector from Julia's RNG (which cannot be
reproduced outside Julia) a `psi0=` / `seed=` keyword is offered instead of
`rng=`.
"""
import ctypes as C
import functools
import inspect

import numpy as np

from . import _lib
from ._lib import ArgumentError, DimensionMismatch, SD_C128, SD_F64, check, lib
from .hamiltonian import _bind_torch_stream, _is_torch, apply_H

_dp = C.POINTER(C.c_double)


def _with_operator(f):
    """Runs f with its `applyH` argument as the operator of `model`: nothing to do for the built-in apply_H, any other
    callable is installed as the recursion-level operator for the duration of the call; its own exception, if any, is
    what the caller sees."""
    sig = inspect.signature(f)

    @functools.wraps(f)
    def g(*args, **kw):
        ba = sig.bind(*args, **kw)
        applyH, model = ba.arguments["applyH"], ba.arguments["model"]
        if applyH is apply_H:
            return f(*args, **kw)
        if not callable(applyH):
            raise ArgumentError("applyH must be callable: applyH(out, psi, model)")
        ctx = model.ctx
        before = (ctx._apply_cb, ctx._apply_owner) if ctx is not None else (None, None)   # an operator installed with model.set_apply
        model.set_apply(applyH)
        try:
            return f(*args, **kw)
        except Exception:
            if getattr(model, "_apply_err", None) is not None:
                raise model._apply_err
            raise
        finally:
            model.set_apply(None)
            if before[0] is not None:
                ctx.install_apply(*before)
    return g


def _c128(x, n=None, name="vector"):
    x = np.ascontiguousarray(x, dtype=np.complex128)
    if n is not None and len(x) != n:
        raise DimensionMismatch(f"{name} has length {len(x)}, expected {n}")
    return x


def _vec(x):
    x = np.ascontiguousarray(x)
    if np.iscomplexobj(x):
        return x.astype(np.complex128, copy=False), SD_C128
    return x.astype(np.float64, copy=False), SD_F64


def _ptr(x):
    return None if x is None else x.ctypes.data


@_with_operator
def lanczos_extremal(applyH, model, lanc_m=100, tol=1e-12, psi0=None, seed=0, negate=False):
    """lanczos_extremal(applyH!, model; lanc_m, tol, rng) -> (Emin, Emax) -- src/Lanczos.jl:27-84"""
    p0 = None if psi0 is None else _c128(psi0, model.N, "psi0")
    lo, hi = C.c_double(), C.c_double()
    check(lib().sd_lanczos_extremal(model.ctx.h, model.h, int(lanc_m), float(tol), _ptr(p0), int(seed), int(bool(negate)),
                                    C.byref(lo), C.byref(hi)), model.ctx.h)
    return lo.value, hi.value


@_with_operator
def estimate_energy_bounds(applyH, model, lanc_m=80, psi0_a=None, psi0_b=None, seed=0):
    """estimate_energy_bounds(applyH!, model; lanc_m=80) -> (Emin, Emax) -- src/Lanczos.jl:255-271"""
    a = None if psi0_a is None else _c128(psi0_a, model.N, "psi0_a")
    b = None if psi0_b is None else _c128(psi0_b, model.N, "psi0_b")
    lo, hi = C.c_double(), C.c_double()
    check(lib().sd_energy_bounds(model.ctx.h, model.h, int(lanc_m), _ptr(a), _ptr(b), int(seed), C.byref(lo), C.byref(hi)),
          model.ctx.h)
    return lo.value, hi.value


@_with_operator
def lanczos_groundstate(applyH, model, lanc_m=100, tol=1e-12, orthogonalize_tol=1e-10, psi0=None, seed=0):
    """lanczos_groundstate(applyH!, model; lanc_m, tol, orthogonalize_tol, rng) -> (E0, psi_gs) -- src/Lanczos.jl:87-181"""
    p0 = None
    if psi0 is not None:
        p0 = np.ascontiguousarray(psi0, dtype=np.float64)
        if len(p0) != model.N:
            raise DimensionMismatch("psi0 length")
    E0, ma = C.c_double(), C.c_int()
    gs = np.empty(model.N, dtype=np.float64)
    check(lib().sd_lanczos_groundstate(model.ctx.h, model.h, int(lanc_m), float(tol), float(orthogonalize_tol),
                                       None if p0 is None else p0.ctypes.data_as(_dp), int(seed), C.byref(E0),
                                       gs.ctypes.data_as(_dp), C.byref(ma)), model.ctx.h)
    return E0.value, gs


@_with_operator
def lanczos_tridiag(applyH, model, v, lanc_m=100, tol=1e-12):
    """lanczos_tridiag(applyH!, model, v; lanc_m, tol) -> (alpha, beta, norm_v) -- src/Lanczos.jl:196-246"""
    v = _c128(v)
    n = len(v)
    m = max(min(int(lanc_m), n), 1)
    alpha, beta = np.zeros(m), np.zeros(max(m - 1, 1))
    me, nv = C.c_int(), C.c_double()
    check(lib().sd_lanczos_tridiag(model.ctx.h, model.h, v.ctypes.data, n, int(lanc_m), float(tol), alpha.ctypes.data_as(_dp),
                                   beta.ctypes.data_as(_dp), C.byref(me), C.byref(nv)), model.ctx.h)
    return alpha[: me.value].copy(), beta[: max(me.value - 1, 0)].copy(), nv.value


@_with_operator
def krylov_time_evolve(psi0, dt, applyH, model, kry_m=30):
    """krylov_time_evolve(psi0, dt, applyH!, model; kry_m) -> psi(t) ComplexF64, normalised -- src/TimeEvolution/Krylov.jl:136-192"""
    if _is_torch(psi0):          # device-resident state
        import torch
        if psi0.dtype not in (torch.float64, torch.complex128):
            raise ArgumentError("vectors must be float64 or complex128")
        _bind_torch_stream(model, psi0)
        out = torch.empty(len(psi0), dtype=torch.complex128, device=psi0.device)
        check(lib().sd_krylov_evolve_dev(model.ctx.h, model.h, SD_C128 if psi0.is_complex() else SD_F64, psi0.data_ptr(),
                                         len(psi0), float(dt), int(kry_m), out.data_ptr()), model.ctx.h)
        return out
    x, code = _vec(psi0)
    out = np.empty(len(x), dtype=np.complex128)
    check(lib().sd_krylov_evolve(model.ctx.h, model.h, code, x.ctypes.data, len(x), float(dt), int(kry_m), out.ctypes.data),
          model.ctx.h)
    return out


@_with_operator
def chebyshev_time_evolve(psi0, dt, applyH, model, cheb_n=100, Ebounds=(-1.0, 1.0), workspace=None):
    """chebyshev_time_evolve(psi0, dt, applyH!, model; cheb_n, Ebounds) -- src/TimeEvolution/Chebyshev.jl:61-124.
    psi0 must be complex (the reference's workspace is typed by psi0 and receives complex coefficients)."""
    if _is_torch(psi0):          # device-resident state: no PCIe per step of a time evolution
        import torch
        if psi0.dtype != torch.complex128:
            raise ArgumentError("chebyshev_time_evolve needs a ComplexF64 psi0 (as the reference does)")
        if int(cheb_n) < 1:
            raise AssertionError("cheb_n must be >= 1")
        _bind_torch_stream(model, psi0)
        out = torch.empty_like(psi0)
        check(lib().sd_chebyshev_evolve_dev(model.ctx.h, model.h, psi0.data_ptr(), len(psi0), float(dt), int(cheb_n),
                                            float(Ebounds[0]), float(Ebounds[1]), out.data_ptr()), model.ctx.h)
        return out
    if not np.iscomplexobj(psi0):
        raise ArgumentError("chebyshev_time_evolve needs a ComplexF64 psi0 (as the reference does)")
    if int(cheb_n) < 1:
        raise AssertionError("cheb_n must be >= 1")
    x = _c128(psi0)
    out = np.empty(len(x), dtype=np.complex128)
    check(lib().sd_chebyshev_evolve(model.ctx.h, model.h, x.ctypes.data, len(x), float(dt), int(cheb_n), float(Ebounds[0]),
                                    float(Ebounds[1]), out.ctypes.data), model.ctx.h)
    return out


def chebyshev_coeffs(cheb_n, a, b, dt):
    c = np.empty(int(cheb_n), dtype=np.complex128)
    check(lib().sd_chebyshev_coeffs(int(cheb_n), float(a), float(b), float(dt), c.ctypes.data_as(_dp)))
    return c


def chebyshev_terms(z):
    """The automatic real-time term count: the first k with k > |z| and |J_k(z)| < 2^-53, z = a dt (sd_chebyshev_terms).
    ArgumentError for |z| > 1e6."""
    n = C.c_int(0)
    check(lib().sd_chebyshev_terms(float(z), C.byref(n)))
    return n.value


def rescaling_from_bounds(Emin, Emax):
    """_rescaling_from_bounds -- src/KPM_Sqw.jl:13-17"""
    a, b = C.c_double(), C.c_double()
    check(lib().sd_kpm_rescaling_from_bounds(float(Emin), float(Emax), C.byref(a), C.byref(b)))
    return a.value, b.value


def get_rescaling_params(applyH, model, lanc_m=80, seed=0):
    """get_rescaling_params -- src/KPM_Sqw.jl:25-28"""
    return rescaling_from_bounds(*estimate_energy_bounds(applyH, model, lanc_m=lanc_m, seed=seed))


def get_kernel(M, kernel="jackson"):
    """get_kernel(M, kernel) -- src/KPM_Sqw.jl:131-145"""
    g = np.empty(int(M))
    check(lib().sd_kpm_kernel(int(M), _lib.KERNELS.get(kernel, 2), g.ctypes.data_as(_dp)))
    return g


@_with_operator
def compute_chebyshev_moments(applyH, phi, M, a, b, model):
    """compute_chebyshev_moments(apply_H!, phi, M, a, b, model) -- src/KPM_Sqw.jl:95-128"""
    phi = _c128(phi)
    mu = np.empty(int(M))
    check(lib().sd_kpm_moments(model.ctx.h, model.h, phi.ctypes.data, len(phi), int(M), float(a), float(b),
                               mu.ctypes.data_as(_dp)), model.ctx.h)
    return mu


def kpm_reconstruct(mu_damped, omega, a, b, E0):
    mu = np.ascontiguousarray(mu_damped, dtype=np.float64)
    om = np.ascontiguousarray(omega, dtype=np.float64)
    S = np.empty(len(om))
    check(lib().sd_kpm_reconstruct(mu.ctypes.data_as(_dp), len(mu), om.ctypes.data_as(_dp), len(om), float(a), float(b),
                                   float(E0), S.ctypes.data_as(_dp)))
    return S


def kpm_sw(phi, applyH, model, omega, a, b, E0, kpm_m=200, kernel="jackson"):
    """kpm_sw -- src/KPM_Sqw.jl:34-93"""
    mu = compute_chebyshev_moments(applyH, phi, kpm_m, a, b, model)
    mu *= get_kernel(kpm_m, kernel)
    return kpm_reconstruct(mu, omega, a, b, E0)


def kpm_sqw(psi0, model, q_list, omega, a=None, b=None, kpm_m=200, kernel="jackson", seed=0):
    """kpm_sqw(psi0, model, q_list, omega; a, b, kpm_m, kernel) -> Smat[Qn, W] -- src/KPM_Sqw.jl:191-256"""
    x, code = _vec(psi0)
    q = np.ascontiguousarray(q_list, dtype=np.float64)
    om = np.ascontiguousarray(omega, dtype=np.float64)
    S = np.empty((len(q), len(om)))
    have = a is not None and b is not None
    check(lib().sd_kpm_sqw(model.ctx.h, model.h, code, x.ctypes.data, len(x), q.ctypes.data_as(_dp), len(q),
                           om.ctypes.data_as(_dp), len(om), int(have), float(a) if have else 0.0, float(b) if have else 0.0,
                           int(kpm_m), _lib.KERNELS.get(kernel, 2), int(seed), S.ctypes.data_as(_dp)), model.ctx.h)
    return S


def spectral_from_tridiagonal(alpha, beta, norm_phi, E0, omega, eta=0.05, broaden="lorentz"):
    """spectral_from_tridiagonal -- src/LanczosSqw.jl:18-43"""
    if broaden not in _lib.BROADEN:
        raise ArgumentError(f"unknown broadening: {broaden}")
    al = np.ascontiguousarray(alpha, dtype=np.float64)
    be = np.ascontiguousarray(beta, dtype=np.float64)
    if len(be) == 0:
        be = np.zeros(1)
    om = np.ascontiguousarray(omega, dtype=np.float64)
    S = np.empty(len(om))
    check(lib().sd_spectral_from_tridiagonal(al.ctypes.data_as(_dp), be.ctypes.data_as(_dp), len(al), float(norm_phi), float(E0),
                                             om.ctypes.data_as(_dp), len(om), float(eta), _lib.BROADEN[broaden],
                                             S.ctypes.data_as(_dp)))
    return S


def lanczos_sqw(psi0, model, q_list, omega, lanc_m=200, eta=0.05, broaden="lorentz"):
    """lanczos_sqw -- src/LanczosSqw.jl:49-80"""
    if broaden not in _lib.BROADEN:
        raise ArgumentError(f"unknown broadening: {broaden}")
    x, code = _vec(psi0)
    q = np.ascontiguousarray(q_list, dtype=np.float64)
    om = np.ascontiguousarray(omega, dtype=np.float64)
    S = np.empty((len(q), len(om)))
    check(lib().sd_lanczos_sqw(model.ctx.h, model.h, code, x.ctypes.data, len(x), q.ctypes.data_as(_dp), len(q),
                               om.ctypes.data_as(_dp), len(om), int(lanc_m), float(eta), _lib.BROADEN[broaden],
                               S.ctypes.data_as(_dp)), model.ctx.h)
    return S


_COMPONENTS = {"+-": (2,), "-+": (1,), "xx": (2, 1)}


def _transverse(psi0, model, q_list, omega, component, run):
    """S^{+-} (op 2: S^-_q, sector nup - 1), S^{-+} (op 1: S^+_q, sector nup + 1) or S^{xx} = (S^{+-} + S^{-+}) / 4.  A
    component without a target sector (S^{+-} at nup = 0, S^{-+} at nup = L) has phi = 0: its rows are zero."""
    from .hamiltonian import _transverse_target
    if component not in _COMPONENTS:
        raise ArgumentError(f"unknown component: {component}; expected \"+-\", \"-+\" or \"xx\"")
    x, code = _vec(psi0)
    if len(x) != model.N:
        raise DimensionMismatch(f"psi0 has length {len(x)}, expected {model.N}")
    q = np.ascontiguousarray(q_list, dtype=np.float64)
    om = np.ascontiguousarray(omega, dtype=np.float64)
    parts = []
    for op in _COMPONENTS[component]:
        S = np.zeros((len(q), len(om)))
        dst = _transverse_target(model, op)
        if dst is not None:
            run(dst, op, x, code, q, om, S)
        parts.append(S)
    if component == "xx":
        return 0.25 * (parts[0] + parts[1])
    return parts[0]


def kpm_sqw_transverse(psi0, model, q_list, omega, component="+-", a=None, b=None, kpm_m=200, kernel="jackson", seed=0):
    """kpm_sqw with phi = S^-_q psi0 ("+-"), S^+_q psi0 ("-+"), or S^{xx} = S^{yy} = (S^{+-} + S^{-+}) / 4 ("xx") -> Smat[Qn, W].
    E0 = <psi0|H psi0> on psi0's sector; bounds (estimated per target sector when a, b are not given), moments and
    reconstruction on the target sector's H (model.adjacent_sector)."""
    have = a is not None and b is not None

    def run(dst, op, x, code, q, om, S):
        check(lib().sd_kpm_sqw_transverse(model.ctx.h, model.h, dst.h, op, code, x.ctypes.data, len(x), q.ctypes.data_as(_dp),
                                          len(q), om.ctypes.data_as(_dp), len(om), int(have), float(a) if have else 0.0,
                                          float(b) if have else 0.0, int(kpm_m), _lib.KERNELS.get(kernel, 2), int(seed),
                                          S.ctypes.data_as(_dp)), model.ctx.h)
    return _transverse(psi0, model, q_list, omega, component, run)


def lanczos_sqw_transverse(psi0, model, q_list, omega, component="+-", lanc_m=200, eta=0.05, broaden="lorentz"):
    """lanczos_sqw with phi = S^-_q psi0 ("+-"), S^+_q psi0 ("-+"), or their mean over the two ("xx", S^{xx} = S^{yy})
    -> Smat[Qn, W].  E0 as lanczos_sqw forms it, on psi0's sector; the tridiagonal on the target sector's H."""
    if broaden not in _lib.BROADEN:
        raise ArgumentError(f"unknown broadening: {broaden}")

    def run(dst, op, x, code, q, om, S):
        check(lib().sd_lanczos_sqw_transverse(model.ctx.h, model.h, dst.h, op, code, x.ctypes.data, len(x),
                                              q.ctypes.data_as(_dp), len(q), om.ctypes.data_as(_dp), len(om), int(lanc_m),
                                              float(eta), _lib.BROADEN[broaden], S.ctypes.data_as(_dp)), model.ctx.h)
    return _transverse(psi0, model, q_list, omega, component, run)


# ---- site-resolved KPM correlations (the quantity of the reference's src/TimeEvolution/KPM.jl) ----
_ip = C.POINTER(C.c_int)


def _host_vec(x):
    """psi0 as a host array and its dtype code; a torch tensor (host or device) is copied to the host."""
    if _is_torch(x):
        x = x.detach().cpu().numpy()
    return _vec(x)


def _sources(model, sources):
    src = np.arange(1, model.L + 1) if sources is None else np.atleast_1d(np.asarray(sources))
    if src.ndim != 1 or len(src) == 0 or not np.issubdtype(src.dtype, np.integer):
        raise ArgumentError("sources must be a non-empty list of 1-based site indices")
    return np.ascontiguousarray(src, dtype=np.int32)


def site_project(model, bra, ket):
    """out[i-1] = <bra| S^z_i |ket> = sum_rows conj(bra) s_i ket for every site i at once (one pass over both vectors, fixed
    summation order) -> complex array of L entries.  bra: Float64 or ComplexF64 (used as it is); ket: ComplexF64.  numpy
    arrays or torch device tensors (both of the same kind)."""
    out = np.empty(model.L, dtype=np.complex128)
    if _is_torch(bra) or _is_torch(ket):
        import torch
        if not (_is_torch(bra) and _is_torch(ket)):
            raise ArgumentError("bra and ket must both be numpy arrays or both torch device tensors")
        if bra.dtype not in (torch.float64, torch.complex128) or ket.dtype != torch.complex128:
            raise ArgumentError("bra must be float64 or complex128 and ket complex128")
        if len(bra) != len(ket):
            raise DimensionMismatch("length(bra) != length(ket)")
        _bind_torch_stream(model, bra)
        _bind_torch_stream(model, ket)
        check(lib().sd_site_project_dev(model.ctx.h, model.h, SD_C128 if bra.is_complex() else SD_F64, bra.data_ptr(),
                                        ket.data_ptr(), len(ket), out.ctypes.data_as(_dp)), model.ctx.h)
        return out
    b, code = _vec(bra)
    k = _c128(ket, len(b), "ket")
    check(lib().sd_site_project(model.ctx.h, model.h, code, b.ctypes.data, k.ctypes.data, len(k), out.ctypes.data_as(_dp)),
          model.ctx.h)
    return out


def kpm_site_moments(psi0, model, M, a, b, sources=None):
    """mu[s, n, i-1] = <psi0| S^z_i T_n(H~) S^z_j |psi0>, j = sources[s] (1-based; None: all sites), n = 0..M-1, H~ = (H - b)/a
    -> complex array (len(sources), M, L).  One recursion of M - 1 applies per source gives the moments against all L sites.
    psi0: numpy array or torch device tensor (stays on the device)."""
    src = _sources(model, sources)
    mu = np.empty((len(src), int(M), model.L), dtype=np.complex128)
    if _is_torch(psi0) and psi0.is_cuda:
        import torch
        if psi0.dtype not in (torch.float64, torch.complex128):
            raise ArgumentError("vectors must be float64 or complex128")
        _bind_torch_stream(model, psi0)
        check(lib().sd_kpm_site_moments_dev(model.ctx.h, model.h, SD_C128 if psi0.is_complex() else SD_F64, psi0.data_ptr(),
                                            len(psi0), src.ctypes.data_as(_ip), len(src), int(M), float(a), float(b),
                                            mu.ctypes.data_as(_dp)), model.ctx.h)
        return mu
    x, code = _host_vec(psi0)
    check(lib().sd_kpm_site_moments(model.ctx.h, model.h, code, x.ctypes.data, len(x), src.ctypes.data_as(_ip), len(src), int(M),
                                    float(a), float(b), mu.ctypes.data_as(_dp)), model.ctx.h)
    return mu


def kpm_reconstruct_signed(mu_damped, omega, a, b, E0):
    """kpm_reconstruct without the clamp at zero (off-diagonal C_ij is signed); complex moments: Re and Im separately."""
    mu = np.ascontiguousarray(mu_damped)
    if np.iscomplexobj(mu):
        return kpm_reconstruct_signed(mu.real, omega, a, b, E0) + 1j * kpm_reconstruct_signed(mu.imag, omega, a, b, E0)
    mu = np.ascontiguousarray(mu, dtype=np.float64)
    om = np.ascontiguousarray(omega, dtype=np.float64)
    out = np.empty(len(om))
    check(lib().sd_kpm_reconstruct_signed(mu.ctypes.data_as(_dp), len(mu), om.ctypes.data_as(_dp), len(om), float(a), float(b),
                                          float(E0), out.ctypes.data_as(_dp)))
    return out


def kpm_correlation_matrix(psi0, model, omega, sources=None, a=None, b=None, kpm_m=200, kernel="jackson", seed=0):
    """C[i-1, s, w] = <psi0| S^z_i delta(omega_w - (H - E0)) S^z_j |psi0>, j = sources[s] (None: all sites) -> complex array
    (L, len(sources), len(omega)).  Rescaling (estimated from `seed` when a, b are not given), kernel and E0 as kpm_sqw; the
    spectrum is NOT clamped at zero.  The reference's kpm_correlation_matrix (src/TimeEvolution/KPM.jl) is the model, with its
    defects left behind."""
    x, code = _host_vec(psi0)
    src = _sources(model, sources)
    om = np.ascontiguousarray(omega, dtype=np.float64)
    out = np.empty((model.L, len(src), len(om)), dtype=np.complex128)
    have = a is not None and b is not None
    check(lib().sd_kpm_site_correlations(model.ctx.h, model.h, code, x.ctypes.data, len(x), src.ctypes.data_as(_ip), len(src),
                                         om.ctypes.data_as(_dp), len(om), int(have), float(a) if have else 0.0,
                                         float(b) if have else 0.0, int(kpm_m), _lib.KERNELS.get(kernel, 2), int(seed),
                                         out.ctypes.data_as(_dp)), model.ctx.h)
    return out


def _shift_invariant(model):
    """Are the hop / zz / field lists of `model` invariant under the cyclic shift i -> i + 1 (mod L)?"""
    L = model.L

    def table(bonds):
        t = {}
        for i, j, J in bonds:
            if i == j:
                continue
            key = (min(i, j), max(i, j))
            t[key] = t.get(key, 0.0) + J
        return {k: v for k, v in t.items() if v != 0.0}

    def shifted(t):
        return {(min(i % L + 1, j % L + 1), max(i % L + 1, j % L + 1)): v for (i, j), v in t.items()}

    for bonds in (model.hopping_list, model.zz_list):
        t = table(bonds)
        if shifted(t) != t:
            return False
    f = np.asarray(model.onsite_field)
    return bool(np.all(f == f[0])) if len(f) else True


def kpm_sqw_sites(psi0, model, q_list, omega, a=None, b=None, kpm_m=200, kernel="jackson", seed=0,
                  translation_invariant=False, source=1, ti_tol=1e-6):
    """S^zz(q, omega) at every q of the list from the site-resolved moments -> Smat[Qn, W], the rows kpm_sqw returns.

    translation_invariant=False: one recursion per site (L x (kpm_m - 1) applies) for any psi0, any boundary and any number
    of momenta.  translation_invariant=True: ONE recursion from site `source` gives every momentum -- valid when H and psi0
    are invariant under the cyclic shift (the ground state of a periodic chain).  The lists are checked first (ArgumentError
    when the shift changes them), and the state through the invariance defect max |Im mu_n(q)| / (|psi0|^2 / 4) the library
    returns: ArgumentError above ti_tol (an invariant state sits at 1e-14, a violating one at >= 0.1)."""
    x, code = _host_vec(psi0)
    q = np.ascontiguousarray(q_list, dtype=np.float64)
    om = np.ascontiguousarray(omega, dtype=np.float64)
    if translation_invariant:
        if not _shift_invariant(model):
            raise ArgumentError("translation_invariant=True needs hop / zz / field lists that the cyclic shift leaves unchanged "
                                "(a periodic chain); use translation_invariant=False")
        src = _sources(model, [source])
    else:
        src = _sources(model, None)
    S = np.empty((len(q), len(om)))
    have = a is not None and b is not None
    defect = C.c_double(0.0)
    check(lib().sd_kpm_sqw_sites(model.ctx.h, model.h, code, x.ctypes.data, len(x), q.ctypes.data_as(_dp), len(q),
                                 om.ctypes.data_as(_dp), len(om), src.ctypes.data_as(_ip), len(src), int(bool(translation_invariant)),
                                 int(have), float(a) if have else 0.0, float(b) if have else 0.0, int(kpm_m),
                                 _lib.KERNELS.get(kernel, 2), int(seed), S.ctypes.data_as(_dp), C.byref(defect)), model.ctx.h)
    kpm_sqw_sites.last_defect = defect.value
    if translation_invariant and not defect.value <= ti_tol:
        raise ArgumentError(f"psi0 is not translation invariant: defect {defect.value:.3e} > ti_tol {ti_tol:.1e}; "
                            "use translation_invariant=False")
    return S


kpm_sqw_sites.last_defect = 0.0


def symtridiag_eig(d, e, vectors=True):
    d = np.ascontiguousarray(d, dtype=np.float64)
    e = np.ascontiguousarray(e, dtype=np.float64)
    n = len(d)
    if len(e) == 0:
        e = np.zeros(1)
    w = np.empty(n)
    z = np.empty((n, n), order="F") if vectors else None
    check(lib().sd_symtridiag_eig(n, d.ctypes.data_as(_dp), e.ctypes.data_as(_dp), w.ctypes.data_as(_dp),
                                  z.ctypes.data_as(_dp) if vectors else None))
    return (w, z) if vectors else w


def sym_eig(A):
    """eigen(Symmetric(A)) by cyclic Jacobi rotations (sd_sym_eig; n <= 128, the lower triangle is read) -> (w ascending, Z)."""
    A = np.asfortranarray(A, dtype=np.float64)
    n = A.shape[0]
    if A.ndim != 2 or A.shape[1] != n:
        raise DimensionMismatch("A must be square")
    w, Z = np.empty(n), np.empty((n, n), order="F")
    check(lib().sd_sym_eig(n, A.ctypes.data_as(_dp), w.ctypes.data_as(_dp), Z.ctypes.data_as(_dp)))
    return w, Z


@_with_operator
def lanczos_eigenpairs(applyH, model, k=4, basis_size=None, tol=1e-10, max_applies=None, confirm=True, psi0=None, seed=0,
                       vectors=True, dtype=None):
    """The lowest k eigenpairs by thick-restart Lanczos in (basis_size + 1) device vectors (sd_lanczos_eigenpairs)
    -> (E, X, info).  E: k ascending levels (info["converged"] of them when max_applies ended the run early); X: their states
    in the columns of an (N, k) array -- a torch tensor on the model's device when psi0 is one, otherwise numpy; None with
    vectors=False; info: converged, restarts, applies, basis_size, workspace_vectors, residuals, scale, next_level (the first level
    above the returned ones, or None).  confirm=True looks for further copies of degenerate levels from fresh random vectors and
    so returns every multiplicity; set it to False for an operator that projects onto a sector.  dtype: np.float64 or
    np.complex128; default psi0's, else float64 for the built-in operator and complex128 for a callable."""
    N = model.N
    on_dev = _is_torch(psi0)
    if dtype is None:
        if psi0 is not None:
            cplx = psi0.is_complex() if on_dev else np.iscomplexobj(psi0)
        else:
            cplx = applyH is not apply_H
    else:
        cplx = np.dtype(dtype) == np.complex128
        if not cplx and np.dtype(dtype) != np.float64:
            raise ArgumentError("dtype must be float64 or complex128")
    code, npdt = (SD_C128, np.complex128) if cplx else (SD_F64, np.float64)
    k = int(k)
    if basis_size is None:
        basis_size = min(N, max(2 * k + 8, 24))
    E, res = np.zeros(max(k, 1)), np.zeros(max(k, 1))
    info = _lib.sd_eigs_info()
    args = (int(basis_size), float(tol), int(max_applies) if max_applies is not None else 200000, int(bool(confirm)))
    if on_dev:
        import torch
        tdt = torch.complex128 if cplx else torch.float64
        if len(psi0) != N:
            raise DimensionMismatch(f"psi0 has length {len(psi0)}, expected {N}")
        p0 = psi0.to(tdt).contiguous()
        _bind_torch_stream(model, p0)
        Xt = torch.empty((max(k, 1), N), dtype=tdt, device=p0.device) if vectors else None
        check(lib().sd_lanczos_eigenpairs_dev(model.ctx.h, model.h, code, k, *args, p0.data_ptr(), int(seed), E.ctypes.data_as(_dp),
                                              Xt.data_ptr() if vectors else None, res.ctypes.data_as(_dp), C.byref(info)),
              model.ctx.h)
        X = Xt[: info.converged].T if vectors else None
    else:
        p0 = None
        if psi0 is not None:
            p0 = np.ascontiguousarray(psi0, dtype=npdt)
            if len(p0) != N:
                raise DimensionMismatch(f"psi0 has length {len(p0)}, expected {N}")
        Xn = np.zeros((N, max(k, 1)), dtype=npdt, order="F") if vectors else None
        check(lib().sd_lanczos_eigenpairs(model.ctx.h, model.h, code, k, *args, _ptr(p0), int(seed), E.ctypes.data_as(_dp),
                                          _ptr(Xn), res.ctypes.data_as(_dp), C.byref(info)), model.ctx.h)
        X = Xn[:, : info.converged] if vectors else None
    nc = info.converged
    out = {"converged": nc, "restarts": info.restarts, "applies": int(info.applies), "basis_size": info.basis_size,
           "workspace_vectors": info.workspace_vectors, "residuals": res[:nc].copy(), "scale": info.scale,
           "next_level": info.next_level if info.have_next_level else None}
    return E[:nc].copy(), X, out


def lowest_eigenpairs(model, k=4, **kw):
    """lanczos_eigenpairs with the built-in operator -> (E, X, info)."""
    return lanczos_eigenpairs(apply_H, model, k=k, **kw)


def spectral_gap(model, **kw):
    """(E0, E1 - E0, degeneracy of E0) from the two lowest levels with confirmation.  degeneracy counts the levels within
    tol * scale of E0 among the two returned levels and the next level, so it reads 1, 2 or 3 (3: at least threefold; ask
    lowest_eigenpairs for more levels).  For a degenerate E0 the second value is 0 to rounding; the gap above the multiplet is
    then next_level - E0 of lowest_eigenpairs(model, k=degeneracy)."""
    kw.setdefault("vectors", False)
    E, _, info = lowest_eigenpairs(model, k=min(2, model.N), confirm=True, **kw)
    levels = list(E) + ([info["next_level"]] if info["next_level"] is not None else [])
    eps = float(kw.get("tol", 1e-10)) * info["scale"]
    deg = sum(1 for e in levels if e - levels[0] <= eps)
    return float(E[0]), float(E[1] - E[0]) if len(E) > 1 else float("nan"), deg
