"""Driven dynamics: H(t) = H0 + sum_k f_k(t) D_k with H0 the model as built and diagonal drives

    D_k = sum_i w_{k,i} S^z_i + sum_b v_{k,b} S^z_{i_b} S^z_{j_b}

(a.c. and pulsed fields, field gradients, ramps and modulations of the anisotropy).  Not in the reference, whose propagators take a
time-independent H.  The time dependence is cut into stages with constant coefficients -- the midpoint rule or the fourth-order
commutator-free Magnus scheme (magnus_schedule), or the protocol itself where it is piecewise constant (piecewise_schedule) -- and
every stage is one Krylov propagation on H0 + sum_k c_k D_k (sd_driven_evolve): the built-in apply followed by one elementwise
kernel that adds d(s) psi and runs the Lanczos step's epilogue, with the state on the device from the first stage to the last.

Hopping drives sit beside the diagonal ones:

    B_k = sum_b (z_{k,b} S^+_{i_b} S^-_{j_b} + conj(z_{k,b}) S^-_{i_b} S^+_{j_b})

(modulated exchange, bond-selective quenches, and -- as the pair T_delta, J_delta of peierls_drives -- the Peierls phase of a vector
potential).  B_k is Hermitian, so the coefficient functions stay real.  drive_check, driven_apply, stage_evolve, driven_time_evolve
and instantaneous_energy take lists that mix both kinds in any order (sd_driven_hop_evolve: one gather kernel adds d(s) psi and
B psi to H0 psi and runs the Lanczos step's epilogue); a list without a HoppingDrive makes exactly the library calls it made before.

Sites are 1-based, as in build_model.  Vectors are numpy arrays or torch CUDA tensors, as everywhere in the package.
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from ._lib import ArgumentError, DimensionMismatch, SD_C128, SD_F64, check, lib
from .hamiltonian import _bind_torch_stream, _check_host, _dtype_code, _is_torch

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)

MAX_DRIVES = 16        # SD_DRIVE_MAX
MAX_DRIVE_BONDS = 128  # SD_DRIVE_MAX_BONDS, all drives of a call together
MAX_HOP_BONDS = 128    # SD_HOP_MAX_BONDS, all hopping drives of a call together


class DiagonalDrive:
    """D = sum_i site_weights[i-1] S^z_i + sum_b bond_weights[b] S^z_i S^z_j over bonds[b] = (i, j), sites 1-based.  Either part may be
    missing; a bond may repeat (its terms are added one after the other, not merged)."""

    def __init__(self, site_weights=None, bonds=None, bond_weights=None):
        self.site_weights = None if site_weights is None else np.ascontiguousarray(site_weights, dtype=np.float64).copy()
        if self.site_weights is not None and self.site_weights.ndim != 1:
            raise ArgumentError("site_weights must be a vector of L entries")
        bonds = [] if bonds is None else [(int(i), int(j)) for (i, j) in bonds]
        if bond_weights is None:
            bond_weights = np.ones(len(bonds))
        self.bond_weights = np.ascontiguousarray(bond_weights, dtype=np.float64).copy()
        if self.bond_weights.shape != (len(bonds),):
            raise ArgumentError("bond_weights must have one entry per bond")
        self.bonds = bonds
        self._zi = np.ascontiguousarray([b[0] for b in bonds], dtype=np.int32)
        self._zj = np.ascontiguousarray([b[1] for b in bonds], dtype=np.int32)

    def __repr__(self):
        return f"DiagonalDrive(sites={'no' if self.site_weights is None else len(self.site_weights)}, bonds={len(self.bonds)})"


def field_drive(model, weights=None):
    """sum_i w_i S^z_i; the uniform field sum_i S^z_i by default"""
    w = np.ones(model.L) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (model.L,):
        raise ArgumentError(f"weights must have L = {model.L} entries")
    return DiagonalDrive(site_weights=w)


def gradient_drive(model):
    """sum_i (i - (L + 1)/2) S^z_i: the tilt of a uniform field gradient about the chain's centre (the length-gauge electric field
    of the equivalent fermion chain)"""
    L = model.L
    return DiagonalDrive(site_weights=np.arange(1, L + 1, dtype=np.float64) - (L + 1) / 2.0)


def zz_drive(model, bonds=None, weights=None):
    """sum_b v_b S^z_i S^z_j; by default over the model's own zz bonds with weight 1 each (a modulation of the anisotropy)"""
    if bonds is None:
        bonds = [(i, j) for (i, j, _J) in model.zz_list]
    return DiagonalDrive(bonds=bonds, bond_weights=weights)


class HoppingDrive:
    """B = sum_b (weights[b] S^+_i S^-_j + conj(weights[b]) S^-_i S^+_j) over bonds[b] = (i, j), sites 1-based, i != j in either
    orientation; weights complex (ones by default).  A bond may repeat (its terms are added one after the other, not merged).  A
    drive whose weights are all real is passed to the library without imaginary parts: a call whose hopping drives are all such
    runs in real form (a float64 vector stays float64)."""

    def __init__(self, bonds, weights=None):
        bonds = [(int(i), int(j)) for (i, j) in bonds]
        if weights is None:
            weights = np.ones(len(bonds))
        self.weights = np.ascontiguousarray(weights, dtype=np.complex128).copy()
        if self.weights.shape != (len(bonds),):
            raise ArgumentError("weights must have one entry per bond")
        self.bonds = bonds
        self._i = np.ascontiguousarray([b[0] for b in bonds], dtype=np.int32)
        self._j = np.ascontiguousarray([b[1] for b in bonds], dtype=np.int32)
        self._re = np.ascontiguousarray(self.weights.real)
        self._im = np.ascontiguousarray(self.weights.imag) if np.any(self.weights.imag != 0.0) else None

    @property
    def is_real(self):
        return self._im is None

    def __repr__(self):
        return f"HoppingDrive(bonds={len(self.bonds)}, {'real' if self.is_real else 'complex'})"


def exchange_drive(model, bonds=None, weights=None):
    """sum_b w_b (S^+_i S^-_j + S^-_i S^+_j).  By default over the model's own hop bonds with their own amplitudes t_b, so that
    H0 + f(t) * exchange_drive(model) is the model with its exchange scaled by 1 + f(t): f is the relative modulation dJ/J."""
    if bonds is None:
        if weights is not None:
            raise ArgumentError("weights need their bonds")
        bonds = [(i, j) for (i, j, _t) in model.hopping_list]
        weights = [t for (_i, _j, t) in model.hopping_list]
    return HoppingDrive(bonds, weights)


def current_drive(model, weights=None):
    """J_w = sum_b w_b i t_b (S^+_i S^-_j - S^-_i S^+_j) over the model's hop list (weights None: ones, the total current): the
    operator of spin_current as a hopping drive, z_b = i w_b t_b."""
    n = len(model.hopping_list)
    w = np.ones(n) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    if w.shape != (n,):
        raise ArgumentError(f"weights must have one entry per hop bond ({n})")
    return HoppingDrive([(i, j) for (i, j, _t) in model.hopping_list], [1j * (w[b] * t) for b, (_i, _j, t) in enumerate(model.hopping_list)])


def _displacement(i, j, L, periodic):
    if not periodic:
        return j - i
    r = (j - i) % L
    if 2 * r == L:
        raise ArgumentError("a displacement of exactly +-L/2 on the ring has no minimum image")
    return r if 2 * r < L else r - L


def peierls_drives(model, boundary="open"):
    """The Peierls phase of a uniform vector potential A(t) on the model's hop bonds, convention

        t_b (e^{i A (j - i)} S^+_i S^-_j + h.c.)   for the bond (i, j, t_b),

    as hopping drives.  With delta = j - i the bond term is t_b (S^+ S^- + h.c.) + (cos(delta A) - 1) t_b (S^+ S^- + h.c.)
    + sin(delta A) i t_b (S^+ S^- - S^- S^+), so per distinct |delta| (bonds with delta < 0 are turned round)

        T_delta = sum_b t_b (S^+_i S^-_j + h.c.),    J_delta = sum_b i t_b (S^+_i S^-_j - S^-_i S^+_j)   (the spin current of the class)

    and H(t) = H0 + sum_delta [(cos(delta A(t)) - 1) T_delta + sin(delta A(t)) J_delta] exactly.  Returns (drives, displacements):
    drives = [T_d1, J_d1, T_d2, J_d2, ...] for displacements = [d1, d2, ...] ascending; peierls_functions(A, displacements) gives the
    coefficient functions in the same order.  boundary "periodic": delta is the minimum image on a ring of L sites; a displacement of
    exactly L/2 has none and is refused, as energy_current_terms refuses it."""
    if boundary not in ("open", "periodic"):
        raise ArgumentError("boundary must be \"open\" or \"periodic\"")
    classes = {}
    for (i, j, t) in model.hopping_list:
        d = _displacement(i, j, model.L, boundary == "periodic")
        if d < 0:
            i, j, d = j, i, -d
        if d == 0:
            continue
        classes.setdefault(d, []).append((i, j, t))
    drives, disp = [], sorted(classes)
    for d in disp:
        bonds = [(i, j) for (i, j, _t) in classes[d]]
        ts = np.array([t for (_i, _j, t) in classes[d]], dtype=np.float64)
        drives += [HoppingDrive(bonds, ts), HoppingDrive(bonds, 1j * ts)]
    return drives, disp


def peierls_functions(A, displacements):
    """The coefficient functions of peierls_drives' list for the vector potential A(t) (a callable): per displacement delta,
    t -> cos(delta A(t)) - 1 for T_delta and t -> sin(delta A(t)) for J_delta.

    Sign convention: the bond (i, j) carries e^{+i A (j - i)} on S^+_i S^-_j.  The unitary exp(-i A(t) sum_i i S^z_i) removes the phase
    and leaves the length-gauge Hamiltonian H0 + E(t) sum_i i S^z_i with E = -dA/dt: the same physics is the existing gradient_drive
    with f(t) = -dA/dt (for A(t0) = 0 the two states agree at every time at which A returns to 0; S^z observables agree always)."""
    fs = []
    for d in displacements:
        d = float(d)
        fs.append(lambda t, d=d: math.cos(d * float(A(t))) - 1.0)
        fs.append(lambda t, d=d: math.sin(d * float(A(t))))
    return fs


def _split(drives):
    """(drives as a list, positions of the diagonal drives, positions of the hopping drives)"""
    if isinstance(drives, (DiagonalDrive, HoppingDrive)):
        drives = [drives]
    drives = list(drives)
    di = [k for k, d in enumerate(drives) if isinstance(d, DiagonalDrive)]
    hi = [k for k, d in enumerate(drives) if isinstance(d, HoppingDrive)]
    if len(di) + len(hi) != len(drives):
        raise ArgumentError("drives must be DiagonalDrive or HoppingDrive objects")
    return drives, di, hi


def _pack_hops(hops):
    """(ctypes array of sd_hop_drive or None, KH): the array points into the drives' own arrays, which the caller keeps alive"""
    KH = len(hops)
    if KH == 0:
        return None, 0
    arr = (_lib.sd_hop_drive * KH)()
    for k, d in enumerate(hops):
        arr[k].n = len(d.bonds)
        if len(d.bonds):
            arr[k].i, arr[k].j = d._i.ctypes.data_as(_ip), d._j.ctypes.data_as(_ip)
            arr[k].re = d._re.ctypes.data_as(_dp)
            if d._im is not None:
                arr[k].im = d._im.ctypes.data_as(_dp)
    return arr, KH


def _permute_columns(coef, di, hi):
    """the caller's coefficient columns in the library's order: the diagonal drives first, then the hopping drives"""
    coef = np.asarray(coef, dtype=np.float64)
    return np.ascontiguousarray(coef[..., di + hi])


def _as_list(drives):
    if isinstance(drives, DiagonalDrive):
        return [drives]
    drives = list(drives)
    for d in drives:
        if not isinstance(d, DiagonalDrive):
            raise ArgumentError("drives must be DiagonalDrive objects")
    return drives


def _pack(model, drives):
    """(ctypes array of sd_drive or None, K): the array points into the drives' own arrays, which the caller keeps alive"""
    drives = _as_list(drives)
    K = len(drives)
    if K == 0:
        return None, 0, drives
    arr = (_lib.sd_drive * K)()
    for k, d in enumerate(drives):
        if d.site_weights is not None:
            if len(d.site_weights) != model.L:
                raise ArgumentError(f"drive {k}: site_weights has {len(d.site_weights)} entries, the model has L = {model.L} sites")
            arr[k].site_w = d.site_weights.ctypes.data_as(_dp)
        arr[k].n_zz = len(d.bonds)
        if len(d.bonds):
            arr[k].zz_i, arr[k].zz_j = d._zi.ctypes.data_as(_ip), d._zj.ctypes.data_as(_ip)
            arr[k].zz_w = d.bond_weights.ctypes.data_as(_dp)
    return arr, K, drives


def drive_check(model, drives):
    """Raises ArgumentError when the library would refuse the drives for this model (sd_drive_check, sd_hop_drive_check): more than 16
    drives, more than 128 zz terms or more than 128 hop terms in all, a site outside 1..L, a bond with i == j, a weight that is not
    finite."""
    drives, di, hi = _split(drives)
    ch = None if model.ctx is None else model.ctx.h
    arr, K, _keep = _pack(model, [drives[k] for k in di])
    check(lib().sd_drive_check(model.h, arr, K), ch)
    if hi:
        if len(drives) > MAX_DRIVES:
            raise ArgumentError(f"diagonal and hopping drives together must be at most {MAX_DRIVES}")
        hops = [drives[k] for k in hi]
        harr, KH = _pack_hops(hops)
        check(lib().sd_hop_drive_check(model.h, harr, KH), ch)


def _coefs(coefs, K):
    c = np.ascontiguousarray(np.atleast_1d(coefs), dtype=np.float64)
    if c.shape != (K,):
        raise ArgumentError(f"coefs must have one entry per drive ({K})")
    return c


def diagonal_apply(psi, model, drives, coefs, y=None, out=None):
    """(sum_k coefs[k] D_k) psi, plus y when given (y may be `out`).  Returns `out` (a new vector by default)."""
    arr, K, _keep = _pack(model, drives)
    c = _coefs(coefs, K)
    code = _dtype_code(psi)
    ctx = model.ctx
    if _is_torch(psi):
        import torch
        _bind_torch_stream(model, psi)
        if out is None:
            out = torch.empty_like(psi)
        if _dtype_code(out) != code or (y is not None and _dtype_code(y) != code):
            raise ArgumentError("psi, y and out must have the same element type")
        if len(out) != len(psi) or (y is not None and len(y) != len(psi)):
            raise DimensionMismatch("psi, y and out must have the same length")
        check(lib().sd_diag_apply_dev(ctx.h, model.h, code, psi.data_ptr(), len(psi), arr, K, c.ctypes.data_as(_dp),
                                      None if y is None else y.data_ptr(), out.data_ptr()), ctx.h)
        return out
    _check_host(psi, "psi")
    if out is None:
        out = np.empty_like(psi)
    _check_host(out, "out")
    if y is not None:
        _check_host(y, "y")
    if out.dtype != psi.dtype or (y is not None and y.dtype != psi.dtype):
        raise ArgumentError("psi, y and out must have the same element type")
    if len(out) != len(psi) or (y is not None and len(y) != len(psi)):
        raise DimensionMismatch("psi, y and out must have the same length")
    check(lib().sd_diag_apply(ctx.h, model.h, code, psi.ctypes.data, len(psi), arr, K, c.ctypes.data_as(_dp),
                              None if y is None else y.ctypes.data, out.ctypes.data), ctx.h)
    return out


def driven_apply(out, psi, model, drives, coefs):
    """out = (H0 + sum_k coefs[k] D_k) psi: the built-in apply and the drive kernel behind it (sd_driven_apply).  With drives and
    coefs bound -- functools.partial, or a lambda (out, psi, m) -- it is an `applyH=` for every solver that takes one."""
    drives, di, hi = _split(drives)
    arr, K, _keep = _pack(model, [drives[k] for k in di])
    code = _dtype_code(psi)
    if _dtype_code(out) != code:
        raise ArgumentError("out and psi must have the same element type")
    if len(out) != len(psi):
        raise DimensionMismatch("length(out) != length(psi)")
    ctx = model.ctx
    if hi:
        hops = [drives[k] for k in hi]
        harr, KH = _pack_hops(hops)
        c = _permute_columns(_coefs(coefs, K + KH), di, hi)
        if _is_torch(psi):
            _bind_torch_stream(model, psi)
            _bind_torch_stream(model, out)
            check(lib().sd_driven_hop_apply_dev(ctx.h, model.h, code, psi.data_ptr(), len(psi), arr, K, harr, KH, c.ctypes.data_as(_dp),
                                                out.data_ptr()), ctx.h)
        else:
            _check_host(out, "out"); _check_host(psi, "psi")
            check(lib().sd_driven_hop_apply(ctx.h, model.h, code, psi.ctypes.data, len(psi), arr, K, harr, KH, c.ctypes.data_as(_dp),
                                            out.ctypes.data), ctx.h)
        return out
    c = _coefs(coefs, K)
    if _is_torch(psi):
        _bind_torch_stream(model, psi)
        _bind_torch_stream(model, out)
        check(lib().sd_driven_apply_dev(ctx.h, model.h, code, psi.data_ptr(), len(psi), arr, K, c.ctypes.data_as(_dp), out.data_ptr()),
              ctx.h)
    else:
        _check_host(out, "out"); _check_host(psi, "psi")
        check(lib().sd_driven_apply(ctx.h, model.h, code, psi.ctypes.data, len(psi), arr, K, c.ctypes.data_as(_dp), out.ctypes.data),
              ctx.h)
    return out


def _values(functions, t):
    return [float(f(t)) if callable(f) else float(f) for f in functions]


SQRT3 = math.sqrt(3.0)
GAUSS_LO, GAUSS_HI = 0.5 - SQRT3 / 6.0, 0.5 + SQRT3 / 6.0           # the two Gauss points of a step, in units of dt
ALPHA_1, ALPHA_2 = (3.0 - 2.0 * SQRT3) / 12.0, (3.0 + 2.0 * SQRT3) / 12.0


def magnus_schedule(functions, t0, dt, n_steps, order=4):
    """(tau, coef) of n_steps steps of length dt from t0 for the coefficient functions f_k(t) (callables, or numbers for constants):
    tau[s] the duration of stage s, coef[s, k] the constant coefficient of D_k during it.
      order 2: the midpoint rule, one stage per step, tau = dt, c_k = f_k(t + dt/2);
      order 4: the commutator-free Magnus scheme of Alvermann and Fehske (J. Comput. Phys. 230, 5930 (2011), CF4:2), two stages per
               step of tau = dt/2 each.  With the Gauss points t1, t2 = t + (1/2 -+ sqrt(3)/6) dt and alpha1, alpha2 = (3 -+ 2 sqrt 3)/12
               the earlier stage has c_k = 2 (alpha2 f_k(t1) + alpha1 f_k(t2)), the later one c_k = 2 (alpha1 f_k(t1) + alpha2 f_k(t2));
               the factor 2 because alpha1 + alpha2 = 1/2 is what multiplies H0."""
    functions = list(functions)
    K, n = len(functions), int(n_steps)
    if order not in (2, 4):
        raise ArgumentError("order must be 2 or 4")
    if n < 1:
        raise ArgumentError("n_steps must be at least 1")
    per = 1 if order == 2 else 2
    tau = np.full(per * n, float(dt) / per)
    coef = np.zeros((per * n, K))
    for s in range(n):
        t = float(t0) + s * float(dt)
        if order == 2:
            coef[s] = _values(functions, t + 0.5 * dt)
        else:
            f1 = np.array(_values(functions, t + GAUSS_LO * dt))
            f2 = np.array(_values(functions, t + GAUSS_HI * dt))
            coef[2 * s] = 2.0 * (ALPHA_2 * f1 + ALPHA_1 * f2)
            coef[2 * s + 1] = 2.0 * (ALPHA_1 * f1 + ALPHA_2 * f2)
    return tau, coef


def piecewise_schedule(segments):
    """(tau, coef) of a protocol that is constant on intervals: segments = [(duration, [c_0, ..., c_{K-1}]), ...] in time order (a
    square-wave Floquet drive is two segments per period, repeated).  Exact up to the Krylov error of the stages."""
    segments = list(segments)
    if not segments:
        raise ArgumentError("at least one segment")
    tau = np.array([float(d) for d, _c in segments])
    coef = np.array([np.atleast_1d(np.asarray(c, dtype=np.float64)) for _d, c in segments], dtype=np.float64)
    if coef.ndim != 2:
        raise ArgumentError("every segment needs the same number of coefficients")
    return tau, coef


def stage_evolve(model, psi0, drives, tau, coef, kry_m=30, return_info=False):
    """psi <- exp(-i tau[s] (H0 + sum_k coef[s, k] D_k)) psi for s = 0, 1, ... in one library call (sd_driven_evolve), the state on the
    device throughout.  Returns the final state (complex128, normalised by every stage, as krylov_time_evolve): a new torch tensor
    for a torch psi0, a numpy vector otherwise.  return_info: also a dict with the stages run, the operator applications and the
    smallest Lanczos beta seen."""
    drives, di, hi = _split(drives)
    arr, K, _keep = _pack(model, [drives[k] for k in di])
    tau = np.ascontiguousarray(np.atleast_1d(tau), dtype=np.float64)
    if len(tau) < 1:
        raise ArgumentError("at least one stage")
    if hi:
        return _stage_evolve_hop(model, psi0, drives, di, hi, arr, K, tau, coef, kry_m, return_info)
    coef = np.ascontiguousarray(coef, dtype=np.float64).reshape(len(tau), K) if K else np.zeros((len(tau), 0))
    info = _lib.sd_driven_info()
    ctx = model.ctx
    cp = coef.ctypes.data_as(_dp) if K else None
    if _is_torch(psi0):
        import torch
        code = _dtype_code(psi0)
        _bind_torch_stream(model, psi0)
        out = torch.empty(len(psi0), dtype=torch.complex128, device=psi0.device)
        check(lib().sd_driven_evolve_dev(ctx.h, model.h, code, psi0.data_ptr(), len(psi0), arr, K, len(tau), tau.ctypes.data_as(_dp), cp,
                                         int(kry_m), out.data_ptr(), C.byref(info)), ctx.h)
    else:
        x = np.ascontiguousarray(psi0)
        if x.dtype not in (np.float64, np.complex128):
            x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
        out = np.empty(len(x), dtype=np.complex128)
        check(lib().sd_driven_evolve(ctx.h, model.h, _dtype_code(x), x.ctypes.data, len(x), arr, K, len(tau), tau.ctypes.data_as(_dp), cp,
                                     int(kry_m), out.ctypes.data, C.byref(info)), ctx.h)
    if return_info:
        return out, {"stages": int(info.stages), "applies": int(info.applies), "min_beta": float(info.min_beta)}
    return out


def _stage_evolve_hop(model, psi0, drives, di, hi, arr, K, tau, coef, kry_m, return_info):
    """stage_evolve with hopping drives in the list (sd_driven_hop_evolve): the coefficient columns go to the library with the diagonal
    drives first"""
    hops = [drives[k] for k in hi]
    harr, KH = _pack_hops(hops)
    coef = _permute_columns(np.asarray(coef, dtype=np.float64).reshape(len(tau), K + KH), di, hi)
    info = _lib.sd_driven_info()
    ctx = model.ctx
    cp = coef.ctypes.data_as(_dp)
    if _is_torch(psi0):
        import torch
        code = _dtype_code(psi0)
        _bind_torch_stream(model, psi0)
        out = torch.empty(len(psi0), dtype=torch.complex128, device=psi0.device)
        check(lib().sd_driven_hop_evolve_dev(ctx.h, model.h, code, psi0.data_ptr(), len(psi0), arr, K, harr, KH, len(tau),
                                             tau.ctypes.data_as(_dp), cp, int(kry_m), out.data_ptr(), C.byref(info)), ctx.h)
    else:
        x = np.ascontiguousarray(psi0)
        if x.dtype not in (np.float64, np.complex128):
            x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
        out = np.empty(len(x), dtype=np.complex128)
        check(lib().sd_driven_hop_evolve(ctx.h, model.h, _dtype_code(x), x.ctypes.data, len(x), arr, K, harr, KH, len(tau),
                                         tau.ctypes.data_as(_dp), cp, int(kry_m), out.ctypes.data, C.byref(info)), ctx.h)
    if return_info:
        return out, {"stages": int(info.stages), "applies": int(info.applies), "min_beta": float(info.min_beta)}
    return out


def hopping_apply(psi, model, drives, coefs, y=None, out=None):
    """(sum_k coefs[k] B_k) psi for hopping drives, plus y when given (y may be `out`).  Returns `out` (a new vector by default).  A
    list with complex weights needs a complex psi."""
    drives, di, hi = _split(drives)
    if di:
        raise ArgumentError("hopping_apply takes HoppingDrive objects")
    harr, KH = _pack_hops(drives)
    c = _coefs(coefs, KH)
    code = _dtype_code(psi)
    ctx = model.ctx
    if _is_torch(psi):
        import torch
        _bind_torch_stream(model, psi)
        if out is None:
            out = torch.empty_like(psi)
        if _dtype_code(out) != code or (y is not None and _dtype_code(y) != code):
            raise ArgumentError("psi, y and out must have the same element type")
        if len(out) != len(psi) or (y is not None and len(y) != len(psi)):
            raise DimensionMismatch("psi, y and out must have the same length")
        check(lib().sd_hop_apply_dev(ctx.h, model.h, code, psi.data_ptr(), len(psi), harr, KH, c.ctypes.data_as(_dp),
                                     None if y is None else y.data_ptr(), out.data_ptr()), ctx.h)
        return out
    _check_host(psi, "psi")
    if out is None:
        out = np.empty_like(psi)
    _check_host(out, "out")
    if y is not None:
        _check_host(y, "y")
    if out.dtype != psi.dtype or (y is not None and y.dtype != psi.dtype):
        raise ArgumentError("psi, y and out must have the same element type")
    if len(out) != len(psi) or (y is not None and len(y) != len(psi)):
        raise DimensionMismatch("psi, y and out must have the same length")
    check(lib().sd_hop_apply(ctx.h, model.h, code, psi.ctypes.data, len(psi), harr, KH, c.ctypes.data_as(_dp),
                             None if y is None else y.ctypes.data, out.ctypes.data), ctx.h)
    return out


def driven_time_evolve(model, psi0, drives, functions, t0, dt, n_steps, order=4, kry_m=30, measure=None, measure_every=1):
    """psi(t0 + n_steps dt) under H(t) = H0 + sum_k functions[k](t) D_k by magnus_schedule(order) and stage_evolve.  psi0 is a numpy
    vector (uploaded once, the result comes back as numpy) or a torch CUDA tensor (no host copy at any step).  measure(t, psi), if
    given, is called with the device vector at t0 and after every measure_every steps (and after the last step); its return values are
    collected.  Returns (psi_final, measurements)."""
    import torch
    n_steps, every = int(n_steps), max(int(measure_every), 1)
    was_torch = _is_torch(psi0)
    if was_torch:
        psi = psi0
    else:
        x = np.ascontiguousarray(psi0)
        if x.dtype not in (np.float64, np.complex128):
            x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
        psi = torch.as_tensor(x, device=torch.device("cuda", model.ctx.device))
    tau, coef = magnus_schedule(functions, t0, dt, n_steps, order)
    per = len(tau) // n_steps
    out = []
    if measure is None:
        psi = stage_evolve(model, psi, drives, tau, coef, kry_m)
    else:
        out.append(measure(float(t0), psi))
        done = 0
        while done < n_steps:
            k = min(every, n_steps - done)
            psi = stage_evolve(model, psi, drives, tau[per * done: per * (done + k)], coef[per * done: per * (done + k)], kry_m)
            done += k
            out.append(measure(float(t0) + done * float(dt), psi))
    return (psi if was_torch else psi.cpu().numpy()), out


def diagonal_expectation(psi, model, drives):
    """<psi|D_k|psi> for every drive (nothing divided by <psi|psi>), from the magnetisation and the zz correlation matrix"""
    from .observables import correlation_matrix, magnetization_per_site
    drives = _as_list(drives)
    drive_check(model, drives)
    sz = magnetization_per_site(psi, model) if any(d.site_weights is not None for d in drives) else None
    Z = correlation_matrix(psi, model, "zz") if any(len(d.bonds) for d in drives) else None
    vals = np.zeros(len(drives))
    for k, d in enumerate(drives):
        if d.site_weights is not None:
            vals[k] += float(np.dot(d.site_weights, sz))
        for (i, j), v in zip(d.bonds, d.bond_weights):
            vals[k] += v * float(Z[i - 1, j - 1])
    return vals


def instantaneous_energy(psi, model, drives, coefs):
    """<psi|H0 + sum_k coefs[k] D_k|psi> (real part; nothing divided by <psi|psi>): one driven apply and a dot product"""
    if _is_torch(psi):
        import torch
        out = torch.empty_like(psi)
        driven_apply(out, psi, model, drives, coefs)
        return float(torch.vdot(psi, out).real) if psi.is_complex() else float(torch.dot(psi, out))
    x = np.ascontiguousarray(psi)
    if x.dtype not in (np.float64, np.complex128):
        x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    out = np.empty_like(x)
    driven_apply(out, x, model, drives, coefs)
    return float(np.vdot(x, out).real)


def drive_expectation(psi, model, drives):
    """<psi|O_k|psi> for every drive of a mixed list (nothing divided by <psi|psi>): diagonal drives as diagonal_expectation, hopping
    drives as sum_b 2 Re(z_b <S^+_i S^-_j>) from the "+-" correlation matrix"""
    from .observables import correlation_matrix
    drives, di, hi = _split(drives)
    drive_check(model, drives)
    vals = np.zeros(len(drives))
    if di:
        vals[di] = diagonal_expectation(psi, model, [drives[k] for k in di])
    if hi:
        P = correlation_matrix(psi, model, "+-")
        for k in hi:
            d = drives[k]
            vals[k] = sum(2.0 * (complex(z) * complex(P[i - 1, j - 1])).real for (i, j), z in zip(d.bonds, d.weights))
    return vals
