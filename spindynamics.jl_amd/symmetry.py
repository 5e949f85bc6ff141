"""Lattice symmetry operators: translation T, reflection R and spin flip Z of a chain as permutation gathers on
the device, the overlaps <bra|U_g|ket> of a whole group and the projector sum_g c_g U_g psi in one pass each, and what follows
from them: the momentum, parity and spin-flip labels of a state, symmetry-restricted vectors and the lowest level of a sector.

Site i is bit i - 1.  T moves the spin of site i to site i + 1 (mod L), R exchanges site i with site L + 1 - i, Z flips every spin
(defined on the full basis and on sectors with 2 nup = L).  A group element (r, refl, flip) is U_g = T^r R^refl Z^flip,
(U_g psi)[idx(s)] = psi[idx(Z^flip R^refl T^-r s)], with the code r | refl << 8 | flip << 9.  Momenta are momenta(model),
k_n = 2 pi n / L:  P_n = (1/L) sum_r e^{+i k_n r} T^r, so T P_n = e^{-i k_n} P_n; parity and spin-flip projectors are (1 +- R)/2 and
(1 +- Z)/2.  Nothing is divided by <psi|psi>.  psi may be a numpy array (host) or a torch CUDA tensor (stays on the device)."""
import ctypes as C
import math

import numpy as np

from ._lib import ArgumentError, DimensionMismatch, SD_C128, SD_F64, ZeroNormError, check, lib
from .hamiltonian import _bind_torch_stream, _dtype_code, _is_torch, apply_H

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
REFLECT, FLIP = 256, 512          # SD_SYM_REFLECT, SD_SYM_FLIP


def element_code(model, shift=0, reflect=False, flip=False):
    """the code of U_g = T^shift R^reflect Z^flip; the shift is taken mod L"""
    if model.L < 1:
        raise ArgumentError("symmetry operators need L >= 1")
    return int(shift) % model.L | (REFLECT if reflect else 0) | (FLIP if flip else 0)


def _codes(model, elements):
    out = []
    for e in elements:
        out.append(int(e) if isinstance(e, (int, np.integer)) else element_code(model, *e))
    return np.ascontiguousarray(np.array(out, dtype=np.intc))


def _host_vec(psi):
    x = np.ascontiguousarray(psi)
    if x.dtype not in (np.float64, np.complex128):
        x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    return x


def _out_for(psi, out, complex_out):
    """(out, its dtype code) for a vector-valued call: a new vector of psi's kind, or the caller's after checks"""
    if _is_torch(psi):
        import torch
        if out is None:
            out = torch.empty(len(psi), dtype=torch.complex128 if complex_out else psi.dtype, device=psi.device)
        elif not _is_torch(out) or out.device != psi.device or not out.is_contiguous() or out.dim() != 1:
            raise ArgumentError("out must be a contiguous 1-D device tensor on psi's device")
    elif out is None:
        out = np.empty(len(psi), dtype=np.complex128 if complex_out else psi.dtype)
    elif not isinstance(out, np.ndarray) or out.ndim != 1 or not out.flags.c_contiguous:
        raise ArgumentError("out must be a contiguous 1-D numpy array")
    if len(out) != len(psi):
        raise DimensionMismatch("length(out) != length(psi)")
    return out, _dtype_code(out)


def symmetry_apply(psi, model, shift=0, reflect=False, flip=False, out=None, *, y=None, c=1.0):
    """out = U_g psi for g = (shift, reflect, flip): a vector of psi's kind and dtype, every entry bit for bit one entry of psi.
    With y (psi's kind, dtype and length) the fused out = U_g psi + c y (c complex; real for a float64 psi) -- one pass, the step
    of a chain of shifts.  out: where to write (same kind, dtype, length; a device tensor must not share memory with psi; it may be y itself)."""
    code = element_code(model, shift, reflect, flip)
    c = complex(c)
    dev = _is_torch(psi)
    x = psi if dev else _host_vec(psi)
    out, ocode = _out_for(x, out, np.iscomplexobj(x) if not dev else x.is_complex())
    if ocode != _dtype_code(x):
        raise ArgumentError("out must have psi's dtype")
    if y is not None:
        if _is_torch(y) != dev:
            raise ArgumentError("y must be of psi's kind")
        if dev and y.device != x.device:
            raise ArgumentError("y must be on psi's device")
        y = y if dev else _host_vec(y).astype(x.dtype, copy=False)
        if _dtype_code(y) != ocode:
            raise ArgumentError("y must have psi's dtype")
        if len(y) != len(x):
            raise DimensionMismatch("length(y) != length(psi)")
    if dev:
        _bind_torch_stream(model, x)
        if y is not None:
            _bind_torch_stream(model, y)
        check(lib().sd_symmetry_apply_dev(model.ctx.h, model.h, ocode, x.data_ptr(), len(x), code,
                                          None if y is None else y.data_ptr(), c.real, c.imag, out.data_ptr()), model.ctx.h)
    else:
        check(lib().sd_symmetry_apply(model.ctx.h, model.h, ocode, x.ctypes.data, len(x), code,
                                      None if y is None else y.ctypes.data, c.real, c.imag, out.ctypes.data), model.ctx.h)
    return out


def translate(psi, model, r=1, out=None):
    """T^r psi: the spin of site i moves to site i + r (mod L); r may be negative"""
    return symmetry_apply(psi, model, shift=r, out=out)


def reflect(psi, model, out=None):
    """R psi: site i <-> site L + 1 - i"""
    return symmetry_apply(psi, model, reflect=True, out=out)


def spin_flip(psi, model, out=None):
    """Z psi: every spin flipped (full basis, or a sector with 2 nup = L)"""
    return symmetry_apply(psi, model, flip=True, out=out)


def _perm_arg(perm, L, what):
    """perm as a contiguous intc array of L entries (the library checks that it is a bijection of 1..L)"""
    p = np.asarray(perm)
    if p.ndim != 1 or len(p) != L or not (np.issubdtype(p.dtype, np.integer) or (p == np.floor(p)).all()):
        raise ArgumentError(f"{what}: perm must be a list of L = {L} integers, a bijection of 1..L")
    return np.ascontiguousarray(p, dtype=np.intc)


def permute_sites(psi, model, perm, out=None):
    """out = U_pi psi for the site permutation perm: perm[i] is the 1-based site to which the spin of site i + 1 moves,
    a bijection of 1..L, so (U_pi psi)[idx(s)] = psi[idx(src(s))] with bit i of src(s) = bit perm[i] - 1 of s.  A vector of psi's
    kind and dtype, every entry bit for bit one entry of psi.  out: where to write (same kind, dtype, length; it must not share
    memory with psi)."""
    pm = _perm_arg(perm, model.L, "permute_sites")
    dev = _is_torch(psi)
    x = psi if dev else _host_vec(psi)
    out, ocode = _out_for(x, out, np.iscomplexobj(x) if not dev else x.is_complex())
    if ocode != _dtype_code(x):
        raise ArgumentError("out must have psi's dtype")
    pp = pm.ctypes.data_as(_ip)
    if dev:
        _bind_torch_stream(model, x)
        check(lib().sd_site_permute_dev(model.ctx.h, model.h, ocode, x.data_ptr(), len(x), pp, out.data_ptr()), model.ctx.h)
    else:
        check(lib().sd_site_permute(model.ctx.h, model.h, ocode, x.ctypes.data, len(x), pp, out.ctypes.data), model.ctx.h)
    return out


def _bijection(p, what):
    p = np.asarray(p, dtype=np.int64)
    if p.ndim != 1 or len(p) < 1 or not np.array_equal(np.sort(p), np.arange(1, len(p) + 1)):
        raise ArgumentError(f"{what}: not a bijection of 1..L")
    return p


def permutation_inverse(perm):
    """the permutation q with U_q U_perm = 1: q[perm[i] - 1] = i + 1 (host only)"""
    p = _bijection(perm, "permutation_inverse")
    q = np.empty_like(p)
    q[p - 1] = np.arange(1, len(p) + 1)
    return q.astype(np.intc)


def permutation_compose(p, q):
    """the permutation r with U_r = U_p U_q (q acts first): r[i] = p[q[i] - 1] (host only)"""
    p, q = _bijection(p, "permutation_compose"), _bijection(q, "permutation_compose")
    if len(p) != len(q):
        raise ArgumentError("permutation_compose: the two permutations have different lengths")
    return p[q - 1].astype(np.intc)


def subsystem_permutation(L, sites):
    """The permutation that brings the listed sites to the front (sd_subsystem_permutation; host only): sites[j] goes to site j + 1,
    in the order given, the remaining sites to len(sites) + 1 .. L in ascending order.  The sites must be distinct, in 1..L, and
    at least 1 and at most L - 1 of them."""
    try:
        s = np.ascontiguousarray([int(x) for x in sites], dtype=np.intc)
    except (TypeError, ValueError):
        raise ArgumentError("subsystem_permutation: sites must be a list of integers") from None
    if any(isinstance(x, bool) or int(x) != x for x in sites) or not 1 <= int(L) <= 63:
        raise ArgumentError("subsystem_permutation: sites must be integers and 1 <= L <= 63")
    out = np.zeros(int(L), dtype=np.intc)
    if lib().sd_subsystem_permutation(int(L), s.ctypes.data_as(_ip), len(s), out.ctypes.data_as(_ip)) != 0:
        raise ArgumentError(f"subsystem_permutation: the sites must be distinct, in 1..L = 1..{int(L)}, and 1 <= len(sites) <= L - 1")
    return out


def symmetry_overlaps(psi, model, elements, bra=None):
    """<bra|U_g|psi> for every element of `elements` ((shift, reflect, flip) tuples, shorter tuples filled with zeros, or codes)
    from one pass over the rows -> complex128 array.  bra None: psi itself.  Sums in a fixed order: same call, same bits."""
    codes = _codes(model, elements)
    out = np.empty(len(codes), dtype=np.complex128)
    cp, op = codes.ctypes.data_as(_ip), out.ctypes.data_as(_dp)
    if _is_torch(psi):
        ket = psi
        if bra is not None:
            if not _is_torch(bra):
                raise ArgumentError("bra must be of psi's kind")
            if bra.device != ket.device:
                raise ArgumentError("bra must be on psi's device")
            if len(bra) != len(ket):                   # the kernel reads bra at every row of psi
                raise DimensionMismatch("length(bra) != length(psi)")
            if bra.dtype != ket.dtype:                 # one dtype per call: the real one is promoted
                import torch
                bra, ket = bra.to(torch.complex128), ket.to(torch.complex128)
            _bind_torch_stream(model, bra)
        _bind_torch_stream(model, ket)
        check(lib().sd_symmetry_overlaps_dev(model.ctx.h, model.h, _dtype_code(ket), None if bra is None else bra.data_ptr(),
                                             ket.data_ptr(), len(ket), cp, len(codes), op), model.ctx.h)
        return out
    ket = _host_vec(psi)
    if bra is not None:
        bra = _host_vec(bra)
        if bra.dtype != ket.dtype:
            bra, ket = bra.astype(np.complex128), ket.astype(np.complex128)
        if len(bra) != len(ket):
            raise DimensionMismatch("length(bra) != length(psi)")
    check(lib().sd_symmetry_overlaps(model.ctx.h, model.h, _dtype_code(ket), None if bra is None else bra.ctypes.data,
                                     ket.ctypes.data, len(ket), cp, len(codes), op), model.ctx.h)
    return out


def _phase(n, r, L):
    """e^{+i k_n r}, k_n = 2 pi n / L, exactly +-1 at k = 0 and k = pi"""
    if (n * r) % L == 0:
        return 1.0 + 0.0j
    if (2 * n * r) % L == 0:
        return -1.0 + 0.0j
    a = 2.0 * math.pi * ((n * r) % L) / L
    return complex(math.cos(a), math.sin(a))


def _weights_from(ov, L):
    return np.array([sum(_phase(n, r, L) * ov[r] for r in range(L)).real / L for n in range(L)])


def momentum_weights(psi, model):
    """w_n = <psi|P_n|psi> = (1/L) sum_r e^{i k_n r} <psi|T^r|psi>, n = 0..L-1, from one overlaps pass -> float64 array.  The
    weights are >= 0 and add up to <psi|psi>."""
    L = model.L
    return _weights_from(symmetry_overlaps(psi, model, [(r,) for r in range(L)]), L)


def _flip_defined(model):
    return model.nup is None or 2 * model.nup == model.L


def quantum_numbers(psi, model, tol=1e-8):
    """The symmetry labels of psi from one overlaps pass: {"momentum": n with w_n >= (1 - tol) <psi|psi>, else None; "parity": +1 or
    -1 when <R> / <psi|psi> is within tol of it, else None; "spin_flip": the same for Z, None where Z is undefined;
    "expectation": the raw values {"norm2", "T" (<T^r>, r = 0..L-1), "weights" (w_n), "R", "Z" (None where undefined)}}."""
    L = model.L
    el = [(r,) for r in range(L)] + [(0, True)] + ([(0, False, True)] if _flip_defined(model) else [])
    ov = symmetry_overlaps(psi, model, el)
    n2 = ov[0].real
    w = _weights_from(ov[:L], L)
    hit = np.nonzero(w >= (1.0 - tol) * n2)[0] if n2 > 0.0 else []

    def sign(v):
        if n2 > 0.0 and abs(v / n2 - 1.0) <= tol:
            return 1
        if n2 > 0.0 and abs(v / n2 + 1.0) <= tol:
            return -1
        return None

    Rv = complex(ov[L])
    Zv = complex(ov[L + 1]) if _flip_defined(model) else None
    return {"momentum": int(hit[0]) if len(hit) else None, "parity": sign(Rv), "spin_flip": None if Zv is None else sign(Zv),
            "expectation": {"norm2": n2, "T": ov[:L].copy(), "weights": w, "R": Rv, "Z": Zv}}


def projector_elements(model, momentum=None, parity=None, spin_flip=None):
    """(codes, coefficients) of the product of the requested projectors P_n (1 + parity R)/2 (1 + spin_flip Z)/2 as a list of
    elements T^r R^refl Z^flip, r fastest-outermost: for r, for refl, for flip.  Coefficients at k = 0 and k = pi are real."""
    L = model.L
    if momentum is not None and (int(momentum) != momentum or not 0 <= int(momentum) < L):
        raise ArgumentError("momentum must be an integer n in 0..L-1 (k_n = 2 pi n / L)")
    for name, v in (("parity", parity), ("spin_flip", spin_flip)):
        if v is not None and v not in (1, -1):
            raise ArgumentError(f"{name} must be +1, -1 or None")
    if parity is not None and momentum is not None and not (momentum == 0 or 2 * int(momentum) == L):
        raise ArgumentError("parity combines with momentum only at n = 0 and, for even L, n = L/2")
    if spin_flip is not None and not _flip_defined(model):
        raise ArgumentError("the spin flip Z is defined on the full basis and on sectors with 2 nup = L only")
    codes, coef = [], []
    for r in (range(L) if momentum is not None else (0,)):
        cr = _phase(int(momentum), r, L) / L if momentum is not None else 1.0 + 0.0j
        for refl in ((0, 1) if parity is not None else (0,)):
            cp = cr * (0.5 * (parity if refl else 1) if parity is not None else 1.0)
            for fl in ((0, 1) if spin_flip is not None else (0,)):
                codes.append(r | (REFLECT if refl else 0) | (FLIP if fl else 0))
                coef.append(cp * (0.5 * (spin_flip if fl else 1) if spin_flip is not None else 1.0))
    return np.array(codes, dtype=np.intc), np.array(coef, dtype=np.complex128)


def symmetry_combine(psi, model, elements, coefficients, out=None):
    """out = sum_g c_g U_g psi for a list of elements and complex coefficients, one pass.  complex128, or float64 for a float64 psi
    when every coefficient is real (a caller's float64 `out` with an imaginary coefficient raises ArgumentError).  An element given
    as a (shift, reflect, flip) tuple has its shift taken mod L; an integer is a code r | refl << 8 | flip << 9, handed on as it is
    and refused (ArgumentError) when r >= L or another bit is set -- in symmetry_overlaps alike."""
    codes = _codes(model, elements)
    coef = np.ascontiguousarray(coefficients, dtype=np.complex128)
    if len(coef) != len(codes):
        raise ArgumentError("one coefficient per element")
    dev = _is_torch(psi)
    x = psi if dev else _host_vec(psi)
    real = _dtype_code(x) == SD_F64 and bool(np.all(coef.imag == 0.0))
    out, ocode = _out_for(x, out, not real)
    cp, fp = codes.ctypes.data_as(_ip), coef.view(np.float64).ctypes.data_as(_dp)
    if dev:
        _bind_torch_stream(model, x)
        check(lib().sd_symmetry_project_dev(model.ctx.h, model.h, _dtype_code(x), x.data_ptr(), len(x), cp, fp, len(codes), ocode,
                                            out.data_ptr()), model.ctx.h)
    else:
        check(lib().sd_symmetry_project(model.ctx.h, model.h, _dtype_code(x), x.ctypes.data, len(x), cp, fp, len(codes), ocode,
                                        out.ctypes.data), model.ctx.h)
    return out


def symmetry_project(psi, model, momentum=None, parity=None, spin_flip=None, out=None):
    """P psi with P the product of the requested projectors: momentum n (P_n), parity +-1 ((1 +- R)/2), spin_flip +-1 ((1 +- Z)/2);
    one pass over the rows whatever the group's size.  float64 stays float64 when the coefficients are real (k = 0, k = pi)."""
    codes, coef = projector_elements(model, momentum, parity, spin_flip)
    return symmetry_combine(psi, model, codes, coef, out=out)


def is_symmetric(model, shift=0, reflect=False, flip=False):
    """Are the hop, zz and field lists of `model` invariant under U_g (sd_model_symmetric; host only)?"""
    yes = C.c_int()
    check(lib().sd_model_symmetric(model.h, element_code(model, shift, reflect, flip), C.byref(yes)),
          model.ctx.h if model.ctx is not None else None)
    return bool(yes.value)


def _check_sector(model, momentum, parity, spin_flip):
    projector_elements(model, momentum, parity, spin_flip)          # argument errors first
    for want, kw, name in ((momentum, {"shift": 1}, "translation"), (parity, {"reflect": True}, "reflection"),
                           (spin_flip, {"flip": True}, "spin-flip")):
        if want is not None and not is_symmetric(model, **kw):
            raise ArgumentError(f"the model is not {name} invariant")


def symmetric_operator(model, momentum=None, parity=None, spin_flip=None):
    """applyH(out, psi, model) for the solvers' applyH= argument that writes P (H psi), P = symmetry_project of the sector.  The
    model must have the symmetries asked for (ArgumentError).  The vectors are device tensors; a projector with complex
    coefficients needs complex vectors (the recursions that take applyH= run in complex128)."""
    _check_sector(model, momentum, parity, spin_flip)
    codes, coef = projector_elements(model, momentum, parity, spin_flip)
    work = {}

    def applyH(out, psi, m):
        key = (psi.dtype, len(psi), psi.device)
        if key not in work:
            work.clear()
            work[key] = psi.new_empty(len(psi))
        tmp = work[key]
        apply_H(tmp, psi, m)
        symmetry_combine(tmp, m, codes, coef, out=out)
        return out

    return applyH


def lowest_level(model, lanc_m=100, psi0=None, seed=0, tol=1e-12, **sector):
    """The lowest eigenvalue of H in a symmetry sector (momentum=, parity=, spin_flip=): lanczos_extremal of
    symmetric_operator(model, **sector) started from P psi0 (psi0 None: the seeded random complex vector).  The start vector lies in
    the sector and every step is projected, so the Krylov space never leaves it and rounding leakage is removed each step.  The
    recursion sees P H P, whose levels outside the sector are 0; a sector smaller than lanc_m is exhausted early and the recursion's
    breakdown test (tol) ends it there.  The projected start vector goes through the host: lanczos_extremal, like the C entry behind
    it, takes its start vector as a host array."""
    import torch
    from .solvers import lanczos_extremal
    op = symmetric_operator(model, **sector)
    dev = torch.device("cuda", model.ctx.device)
    if psi0 is None:
        x = torch.empty(model.N, dtype=torch.complex128, device=dev)
        _bind_torch_stream(model, x)
        check(lib().sd_fill_randn_dev(model.ctx.h, x.data_ptr(), 2 * model.N, int(seed), 0), model.ctx.h)
    else:
        if _is_torch(psi0) and psi0.device != dev:
            raise ArgumentError("psi0 must be on the model's device")
        x = torch.as_tensor(np.ascontiguousarray(psi0, dtype=np.complex128), device=dev) if not _is_torch(psi0) else psi0.to(torch.complex128)
        if len(x) != model.N:
            raise DimensionMismatch(f"psi0 has length {len(x)}, expected {model.N}")
    p0 = symmetry_project(x, model, **sector)
    if float(torch.linalg.vector_norm(p0)) == 0.0:
        raise ZeroNormError("the start vector has no component in the sector")
    return lanczos_extremal(op, model, lanc_m=lanc_m, tol=tol, psi0=p0.cpu().numpy(), seed=seed)[0]


def lowest_levels(model, k, psi0=None, seed=0, **sector):
    """The lowest k eigenpairs of H in a symmetry sector (momentum=, parity=, spin_flip=) -> (E, X): lanczos_eigenpairs of
    symmetric_operator(model, **sector) in complex128, started from P psi0 (psi0 None: the seeded random complex vector); X is a
    torch tensor (N, k) on the model's device.  basis_size=, tol= and max_applies= are passed on.  The call sets confirm=False: the
    confirmation step starts from a fresh random vector, which would leave the sector (the solver sees P H P, whose levels outside
    the sector are 0).  What it is for is done by the sector itself, which resolves the lattice degeneracies: the +-k partners of a
    ring lie in different sectors.  k must not exceed the sector's dimension, for the same reason."""
    import torch
    from .solvers import lanczos_eigenpairs
    kw = {n: sector.pop(n) for n in ("basis_size", "tol", "max_applies") if n in sector}
    op = symmetric_operator(model, **sector)
    dev = torch.device("cuda", model.ctx.device)
    if psi0 is None:
        x = torch.empty(model.N, dtype=torch.complex128, device=dev)
        _bind_torch_stream(model, x)
        check(lib().sd_fill_randn_dev(model.ctx.h, x.data_ptr(), 2 * model.N, int(seed), 0), model.ctx.h)
    else:
        if _is_torch(psi0) and psi0.device != dev:
            raise ArgumentError("psi0 must be on the model's device")
        x = torch.as_tensor(np.ascontiguousarray(psi0, dtype=np.complex128), device=dev) if not _is_torch(psi0) else psi0.to(torch.complex128)
        if len(x) != model.N:
            raise DimensionMismatch(f"psi0 has length {len(x)}, expected {model.N}")
    p0 = symmetry_project(x, model, **sector)
    if float(torch.linalg.vector_norm(p0)) == 0.0:
        raise ZeroNormError("the start vector has no component in the sector")
    E, X, _ = lanczos_eigenpairs(op, model, k=k, confirm=False, psi0=p0, seed=seed, **kw)
    return E, X
