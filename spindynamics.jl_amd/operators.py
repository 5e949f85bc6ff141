"""Operator strings: any product of S^+, S^-, S^z, S^x, S^y on distinct sites, and sums of such products, applied and
measured by one gather kernel family -- no new kernel per observable.

Site i is bit i - 1.  A term is Term(plus, minus, z, c, op): three disjoint site masks, a complex coefficient and the index of the
operator it belongs to,  O_k = sum_{t: op_t = k} c_t prod_{P_t} S^+ prod_{M_t} S^- prod_{Z_t} S^z.  A list of terms is a plain Python
list (lists add up with +); the calls also take the packed structured array (dtype OPTERM).  In a fixed-nup sector every term needs
as many S^+ as S^- factors; on the full basis any term is allowed.  Nothing is divided by <psi|psi>.  Vectors are numpy arrays (host)
or torch CUDA tensors (stay on the device)."""
import ctypes as C
import itertools
from collections import namedtuple

import numpy as np

from ._lib import ArgumentError, DimensionMismatch, SD_C128, SD_F64, check, lib
from .hamiltonian import _bind_torch_stream, _dtype_code, _is_torch, apply_H

_dp = C.POINTER(C.c_double)
OPTERM_MAX, MAX_OPS = 4096, 256          # SD_OPTERM_MAX, SD_OPSTRING_MAX_OPS
# sd_opterm (include/spindyn.h)
OPTERM = np.dtype([("plus", np.uint64), ("minus", np.uint64), ("z", np.uint64), ("c_re", np.float64), ("c_im", np.float64),
                   ("op", np.int32), ("reserved", np.int32)], align=True)
Term = namedtuple("Term", "plus minus z c op")


def _bit(site):
    s = int(site)
    if s != site or not 1 <= s <= 64:
        raise ArgumentError("a site must be an integer in 1..L")
    return 1 << (s - 1)


def op_string(coeff, *factors, op=0):
    """coeff * the product of the factors ("+", i), ("-", j), ("z", k), ("x", a), ("y", b), ... (1-based sites, all distinct) as a
    list of terms of operator `op`.  x and y are expanded on the host, S^x = (S^+ + S^-)/2, S^y = (S^+ - S^-)/(2i): n such factors
    give 2^n terms (the S^+ choice first).  A repeated site is an ArgumentError."""
    plus = minus = z = 0
    xy = []
    seen = 0
    for f in factors:
        kind, site = f
        b = _bit(site)
        if seen & b:
            raise ArgumentError(f"site {int(site)} appears twice in one string")
        seen |= b
        kind = str(kind).lstrip(":")
        if kind in ("+", "plus"):
            plus |= b
        elif kind in ("-", "minus"):
            minus |= b
        elif kind == "z":
            z |= b
        elif kind in ("x", "y"):
            xy.append((kind, b))
        else:
            raise ArgumentError(f"unknown factor {kind!r}: expected \"+\", \"-\", \"z\", \"x\" or \"y\"")
    out = []
    for choice in itertools.product((0, 1), repeat=len(xy)):
        p, m, c = plus, minus, complex(coeff)
        for (kind, b), lower in zip(xy, choice):
            if lower:
                m |= b
                c = c * 0.5 if kind == "x" else complex(-0.5 * c.imag, 0.5 * c.real)      # * (+i/2)
            else:
                p |= b
                c = c * 0.5 if kind == "x" else complex(0.5 * c.imag, -0.5 * c.real)      # * (-i/2)
        out.append(Term(p, m, z, c, int(op)))
    return out


def _as_terms(terms):
    if isinstance(terms, np.ndarray) and terms.dtype == OPTERM:
        return [Term(int(t["plus"]), int(t["minus"]), int(t["z"]), complex(t["c_re"], t["c_im"]), int(t["op"])) for t in terms]
    return [Term(int(t[0]), int(t[1]), int(t[2]), complex(t[3]), int(t[4])) for t in terms]


def pack_terms(terms):
    """the list as the structured array the library reads (dtype OPTERM = sd_opterm)"""
    if isinstance(terms, np.ndarray) and terms.dtype == OPTERM:
        return np.ascontiguousarray(terms)
    tl = _as_terms(terms)
    a = np.zeros(len(tl), dtype=OPTERM)
    for n, t in enumerate(tl):
        for name, v in (("plus", t.plus), ("minus", t.minus), ("z", t.z)):
            if not 0 <= v < 1 << 64:
                raise ArgumentError("a site mask does not fit 64 bits")
            a[n][name] = v
        if not -(1 << 31) <= t.op < 1 << 31:
            raise ArgumentError("op does not fit 32 bits")
        a[n]["c_re"], a[n]["c_im"], a[n]["op"] = t.c.real, t.c.imag, t.op
    return a


def operator_simplify(terms):
    """The same operators with the coefficients of equal (op, plus, minus, z) added up, exact zeros dropped and the terms sorted by
    (op, plus, minus, z), so that every (plus, minus) of an operator is one group (one gather)."""
    acc = {}
    for t in _as_terms(terms):
        key = (t.op, t.plus, t.minus, t.z)
        acc[key] = acc.get(key, 0j) + t.c
    return [Term(p, m, z, c, op) for (op, p, m, z), c in sorted(acc.items()) if c != 0]


def operator_adjoint(terms):
    """the adjoint of every operator of the list: plus and minus swapped, coefficients conjugated, same order"""
    return [Term(t.minus, t.plus, t.z, t.c.conjugate(), t.op) for t in _as_terms(terms)]


def operator_is_hermitian(terms):
    """Is every operator of the list equal to its own adjoint?  Coefficients of equal (plus, minus, z) are added up first and compared
    exactly (the rule of sd_opstring_check)."""
    acc = {}
    for t in _as_terms(terms):
        key = (t.op, t.plus, t.minus, t.z)
        acc[key] = acc.get(key, 0j) + t.c
    return all(c == acc.get((op, m, p, z), 0j).conjugate() for (op, p, m, z), c in acc.items())


def operator_check(model, terms):
    """(K, hermitian) of a list against a model (sd_opstring_check; host only): K = 1 + the largest op.  ArgumentError for a list the
    model does not admit."""
    tl = pack_terms(terms)
    k, h = C.c_int(0), C.c_int(0)
    check(lib().sd_opstring_check(model.h, tl.ctypes.data, len(tl), C.byref(k), C.byref(h)), model.ctx.h if model.ctx is not None else None)
    return k.value, bool(h.value)


def hamiltonian_terms(model):
    """The model's hop, zz and field lists as operator strings of op 0 (sd_hamiltonian_terms; host only), in list order: a hop
    (i, j, t) gives t S^+_i S^-_j then t S^-_i S^+_j, a zz term v S^z_i S^z_j, a field entry B_i S^z_i -> list of terms."""
    ch = model.ctx.h if model.ctx is not None else None
    n = C.c_int(0)
    check(lib().sd_hamiltonian_terms(model.h, None, 0, C.byref(n)), ch)
    out = np.zeros(n.value, dtype=OPTERM)
    if n.value:
        check(lib().sd_hamiltonian_terms(model.h, out.ctypes.data, n.value, C.byref(n)), ch)
    return _as_terms(out)


def _host_vec(psi):
    x = np.ascontiguousarray(psi)
    if x.dtype not in (np.float64, np.complex128):
        x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    return x


def _is_complex(x):
    return x.is_complex() if _is_torch(x) else np.iscomplexobj(x)


def operator_apply(psi, model, terms, y=None, b=1.0, out=None):
    """out = O psi for the operator of a list whose terms all have op = 0, or with y the fused out = O psi + b y (one pass).  The
    result is complex128, or float64 when psi (and y, b, a caller's out) are real and every coefficient is real.  out: where to
    write (psi's kind and length; a device tensor must not share memory with psi; it may be y itself)."""
    tl = pack_terms(terms)
    b = complex(b)
    dev = _is_torch(psi)
    x = psi if dev else _host_vec(psi)
    real = (not _is_complex(x) and bool(np.all(tl["c_im"] == 0.0)) and (y is None or (b.imag == 0.0 and not _is_complex(y)))
            and (out is None or not _is_complex(out)))
    if dev:
        import torch
        want = torch.float64 if real else torch.complex128
        if out is None:
            out = torch.empty(len(x), dtype=want, device=x.device)
        elif not _is_torch(out) or out.device != x.device or not out.is_contiguous() or out.dim() != 1:
            raise ArgumentError("out must be a contiguous 1-D device tensor on psi's device")
    else:
        want = np.float64 if real else np.complex128
        if out is None:
            out = np.empty(len(x), dtype=want)
        elif not isinstance(out, np.ndarray) or out.ndim != 1 or not out.flags.c_contiguous:
            raise ArgumentError("out must be a contiguous 1-D numpy array")
    if len(out) != len(x):
        raise DimensionMismatch("length(out) != length(psi)")
    ocode = _dtype_code(out)
    if ocode == SD_F64 and not real:
        raise ArgumentError("a float64 out needs a float64 psi, real coefficients and a real b y: pass complex128 vectors")
    if y is not None:
        if _is_torch(y) != dev:
            raise ArgumentError("y must be of psi's kind")
        if len(y) != len(x):
            raise DimensionMismatch("length(y) != length(psi)")
        if dev:
            if y.device != x.device:
                raise ArgumentError("y must be on psi's device")
            if y.dtype != out.dtype:
                if y is out:
                    raise ArgumentError("out = y must have the result's dtype")
                y = y.to(out.dtype)
        else:
            y = y if y is out else _host_vec(y).astype(out.dtype, copy=False)
    if dev:
        _bind_torch_stream(model, x)
        _bind_torch_stream(model, out)
        if y is not None:
            _bind_torch_stream(model, y)
        check(lib().sd_opstring_apply_dev(model.ctx.h, model.h, _dtype_code(x), x.data_ptr(), len(x), tl.ctypes.data, len(tl),
                                          None if y is None else y.data_ptr(), b.real, b.imag, ocode, out.data_ptr()), model.ctx.h)
    else:
        check(lib().sd_opstring_apply(model.ctx.h, model.h, _dtype_code(x), x.ctypes.data, len(x), tl.ctypes.data, len(tl),
                                      None if y is None else y.ctypes.data, b.real, b.imag, ocode, out.ctypes.data), model.ctx.h)
    return out


def operator_expectations(ket, model, terms, bra=None):
    """<bra|O_k|ket> for the K = 1 + max op operators of the list from one pass over the rows, no vector O_k ket stored -> complex128
    array of K entries.  bra None: ket itself.  Sums in a fixed order: same call, same bits."""
    tl = pack_terms(terms)
    K = int(tl["op"].max()) + 1 if len(tl) else 0
    out = np.zeros(max(K, 0), dtype=np.complex128)
    op = out.ctypes.data_as(_dp)
    if _is_torch(ket):
        if bra is not None:
            if not _is_torch(bra):
                raise ArgumentError("bra must be of ket's kind")
            if bra.device != ket.device:
                raise ArgumentError("bra must be on ket's device")
            if len(bra) != len(ket):
                raise DimensionMismatch("length(bra) != length(ket)")
            if bra.dtype != ket.dtype:                 # one dtype per call: the real one is promoted
                import torch
                bra, ket = bra.to(torch.complex128), ket.to(torch.complex128)
            _bind_torch_stream(model, bra)
        _bind_torch_stream(model, ket)
        check(lib().sd_opstring_expect_dev(model.ctx.h, model.h, _dtype_code(ket), None if bra is None else bra.data_ptr(),
                                           ket.data_ptr(), len(ket), tl.ctypes.data, len(tl), op), model.ctx.h)
        return out
    ket = _host_vec(ket)
    if bra is not None:
        bra = _host_vec(bra)
        if bra.dtype != ket.dtype:
            bra, ket = bra.astype(np.complex128), ket.astype(np.complex128)
        if len(bra) != len(ket):
            raise DimensionMismatch("length(bra) != length(ket)")
    check(lib().sd_opstring_expect(model.ctx.h, model.h, _dtype_code(ket), None if bra is None else bra.ctypes.data, ket.ctypes.data,
                                   len(ket), tl.ctypes.data, len(tl), op), model.ctx.h)
    return out


def operator_hamiltonian(model, terms, include_model=True):
    """applyH(out, psi, model) for the solvers' applyH= argument: out = (H + O) psi with O the Hermitian operator of the list (op = 0)
    and H the model's own Hamiltonian (include_model=False: O alone).  With include_model it runs apply_H into out, then the fused
    string kernel with y = out: no work vector.  ArgumentError unless the list is Hermitian.  The vectors are device tensors; a list
    with imaginary coefficients (a chirality, a Dzyaloshinskii-Moriya bond) needs complex vectors -- the recursions that take
    complex vectors (lanczos_extremal, lanczos_tridiag, the time evolutions, KPM), or operator_groundstate."""
    tl = pack_terms(terms)
    _k, herm = operator_check(model, tl)
    if not herm:
        raise ArgumentError("the operator is not Hermitian: the list must equal its own adjoint (operator_adjoint)")
    if len(tl) and int(tl["op"].max()) != 0:
        raise ArgumentError("a Hamiltonian is one operator: every term must have op = 0")

    def applyH(out, psi, m):
        if include_model:
            apply_H(out, psi, m)
            return operator_apply(psi, m, tl, y=out, b=1.0, out=out)
        return operator_apply(psi, m, tl, out=out)

    return applyH


def operator_groundstate(model, terms, include_model=True, lanc_m=100, tol=1e-12, seed=0, max_rounds=40):
    """(E0, psi) of H + O (operator_hamiltonian).  A list with real coefficients goes through lanczos_groundstate (float64, as the
    reference).  A list with imaginary coefficients makes H + O complex Hermitian, which that recursion (real vectors) cannot hold:
    the state is then filtered out of the seeded random complex vector by rounds of exp(-tau (H + O)) of the library's imaginary-time
    Chebyshev evolution, run with the operator installed, until <H + O> stops falling by more than tol (relative), and
    E0 = <psi|(H + O)|psi>.  Returns a float64 or complex128 numpy vector, normalised."""
    import torch
    from . import solvers
    from .typicality import thermal_state
    tl = pack_terms(terms)
    op = operator_hamiltonian(model, tl, include_model)
    if bool(np.all(tl["c_im"] == 0.0)):
        return solvers.lanczos_groundstate(op, model, lanc_m=lanc_m, tol=tol, seed=seed)
    lo, hi = solvers.estimate_energy_bounds(op, model, seed=seed)
    pad = 0.05 * (hi - lo) + 1e-3
    lo, hi = lo - pad, hi + pad
    tau = 300.0 / max(hi - lo, 1e-300)            # a tau = 150 with a the half width: inside the Chebyshev routine's range
    dev = torch.device("cuda", model.ctx.device)
    x = np.empty(model.N, dtype=np.complex128)
    check(lib().sd_fill_randn_host(x.ctypes.data_as(_dp), 2 * model.N, int(seed), 0))
    psi = torch.as_tensor(x / np.linalg.norm(x), device=dev)
    hpsi = torch.empty_like(psi)
    e_old, settled = None, 0
    model.set_apply(op)
    try:
        for _ in range(int(max_rounds)):
            psi, _ln = thermal_state(model, 2.0 * tau, r=psi, Ebounds=(lo, hi))
            op(hpsi, psi, model)
            e = float(torch.vdot(psi, hpsi).real)
            # the energy error is second order in the admixture of excited states, other observables first order: two more
            # rounds after the energy has settled
            settled = settled + 1 if e_old is not None and e_old - e <= tol * max(abs(e), 1.0) else 0
            if settled == 3:
                break
            e_old = e
    except Exception:
        if getattr(model, "_apply_err", None) is not None:
            raise model._apply_err
        raise
    finally:
        model.set_apply(None)
    return e, psi.cpu().numpy()


# ---- derived observables: each is one operator_expectations call ----
_EPS = (((0, 1, 2), 1.0), ((1, 2, 0), 1.0), ((2, 0, 1), 1.0), ((0, 2, 1), -1.0), ((2, 1, 0), -1.0), ((1, 0, 2), -1.0))


def chirality_terms(i, j, k, coeff=1.0, op=0):
    """coeff * S_i . (S_j x S_k) = coeff * sum_abc eps_abc S^a_i S^b_j S^c_k as a list of terms: the six products through op_string,
    added up per (plus, minus, z) -- six terms i/2 [S^z (S^+ S^- - S^- S^+) + cyclic] remain."""
    sites = (i, j, k)
    tl = []
    for perm, sign in _EPS:
        tl += op_string(sign * complex(coeff), *[("xyz"[a], s) for a, s in zip(perm, sites)], op=op)
    return operator_simplify(tl)


def scalar_chirality(psi, model, triples):
    """<S_i . (S_j x S_k)> for every triple (i, j, k) of the list -> float64 array (the operator is Hermitian; a real psi gives 0)."""
    tl = []
    for n, (i, j, k) in enumerate(triples):
        tl += chirality_terms(i, j, k, op=n % MAX_OPS)
        if (n + 1) % MAX_OPS == 0 or n + 1 == len(triples):
            tl.append(None)
    return _batched(psi, model, tl).real.copy()


def _batched(psi, model, marked):
    """operator_expectations over a list cut at the None marks (each part within the limits of one call), results joined"""
    out, part = [], []
    for t in marked:
        if t is None:
            if part:
                out.append(operator_expectations(psi, model, part))
            part = []
        else:
            part.append(t)
    return np.concatenate(out) if out else np.zeros(0, dtype=np.complex128)


def _product(a, b, op):
    """the product of two operators on disjoint sites as a list of terms of operator `op`"""
    return operator_simplify([Term(s.plus | t.plus, s.minus | t.minus, s.z | t.z, s.c * t.c, op) for s in a for t in b])


def chirality_correlations(psi, model, triples, pairs=None):
    """<chi_a chi_b> for pairs (a, b) of triples that share no site, chi = S_i . (S_j x S_k) -> T x T float64 matrix, symmetric,
    NaN where no pair was asked for (the diagonal: chi_a^2 is not a product of factors on distinct sites).  pairs None: every a < b.  A
    pair whose triples share a site is an ArgumentError."""
    tr = [tuple(int(s) for s in t) for t in triples]
    T = len(tr)
    pl = [(a, b) for a in range(T) for b in range(a + 1, T)] if pairs is None else [(int(a), int(b)) for a, b in pairs]
    chi = [chirality_terms(*t) for t in tr]
    marked, k, nt = [], 0, 0
    for a, b in pl:
        if not (0 <= a < T and 0 <= b < T):
            raise ArgumentError("a pair names a triple that is not in the list")
        if set(tr[a]) & set(tr[b]):
            raise ArgumentError(f"triples {tr[a]} and {tr[b]} share a site: their product is not a string on distinct sites")
        prod = _product(chi[a], chi[b], 0)
        if k == MAX_OPS or nt + len(prod) > OPTERM_MAX:
            marked.append(None)
            k, nt = 0, 0
        marked += [t._replace(op=k) for t in prod]
        k, nt = k + 1, nt + len(prod)
    marked.append(None)
    vals = _batched(psi, model, marked)
    Cm = np.full((T, T), np.nan)
    for (a, b), v in zip(pl, vals):
        Cm[a, b] = Cm[b, a] = v.real
    return Cm


def string_order_terms(i, j, op=0):
    """-S^z_i exp(i pi sum_{i<l<j} S^z_l) S^z_j as one diagonal term: exp(i pi S^z) = 2i S^z for spin 1/2"""
    i, j = int(i), int(j)
    if not 1 <= i < j:
        raise ArgumentError("string_order needs sites 1 <= i < j")
    return op_string(-((2j) ** (j - i - 1)), *[("z", l) for l in range(i, j + 1)], op=op)


def string_order(psi, model, i, j):
    """-<S^z_i exp(i pi sum_{i<l<j} S^z_l) S^z_j> (the den Nijs-Rommelse string order parameter of sites i < j) -> complex; real for
    an even number of sites in between."""
    return complex(operator_expectations(psi, model, string_order_terms(i, j))[0])


def multi_spin_expectation(psi, model, strings):
    """<psi| c prod factors |psi> for every string (c, factor, factor, ...) of a caller's list, e.g. (1.0, ("z", 1), ("z", 2), ("+", 3),
    ("-", 4)) -> complex128 array, one entry per string; all from one pass (lists beyond the limits of one call are cut)."""
    marked, k, nt = [], 0, 0
    for s in strings:
        tl = op_string(s[0], *s[1:], op=0)
        if k == MAX_OPS or nt + len(tl) > OPTERM_MAX:
            marked.append(None)
            k, nt = 0, 0
        marked += [t._replace(op=k) for t in tl]
        k, nt = k + 1, nt + len(tl)
    marked.append(None)
    return _batched(psi, model, marked)
