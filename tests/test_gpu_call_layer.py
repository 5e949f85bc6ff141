"""The host call layer of the one-pass entry points: what lies between the C ABI and a kernel launch -- the argument
checks in their order, the staging of host vectors through the context's pool, the read-back -- for every host / _dev pair that
stages a vector that way.  No arithmetic is judged here; the kernels have their own files.

1. Refusals (REFUSALS, on L = 6, nup = 3, N = 20, periodic).  Every row is a bad call with the exact status and the exact text of
   sd_last_error, copied by hand from the sd_set_err calls of the cores (csrc/), never recorded from a run.  A row whose call
   violates two checks pins which of them comes first.  After every refusal the entry's valid call runs on the same context and
   must give the bits it gave before: a refusal leaves nothing behind.  Not in the table, with the reason:
     * ctx == NULL: there is no context to hold a text, and the Python binding never passes one;
     * the SD_ENOMEM / SD_EHIP returns of sd_pool_take, sd_xfer_* and SD_HIP: they need an exhausted or broken device;
     * "bad dtype" / "null argument" of the staging helper where the core has checked the same thing before (bond_apply,
       dimer_correlations, dcurrent, symmetry_*, opstring_*, the bra of the two bracket forms): unreachable;
     * "communicator size does not match the model's shard count": the unsharded entry points pass no communicator;
     * the N == 0 return of cut_gram and the n == 0 returns of site_permute / subsystem_gram: sd_model_create admits no empty basis;
     * "operator strings need 1 <= L <= 63", "diagonal drives need 1 <= L <= 63", "null model": sd_model_create admits no such model;
     * the remaining texts of sd_opstring_build, sd_drive_build, sd_cut_layout and of the launchers (each has one row here, to pin
       where the builder is called): they are checked where those builders are tested (test_gpu_opstrings, test_gpu_drive_kernel,
       test_cut_plan_host, test_gpu_basis_stats).
2. Host form == device form, bit for bit (test_host_form_equals_device_form): every pair, Float64 and ComplexF64 where the entry
   takes both, on the tiled plan (L = 10, nup = 5, N = 252), the per-row plan (L = 13, nup = 1) and the full basis (L = 7), from a
   random state of sd_fill_randn_host.  The two forms run the same kernel on the same bits, so every output double is equal.
3. Empty inputs (test_empty_inputs): the early returns write what they write today."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EARG, EDIM = 1, 2
F64, C128 = 1, 2
NAN, INF = float("nan"), float("inf")

# sd_dterm / sd_opterm (include/spindyn.h)
DTERM = np.dtype([("i", np.int32), ("j", np.int32), ("k", np.int32), ("c", np.float64)], align=True)
OPTERM = np.dtype([("plus", np.uint64), ("minus", np.uint64), ("z", np.uint64), ("c_re", np.float64), ("c_im", np.float64),
                   ("op", np.int32), ("reserved", np.int32)], align=True)

T_TABLES = "model has no device tables"
T_TABLES_CTX = "model has no device tables (created without a context)"
T_SHARDED = "a sharded model needs a communicator (the unsharded entry points take an unsharded model)"
T_LEN = "vector length does not match the basis dimension"
T_NULL = "null argument"
T_DTYPE = "dtype must be SD_F64 or SD_C128"
T_BAD = "bad dtype"
T_ALIAS = "out must not alias psi"
T_OVERLAP = "out must not alias or overlap psi"
T_YPART = "out may be y itself but must not overlap it partly"


def _addr(v):
    if v is None:
        return None
    if isinstance(v, np.ndarray):
        return v.ctypes.data
    if isinstance(v, C.Structure) or isinstance(v, C.Array) or hasattr(v, "_b_base_"):
        return C.addressof(v)
    if hasattr(v, "data_ptr"):
        return v.data_ptr()
    return v


class Env:
    """one model on the default context with its random vectors, on the host and on the device"""

    def __init__(self, pkg, L, nup, seed=11):
        import torch
        self.torch, self.pkg, self.lib = torch, pkg, pkg.lib()
        self.m = pkg.XXZChain(L, Jxy=0.8, Jz=0.7, hz=0.0, nup=nup, boundary="periodic")
        self.L, self.N, self.ctx = L, self.m.N, self.m.ctx.h
        self.m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        self.host, self.dev, self.keep = {}, {}, []
        for which in (0, 1):
            g = np.empty(2 * self.N)
            assert self.lib.sd_fill_randn_host(g.ctypes.data_as(C.POINTER(C.c_double)), 2 * self.N, seed + which, 0) == 0
            self.host[F64, which] = g[: self.N].copy()
            self.host[C128, which] = g.view(np.complex128).copy()
            for dt in (F64, C128):
                self.dev[dt, which] = torch.from_numpy(self.host[dt, which]).cuda()
        torch.cuda.synchronize()

    def vec(self, dt, dev, which=0):
        return (self.dev if dev else self.host)[dt, which]

    def out(self, dt, dev, n=None):
        """a result vector of n elements of dt, filled with NaN, where the form wants it"""
        n = self.N if n is None else n
        np_dt = np.complex128 if dt == C128 else np.float64
        h = np.full(n, np.nan, dtype=np_dt)
        return self.torch.from_numpy(h).cuda() if dev else h

    def call(self, name, dev, order, args, over, outs):
        """the entry `name` (its _dev form when dev) on args + over -> (status, last error text, outputs as host arrays)"""
        a = dict(args)
        a.update(over)
        for k, v in list(a.items()):
            if isinstance(v, tuple) and len(v) == 3 and v[0] == "@":         # ("@", other argument, byte offset): an alias of it
                a[k] = _addr(args[v[1]]) + v[2]
        full = name + ("_dev" if dev else "")
        types = self.pkg._lib.PROTOTYPES[full][1]
        assert len(types) == len(order), full
        vals = []
        for k, t in zip(order, types):
            v = a[k]
            if isinstance(v, C.c_void_p):
                vals.append(v)
                continue
            if v is not None and not isinstance(v, (int, float)):
                v = _addr(v)
            if v is not None and t is not C.c_void_p and isinstance(t, type) and issubclass(t, C._Pointer):
                v = C.cast(C.c_void_p(v), t)
            vals.append(v)
        rc = getattr(self.lib, full)(*vals)
        self.torch.cuda.synchronize()
        msg = self.lib.sd_last_error(self.ctx)
        res = [o.cpu().numpy() if hasattr(o, "data_ptr") else np.array(o, copy=True) for o in outs]
        return rc, (msg.decode() if msg else ""), res


# ---- the entries: name -> (argument names in ABI order, builder(env, dev, dt) -> (arguments, outputs), dtypes it takes) ----
def _dterms(rows):
    t = np.zeros(len(rows), dtype=DTERM)
    for n, (i, j, k, c) in enumerate(rows):
        t[n] = (i, j, k, c)
    return t


def _opterms(rows):
    t = np.zeros(len(rows), dtype=OPTERM)
    for n, (p, mi, z, cr, ci, op) in enumerate(rows):
        t[n] = (p, mi, z, cr, ci, op, 0)
    return t


def _ints(*v):
    return np.array(v, dtype=np.intc)


def _f(*v):
    return np.array(v, dtype=np.float64)


DLIST = [(1, 2, 0, 0.5), (1, 2, 4, -0.25), (3, 2, 5, 0.75), (5, 6, 0, 1.5)]


def oplist(dt, ops=False):
    """two groups of one operator (ops: a second operator, for the expectation form); real coefficients for a Float64 vector"""
    ci = 0.0 if dt == F64 else 0.2
    rows = [(1, 2, 4, 0.7, ci, 0), (2, 1, 0, -0.3, 0.0, 0), (0, 0, 1 | 8, 0.5, 0.0, 0)]
    if ops:
        rows += [(0, 0, 2, 1.0, 0.0, 1), (4, 8, 0, 0.25, ci, 1)]
    return _opterms(rows)


def _drives(env):
    """two drives: a site-weight drive and a zz-bond drive; the arrays stay alive in env.keep"""
    sd_drive = env.pkg._lib.sd_drive
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
    w = _f(*[0.1 * (i + 1) for i in range(env.L)])
    zi, zj, zw = _ints(1, 2), _ints(2, 4), _f(0.5, -0.25)
    arr = (sd_drive * 2)()
    arr[0] = sd_drive(w.ctypes.data_as(dp), 0, None, None, None)
    arr[1] = sd_drive(None, 2, zi.ctypes.data_as(ip), zj.ctypes.data_as(ip), zw.ctypes.data_as(dp))
    env.keep += [w, zi, zj, zw, arr]
    return arr


def _gram_elems(env, cut, side):
    nb, ne = C.c_int(0), C.c_int64(0)
    assert env.lib.sd_cut_blocks(env.m.h, cut, side, None, 0, C.byref(nb), C.byref(ne)) == 0
    return int(ne.value)


def b_site_project(env, dev, dt):
    out = np.full(2 * env.L, np.nan)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, bra=env.vec(dt, dev, 1), ket=env.vec(C128, dev), n=env.N, out=out), [out]


def b_site_moments(env, dev, dt):
    src, M = _ints(1, 3), 6
    mu = np.full(2 * M * env.L * 2, np.nan)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, sources=src, ns=2, M=M, a=float(env.L), b=0.0, mu=mu), [mu]


def b_imag_evolve(env, dev, dt):
    out, ln = env.out(C128, dev), np.full(1, np.nan)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, tau=0.05, method=0, cheb_n=0, kry_m=8,
                Emin=-float(env.L), Emax=float(env.L), out=out, ln=ln), [out, ln]


def b_current_apply(env, dev, dt):
    out = env.out(C128, dev)
    w = _f(*[1.0 + 0.1 * b for b in range(env.L)])
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, w=w, out=out), [out]


def b_current_bracket(env, dev, dt):
    out = np.full(2, np.nan)
    w = _f(*[1.0 + 0.1 * b for b in range(env.L)])
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, bra=env.vec(dt, dev, 1), ket=env.vec(C128, dev), n=env.N, w=w, out=out), [out]


def b_dcurrent_apply(env, dev, dt):
    out = env.out(C128, dev)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, terms=_dterms(DLIST), n_terms=len(DLIST), out=out), [out]


def b_dcurrent_bracket(env, dev, dt):
    out = np.full(2, np.nan)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, bra=env.vec(dt, dev, 1), ket=env.vec(C128, dev), n=env.N, terms=_dterms(DLIST),
                n_terms=len(DLIST), out=out), [out]


def b_pair(env, dev, dt):
    out = np.full(2 * env.L * env.L, np.nan)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, component=1, out=out), [out]


def b_moments(env, dev, dt):
    out = np.full(5 + 2, np.nan)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, q=_f(2.0, 0.5), nq=2, out=out), [out]


def b_counting(env, dev, dt):
    masks = np.array([0b111, 0b101010], dtype=np.uint64)
    out = np.full(2 * (env.L + 1), np.nan)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, masks=masks, K=2, out=out), [out]


def b_sample(env, dev, dt):
    rows, cfg = np.full(7, -1, dtype=np.int64), np.full(7, 2 ** 63, dtype=np.uint64)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, shots=7, seed=5, rows=rows, cfg=cfg), [rows, cfg]


def b_bond(env, dev, dt):
    out = env.out(dt, dev)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, i=2, j=5, xy=0.8, zz=0.7, out=out), [out]


def b_dimer(env, dev, dt):
    bonds, B = _ints(1, 2, 3, 2, 2, 5, 6, 1, 4, 5), 5
    D, e = np.full(2 * B * B, np.nan), np.full(B, np.nan)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, bonds=bonds, B=B, xy=0.8, zz=0.7, D=D, e=e), [D, e]


def b_sym_apply(env, dev, dt):
    out = env.out(dt, dev)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, code=256 + 2, y=env.vec(dt, dev, 1), c_re=0.5,
                c_im=0.0 if dt == F64 else -0.25, out=out), [out]


def b_sym_overlaps(env, dev, dt):
    out = np.full(6, np.nan)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, bra=env.vec(dt, dev, 1), ket=env.vec(dt, dev), n=env.N, codes=_ints(0, 1, 256 + 3),
                n_codes=3, out=out), [out]


def b_sym_project(env, dev, dt):
    out = env.out(dt, dev)
    coef = _f(0.5, 0.0, 0.25, 0.0 if dt == F64 else 0.125, -1.0, 0.0)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, codes=_ints(0, 1, 256 + 3), coef=coef, n_codes=3,
                dtype_out=dt, out=out), [out]


def b_op_apply(env, dev, dt):
    out = env.out(dt, dev)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, terms=oplist(dt), n_terms=3, y=env.vec(dt, dev, 1),
                b_re=0.5, b_im=0.0 if dt == F64 else 0.75, dtype_out=dt, out=out), [out]


def b_op_expect(env, dev, dt):
    out = np.full(4, np.nan)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, bra=env.vec(dt, dev, 1), ket=env.vec(dt, dev), n=env.N, terms=oplist(dt, True),
                n_terms=5, out=out), [out]


def b_diag_apply(env, dev, dt):
    out = env.out(dt, dev)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, drives=_drives(env), K=2, coef=_f(0.3, -1.1),
                y=env.vec(dt, dev, 1), out=out), [out]


def b_driven_apply(env, dev, dt):
    out = env.out(dt, dev)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, drives=_drives(env), K=2, coef=_f(0.3, -1.1), out=out), [out]


def b_driven_evolve(env, dev, dt):
    out = env.out(C128, dev)
    info = env.pkg._lib.sd_driven_info()
    env.keep.append(info)
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, drives=_drives(env), K=2, n_stages=2, tau=_f(0.05, 0.1),
                coef=_f(0.3, -1.1, 0.0, 0.0), kry_m=6, out=out, info=info), [out]


def b_cut_gram(env, dev, dt):
    G = env.out(dt, False, _gram_elems(env, 3, 2))
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, cut=3, side=2, G=G), [G]


def b_permute(env, dev, dt):
    out = env.out(dt, dev)
    perm = _ints(*([3, 1, 2] + list(range(4, env.L + 1))))
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, perm=perm, out=out), [out]


def b_subsystem(env, dev, dt):
    G = env.out(dt, False, _gram_elems(env, 2, 2))
    return dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, sites=_ints(2, 5), n_sites=2, side=2, G=G), [G]


def _b_obs(with_q):
    def build(env, dev, dt):
        out = np.full(env.L, np.nan)
        a = dict(ctx=env.ctx, m=env.m.h, dtype=dt, psi=env.vec(dt, dev), n=env.N, out=out)
        if not with_q:
            return a, [out]
        q = np.full(env.L, np.nan)
        a["q"] = q
        return a, [q, out]
    return build


BOTH = (F64, C128)
ENTRIES = {
    "sd_site_project": ("ctx m dtype bra ket n out", b_site_project, BOTH),
    "sd_kpm_site_moments": ("ctx m dtype psi n sources ns M a b mu", b_site_moments, BOTH),
    "sd_imag_evolve": ("ctx m dtype psi n tau method cheb_n kry_m Emin Emax out ln", b_imag_evolve, BOTH),
    "sd_current_apply": ("ctx m dtype psi n w out", b_current_apply, BOTH),
    "sd_current_bracket": ("ctx m dtype bra ket n w out", b_current_bracket, BOTH),
    "sd_dcurrent_apply": ("ctx m dtype psi n terms n_terms out", b_dcurrent_apply, BOTH),
    "sd_dcurrent_bracket": ("ctx m dtype bra ket n terms n_terms out", b_dcurrent_bracket, BOTH),
    "sd_pair_correlations": ("ctx m dtype psi n component out", b_pair, BOTH),
    "sd_basis_moments": ("ctx m dtype psi n q nq out", b_moments, BOTH),
    "sd_counting_statistics": ("ctx m dtype psi n masks K out", b_counting, BOTH),
    "sd_sample_configurations": ("ctx m dtype psi n shots seed rows cfg", b_sample, BOTH),
    "sd_bond_apply": ("ctx m dtype psi n i j xy zz out", b_bond, BOTH),
    "sd_dimer_correlations": ("ctx m dtype psi n bonds B xy zz D e", b_dimer, BOTH),
    "sd_symmetry_apply": ("ctx m dtype psi n code y c_re c_im out", b_sym_apply, BOTH),
    "sd_symmetry_overlaps": ("ctx m dtype bra ket n codes n_codes out", b_sym_overlaps, BOTH),
    "sd_symmetry_project": ("ctx m dtype psi n codes coef n_codes dtype_out out", b_sym_project, BOTH),
    "sd_opstring_apply": ("ctx m dtype psi n terms n_terms y b_re b_im dtype_out out", b_op_apply, BOTH),
    "sd_opstring_expect": ("ctx m dtype bra ket n terms n_terms out", b_op_expect, BOTH),
    "sd_diag_apply": ("ctx m dtype psi n drives K coef y out", b_diag_apply, BOTH),
    "sd_driven_apply": ("ctx m dtype psi n drives K coef out", b_driven_apply, BOTH),
    "sd_driven_evolve": ("ctx m dtype psi n drives K n_stages tau coef kry_m out info", b_driven_evolve, BOTH),
    "sd_cut_gram": ("ctx m dtype psi n cut side G", b_cut_gram, BOTH),
    "sd_site_permute": ("ctx m dtype psi n perm out", b_permute, BOTH),
    "sd_subsystem_gram": ("ctx m dtype psi n sites n_sites side G", b_subsystem, BOTH),
    "sd_magnetization": ("ctx m dtype psi n out", _b_obs(False), BOTH),
    "sd_connected_correlations": ("ctx m dtype psi n out", _b_obs(False), BOTH),
    "sd_structure_factor": ("ctx m dtype psi n q out", _b_obs(True), BOTH),
}


def run(env, name, dev, dt, **over):
    order, build, _ = ENTRIES[name]
    args, outs = build(env, dev, dt)
    for k in ("m",):
        if over.get(k) == "@sharded":
            over[k] = env.sharded.h
        elif over.get(k) == "@bare":
            over[k] = env.bare.h
    return env.call(name, dev, order.split(), args, over, outs)


# ---- 1. the refusals ----
SELF, PART = ("@", "psi", 0), ("@", "psi", 8)
# (entry, forms: h host / d device, overrides of the valid ComplexF64 call, status, text)
REFUSALS = []


def rows(name, *table):
    for forms, over, status, text in table:
        REFUSALS.append((name, forms, over, status, text))


def common(name, tables=T_TABLES, sharded=T_SHARDED, length=T_LEN):
    """the model checks and the length check every core makes"""
    rows(name, ("hd", dict(m="@bare"), EARG, tables), ("hd", dict(m="@sharded"), EARG, sharded), ("hd", dict(n=19), EDIM, length))


common("sd_site_project")
rows("sd_site_project",
     ("hd", dict(m="@bare", n=19, ket=None), EARG, T_TABLES),
     ("hd", dict(ket=None), EARG, T_NULL), ("hd", dict(out=None), EARG, T_NULL),
     ("hd", dict(n=19, ket=None), EDIM, T_LEN),
     ("hd", dict(dtype=3), EARG, T_BAD), ("hd", dict(bra=None), EARG, T_NULL),
     ("hd", dict(dtype=3, n=19), EDIM, T_LEN), ("hd", dict(dtype=3, out=None), EARG, T_NULL), ("hd", dict(dtype=3, bra=None), EARG, T_BAD))

common("sd_kpm_site_moments", length="psi0 length does not match the basis dimension")
rows("sd_kpm_site_moments",
     ("hd", dict(dtype=3), EARG, T_BAD), ("hd", dict(psi=None), EARG, T_NULL),
     ("hd", dict(dtype=3, n=19), EDIM, "psi0 length does not match the basis dimension"), ("hd", dict(dtype=3, psi=None), EARG, T_BAD),
     ("hd", dict(M=1), EARG, "kpm_m must be >= 2"), ("hd", dict(psi=None, M=1), EARG, T_NULL))

common("sd_imag_evolve")
rows("sd_imag_evolve",
     ("hd", dict(out=None), EARG, T_NULL), ("hd", dict(ln=None), EARG, T_NULL), ("hd", dict(n=19, out=None), EDIM, T_LEN),
     ("hd", dict(dtype=3), EARG, T_BAD), ("hd", dict(psi=None), EARG, T_NULL), ("hd", dict(dtype=3, ln=None), EARG, T_NULL),
     ("hd", dict(tau=-1.0), EARG, "the imaginary time must be finite and >= 0"), ("hd", dict(tau=NAN), EARG, "the imaginary time must be finite and >= 0"),
     ("hd", dict(tau=-1.0, psi=None), EARG, T_NULL), ("hd", dict(cheb_n=-1), EARG, "cheb_n must be >= 0 (0: automatic)"),
     ("hd", dict(method=7), EARG, "unknown evolution method"))

common("sd_current_apply")
rows("sd_current_apply",
     ("hd", dict(out=None), EARG, T_NULL), ("hd", dict(n=19, out=None), EDIM, T_LEN), ("d", dict(out=SELF), EARG, T_ALIAS),
     ("hd", dict(w=_f(1, 1, NAN, 1, 1, 1)), EARG, "current weights must be finite"), ("d", dict(out=SELF, w=_f(1, 1, INF, 1, 1, 1)), EARG, T_ALIAS),
     ("hd", dict(dtype=3), EARG, T_BAD), ("hd", dict(psi=None), EARG, T_NULL),
     ("hd", dict(dtype=3, w=_f(1, 1, NAN, 1, 1, 1)), EARG, "current weights must be finite"), ("hd", dict(dtype=3, psi=None), EARG, T_BAD))

common("sd_current_bracket")
rows("sd_current_bracket",
     ("hd", dict(bra=None), EARG, T_NULL), ("hd", dict(bra=None, m="@bare"), EARG, T_NULL), ("hd", dict(out=None), EARG, T_NULL),
     ("hd", dict(n=19, out=None), EDIM, T_LEN), ("hd", dict(w=_f(1, 1, NAN, 1, 1, 1)), EARG, "current weights must be finite"),
     ("hd", dict(dtype=3), EARG, T_BAD), ("hd", dict(ket=None), EARG, T_NULL), ("hd", dict(dtype=3, ket=None), EARG, T_NULL))

for nm in ("sd_dcurrent_apply", "sd_dcurrent_bracket"):
    common(nm)
    rows(nm,
         ("hd", dict(dtype=3), EARG, T_DTYPE), ("hd", dict(dtype=3, n=19), EARG, T_DTYPE), ("hd", dict(out=None), EARG, T_NULL),
         ("hd", dict(n=19, out=None), EDIM, T_LEN),
         ("hd", dict(n_terms=-1), EARG, "the number of terms must be in 0..SD_DTERM_MAX"),
         ("hd", dict(n_terms=4097), EARG, "the number of terms must be in 0..SD_DTERM_MAX"),
         ("hd", dict(terms=None), EARG, T_NULL), ("hd", dict(terms=None, n_terms=4097), EARG, "the number of terms must be in 0..SD_DTERM_MAX"),
         ("hd", dict(terms=_dterms([(1, 2, 0, 1.0), (1, 7, 0, 1.0), (2, 2, 0, 1.0), (1, 2, 0, 1.0)])), EARG, "a site of a term is outside 1..L (k may also be 0)"),
         ("hd", dict(terms=_dterms([(0, 2, 0, 1.0)]), n_terms=1), EARG, "a site of a term is outside 1..L (k may also be 0)"),
         ("hd", dict(terms=_dterms([(1, 2, 7, 1.0)]), n_terms=1), EARG, "a site of a term is outside 1..L (k may also be 0)"),
         ("hd", dict(terms=_dterms([(2, 2, 2, NAN)]), n_terms=1), EARG, "the two sites of a bond current must differ"),
         ("hd", dict(terms=_dterms([(1, 2, 1, NAN)]), n_terms=1), EARG, "the S^z site of a term must not be one of its bond's sites"),
         ("hd", dict(terms=_dterms([(1, 2, 2, 1.0)]), n_terms=1), EARG, "the S^z site of a term must not be one of its bond's sites"),
         ("hd", dict(terms=_dterms([(1, 2, 3, INF)]), n_terms=1), EARG, "the coefficients must be finite"))
rows("sd_dcurrent_apply",
     ("hd", dict(psi=None), EARG, T_NULL), ("d", dict(out=SELF), EARG, T_ALIAS), ("d", dict(out=SELF, n_terms=-1), EARG, T_ALIAS),
     ("hd", dict(psi=None, n_terms=-1), EARG, T_NULL))
rows("sd_dcurrent_bracket",
     ("hd", dict(bra=None), EARG, T_NULL), ("hd", dict(bra=None, m="@bare"), EARG, T_NULL), ("hd", dict(ket=None), EARG, T_NULL),
     ("hd", dict(ket=None, n_terms=-1), EARG, T_NULL))

common("sd_pair_correlations")
rows("sd_pair_correlations",
     ("hd", dict(component=2), EARG, "component must be SD_PAIR_ZZ or SD_PAIR_PM"), ("hd", dict(component=-1, n=19), EARG, "component must be SD_PAIR_ZZ or SD_PAIR_PM"),
     ("hd", dict(out=None), EARG, T_NULL), ("hd", dict(n=19, out=None), EDIM, T_LEN),
     ("hd", dict(dtype=3), EARG, T_BAD), ("hd", dict(psi=None), EARG, T_NULL), ("hd", dict(dtype=3, out=None), EARG, T_NULL),
     ("hd", dict(dtype=0, psi=None), EARG, T_BAD))

common("sd_basis_moments")
rows("sd_basis_moments",
     ("hd", dict(out=None), EARG, T_NULL), ("hd", dict(q=None), EARG, T_NULL), ("hd", dict(n=19, q=None), EDIM, T_LEN),
     ("hd", dict(nq=-1), EARG, "basis moments: between 0 and SD_MOMENT_MAX_Q exponents"),
     ("hd", dict(nq=9, q=_f(*[2.0] * 9)), EARG, "basis moments: between 0 and SD_MOMENT_MAX_Q exponents"),
     ("hd", dict(nq=9, q=None), EARG, T_NULL), ("hd", dict(nq=-1, q=None, dtype=3), EARG, "basis moments: between 0 and SD_MOMENT_MAX_Q exponents"),
     ("hd", dict(dtype=3), EARG, T_BAD), ("hd", dict(psi=None), EARG, T_NULL),
     ("hd", dict(q=_f(2.0, 1.0)), EARG, "basis moments: every exponent must be finite, positive and not 1 (q = 1 is the Shannon term, always returned)"))

common("sd_counting_statistics")
rows("sd_counting_statistics",
     ("hd", dict(out=None), EARG, T_NULL), ("hd", dict(masks=None), EARG, T_NULL), ("hd", dict(n=19, masks=None), EDIM, T_LEN),
     ("hd", dict(K=0), EARG, "counting statistics: between 1 and SD_COUNT_MAX_MASKS masks"),
     ("hd", dict(K=257), EARG, "counting statistics: between 1 and SD_COUNT_MAX_MASKS masks"), ("hd", dict(K=0, out=None), EARG, T_NULL),
     ("hd", dict(dtype=3), EARG, T_BAD), ("hd", dict(psi=None), EARG, T_NULL), ("hd", dict(K=0, psi=None), EARG, "counting statistics: between 1 and SD_COUNT_MAX_MASKS masks"),
     ("hd", dict(masks=np.array([1, 64], dtype=np.uint64)), EARG, "counting statistics: a mask has a bit at or above L"))

common("sd_sample_configurations")
rows("sd_sample_configurations",
     ("hd", dict(shots=-1), EARG, "snapshots: a negative number of shots"), ("hd", dict(shots=-1, n=19), EDIM, T_LEN),
     ("hd", dict(cfg=None), EARG, T_NULL), ("hd", dict(shots=-1, cfg=None), EARG, "snapshots: a negative number of shots"),
     ("hd", dict(rows=None), 0, ""), ("hd", dict(dtype=3), EARG, T_BAD), ("hd", dict(psi=None), EARG, T_NULL),
     ("hd", dict(psi=None, cfg=None), EARG, T_NULL))

common("sd_bond_apply")
rows("sd_bond_apply",
     ("hd", dict(dtype=3), EARG, T_DTYPE), ("hd", dict(dtype=3, i=0), EARG, T_DTYPE),
     ("hd", dict(i=0), EARG, "a bond site is outside 1..L"), ("hd", dict(j=7), EARG, "a bond site is outside 1..L"),
     ("hd", dict(i=3, j=3), EARG, "the two sites of a bond must differ"), ("hd", dict(i=7, j=7), EARG, "a bond site is outside 1..L"),
     ("hd", dict(xy=NAN), EARG, "the bond weights must be finite"), ("hd", dict(zz=INF), EARG, "the bond weights must be finite"),
     ("hd", dict(i=3, j=3, xy=NAN), EARG, "the two sites of a bond must differ"), ("hd", dict(xy=NAN, n=19), EARG, "the bond weights must be finite"),
     ("hd", dict(out=None), EARG, T_NULL), ("hd", dict(n=19, out=None), EDIM, T_LEN), ("d", dict(out=SELF), EARG, T_ALIAS),
     ("hd", dict(psi=None), EARG, T_NULL))

common("sd_dimer_correlations")
rows("sd_dimer_correlations",
     ("hd", dict(dtype=3), EARG, T_DTYPE), ("hd", dict(dtype=3, B=0), EARG, T_DTYPE),
     ("hd", dict(B=0), EARG, "the number of bonds must be in 1..SD_DIMER_MAX_BONDS"), ("hd", dict(B=129), EARG, "the number of bonds must be in 1..SD_DIMER_MAX_BONDS"),
     ("hd", dict(B=0, bonds=None), EARG, "the number of bonds must be in 1..SD_DIMER_MAX_BONDS"),
     ("hd", dict(bonds=None), EARG, T_NULL), ("hd", dict(D=None), EARG, T_NULL), ("hd", dict(e=None), EARG, T_NULL),
     ("hd", dict(bonds=_ints(1, 2, 3, 7, 2, 2, 1, 2, 1, 2)), EARG, "a bond site is outside 1..L"),
     ("hd", dict(bonds=_ints(1, 2, 2, 2, 3, 7, 1, 2, 1, 2)), EARG, "the two sites of a bond must differ"),
     ("hd", dict(bonds=_ints(1, 2, 2, 2, 3, 4, 1, 2, 1, 2), e=None), EARG, T_NULL),
     ("hd", dict(xy=INF), EARG, "the bond weights must be finite"), ("hd", dict(zz=NAN, n=19), EARG, "the bond weights must be finite"),
     ("hd", dict(psi=None), EARG, T_NULL), ("hd", dict(psi=None, n=19), EDIM, T_LEN))

T_CODE = "element code: the shift must be in 0..L-1 and no bit above bit 9 set"
common("sd_symmetry_apply")
rows("sd_symmetry_apply",
     ("hd", dict(dtype=3), EARG, T_DTYPE), ("hd", dict(dtype=3, code=6), EARG, T_DTYPE),
     ("hd", dict(code=6), EARG, T_CODE), ("hd", dict(code=-1), EARG, T_CODE), ("hd", dict(code=1024), EARG, T_CODE),
     ("hd", dict(c_re=NAN), EARG, "the coefficient must be finite"), ("hd", dict(c_im=INF), EARG, "the coefficient must be finite"),
     ("hd", dict(code=6, c_re=NAN), EARG, T_CODE), ("hd", dict(y=None, c_re=NAN), 0, ""),
     ("hd", dict(dtype=1, c_im=0.5), EARG, "a Float64 vector takes a real coefficient (c_im = 0)"),
     ("hd", dict(dtype=1, c_im=0.5, n=19), EARG, "a Float64 vector takes a real coefficient (c_im = 0)"),
     ("hd", dict(out=None), EARG, T_NULL), ("hd", dict(psi=None), EARG, T_NULL), ("hd", dict(n=19, psi=None), EDIM, T_LEN),
     ("d", dict(out=SELF), EARG, T_OVERLAP), ("d", dict(out=PART), EARG, T_OVERLAP), ("d", dict(out=("@", "psi", -16 * 19)), EARG, T_OVERLAP),
     ("d", dict(out=("@", "y", 16)), EARG, T_YPART),
     ("d", dict(out=SELF, y=("@", "psi", 16)), EARG, T_OVERLAP))

common("sd_symmetry_overlaps")
rows("sd_symmetry_overlaps",
     ("hd", dict(dtype=3), EARG, T_DTYPE), ("hd", dict(dtype=3, ket=None), EARG, T_DTYPE),
     ("hd", dict(ket=None), EARG, T_NULL), ("hd", dict(out=None), EARG, T_NULL), ("hd", dict(bra=None), 0, ""),
     ("hd", dict(n_codes=0), EARG, "the number of elements must be in 1..SD_SYM_MAX_ELEMENTS"),
     ("hd", dict(n_codes=253), EARG, "the number of elements must be in 1..SD_SYM_MAX_ELEMENTS"),
     ("hd", dict(n_codes=0, out=None), EARG, T_NULL), ("hd", dict(codes=None), EARG, T_NULL),
     ("hd", dict(codes=None, n_codes=0), EARG, "the number of elements must be in 1..SD_SYM_MAX_ELEMENTS"),
     ("hd", dict(codes=_ints(0, 6, 1)), EARG, T_CODE), ("hd", dict(codes=_ints(0, 6, 1), n=19), EARG, T_CODE))

common("sd_symmetry_project")
rows("sd_symmetry_project",
     ("hd", dict(dtype=3), EARG, T_DTYPE), ("hd", dict(dtype_out=3), EARG, "dtype_out must be SD_F64 or SD_C128"), ("hd", dict(dtype=3, dtype_out=3), EARG, T_DTYPE),
     ("hd", dict(coef=None), EARG, T_NULL), ("hd", dict(out=None), EARG, T_NULL), ("hd", dict(psi=None), EARG, T_NULL),
     ("hd", dict(dtype_out=0, coef=None), EARG, "dtype_out must be SD_F64 or SD_C128"),
     ("hd", dict(n_codes=0), EARG, "the number of elements must be in 1..SD_SYM_MAX_ELEMENTS"), ("hd", dict(n_codes=0, psi=None), EARG, T_NULL),
     ("hd", dict(codes=None), EARG, T_NULL), ("hd", dict(codes=_ints(1024, 0, 1)), EARG, T_CODE),
     ("hd", dict(coef=_f(1, 0, NAN, 0, 1, 0)), EARG, "the coefficients must be finite"),
     ("hd", dict(coef=_f(1, 0, 1, 0, 1, INF), codes=_ints(0, 6, 1)), EARG, T_CODE),
     ("hd", dict(dtype_out=1), EARG, "an SD_F64 result needs an SD_F64 psi"), ("hd", dict(dtype_out=1, n_codes=253), EARG, "the number of elements must be in 1..SD_SYM_MAX_ELEMENTS"),
     ("hd", dict(dtype=1, dtype_out=1), EARG, "an SD_F64 result needs real coefficients"),
     ("hd", dict(dtype=1, dtype_out=1, n=19), EARG, "an SD_F64 result needs real coefficients"),
     ("d", dict(out=SELF), EARG, T_OVERLAP), ("d", dict(out=PART), EARG, T_OVERLAP), ("d", dict(out=SELF, n=19), EDIM, T_LEN),
     ("d", dict(dtype=1, out=("@", "psi", 8 * 19)), EARG, T_OVERLAP))

common("sd_opstring_apply")
rows("sd_opstring_apply",
     ("hd", dict(dtype=3), EARG, T_DTYPE), ("hd", dict(dtype_out=3), EARG, "dtype_out must be SD_F64 or SD_C128"), ("hd", dict(dtype=0, dtype_out=3), EARG, T_DTYPE),
     ("hd", dict(n_terms=-1), EARG, "the number of terms must be in 0..SD_OPTERM_MAX"), ("hd", dict(n_terms=-1, dtype_out=3), EARG, "dtype_out must be SD_F64 or SD_C128"),
     ("hd", dict(terms=None), EARG, T_NULL), ("hd", dict(terms=_opterms([(1, 1, 0, 1.0, 0.0, 0)]), n_terms=1), EARG, "the plus, minus and z masks of a term must be pairwise disjoint"),
     ("hd", dict(terms=_opterms([(1, 2, 0, 1.0, 0.0, 0), (2, 1, 0, 1.0, 0.0, 1)]), n_terms=2), EARG, "the write form takes one operator: every term must have op = 0"),
     ("hd", dict(terms=_opterms([(1, 2, 0, 1.0, 0.0, 0), (2, 1, 0, 1.0, 0.0, 1)]), n_terms=2, b_re=NAN), EARG, "the write form takes one operator: every term must have op = 0"),
     ("hd", dict(b_re=NAN), EARG, "the coefficient b must be finite"), ("hd", dict(b_im=INF), EARG, "the coefficient b must be finite"),
     ("hd", dict(y=None, b_re=NAN), 0, ""), ("hd", dict(b_re=NAN, dtype_out=1), EARG, "the coefficient b must be finite"),
     ("hd", dict(dtype_out=1), EARG, "an SD_F64 output needs an SD_F64 psi"),
     ("hd", dict(dtype=1, dtype_out=1, b_im=0.0), EARG, "an SD_F64 output needs real coefficients (every c_im = 0)"),
     ("hd", dict(dtype=1, dtype_out=1), EARG, "an SD_F64 output needs real coefficients (every c_im = 0)"),
     ("hd", dict(dtype=1, dtype_out=1, terms=oplist(F64)), EARG, "an SD_F64 output takes a real b (b_im = 0)"),
     ("hd", dict(dtype=1, dtype_out=1, terms=oplist(F64), n=19), EARG, "an SD_F64 output takes a real b (b_im = 0)"),
     ("hd", dict(out=None), EARG, T_NULL), ("hd", dict(psi=None), EARG, T_NULL), ("hd", dict(n=19, out=None), EDIM, T_LEN),
     ("d", dict(out=SELF), EARG, T_OVERLAP), ("d", dict(out=PART), EARG, T_OVERLAP), ("d", dict(out=SELF, psi=None), EARG, T_NULL),
     ("d", dict(out=("@", "y", -16)), EARG, T_YPART), ("d", dict(out=SELF, y=("@", "psi", 16)), EARG, T_OVERLAP))

common("sd_opstring_expect")
rows("sd_opstring_expect",
     ("hd", dict(dtype=3), EARG, T_DTYPE), ("hd", dict(dtype=3, n_terms=-1), EARG, T_DTYPE),
     ("hd", dict(n_terms=4097), EARG, "the number of terms must be in 0..SD_OPTERM_MAX"), ("hd", dict(n_terms=4097, n=19), EARG, "the number of terms must be in 0..SD_OPTERM_MAX"),
     ("hd", dict(terms=None), EARG, T_NULL),
     ("hd", dict(terms=_opterms([(1, 0, 0, 1.0, 0.0, 0)]), n_terms=1), EARG, "in a fixed-nup sector every term needs as many S^+ as S^- factors"),
     ("hd", dict(ket=None), EARG, T_NULL), ("hd", dict(n=19, ket=None), EDIM, T_LEN), ("hd", dict(out=None), EARG, T_NULL),
     ("hd", dict(out=None, n_terms=0), 0, ""), ("hd", dict(ket=None, n_terms=0), EARG, T_NULL), ("hd", dict(bra=None), 0, ""))

T_DRIVES = "the number of drives must be 0..16"
for nm in ("sd_diag_apply", "sd_driven_apply"):
    common(nm)
    rows(nm,
         ("hd", dict(dtype=3), EARG, T_DTYPE), ("hd", dict(dtype=3, coef=None), EARG, T_DTYPE),
         ("hd", dict(coef=None), EARG, "null coefficients"), ("hd", dict(coef=None, K=17), EARG, "null coefficients"),
         ("hd", dict(K=17), EARG, T_DRIVES), ("hd", dict(K=-1), EARG, T_DRIVES), ("hd", dict(drives=None), EARG, "null drive list"),
         ("hd", dict(coef=_f(0.3, NAN)), EARG, "drive coefficient 1 is not finite"), ("hd", dict(K=17, n=19), EARG, T_DRIVES),
         ("hd", dict(psi=None), EARG, T_NULL), ("hd", dict(out=None), EARG, T_NULL), ("hd", dict(n=19, psi=None), EDIM, T_LEN),
         ("d", dict(out=SELF), EARG, T_ALIAS), ("d", dict(out=SELF, n=19), EDIM, T_LEN), ("hd", dict(K=0, coef=None, drives=None), 0, ""))

common("sd_driven_evolve")
rows("sd_driven_evolve",
     ("hd", dict(psi=None), EARG, "null vector"), ("hd", dict(out=None), EARG, "null vector"), ("hd", dict(psi=None, m="@sharded"), EARG, T_SHARDED),
     ("hd", dict(n_stages=0), EARG, "a driven evolution needs at least one stage and its durations"),
     ("hd", dict(tau=None), EARG, "a driven evolution needs at least one stage and its durations"),
     ("hd", dict(n_stages=0, out=None), EARG, "null vector"), ("hd", dict(coef=None), EARG, "null coefficients"),
     ("hd", dict(coef=None, tau=None), EARG, "a driven evolution needs at least one stage and its durations"),
     ("hd", dict(dtype=3), EARG, T_BAD), ("hd", dict(dtype=3, coef=None), EARG, "null coefficients"), ("hd", dict(dtype=3, n=19), EARG, T_BAD),
     ("hd", dict(kry_m=0), EARG, "kry_m must be >= 1"), ("hd", dict(kry_m=0, n=19), EDIM, T_LEN),
     ("hd", dict(K=17), EARG, T_DRIVES), ("hd", dict(K=17, kry_m=0), EARG, "kry_m must be >= 1"),
     ("hd", dict(tau=_f(0.05, INF)), EARG, "a stage duration is not finite"), ("hd", dict(tau=_f(0.05, INF), K=17), EARG, T_DRIVES),
     ("hd", dict(coef=_f(0.3, -1.1, NAN, 0.0)), EARG, "a stage coefficient is not finite"),
     ("hd", dict(coef=_f(NAN, -1.1, 0.0, 0.0), tau=_f(0.05, NAN)), EARG, "a stage coefficient is not finite"),
     ("hd", dict(info=None), 0, ""))

T_CUT_SHARDED = "entanglement needs an unsharded model"
common("sd_cut_gram", tables=T_TABLES_CTX, sharded=T_CUT_SHARDED)
rows("sd_cut_gram",
     ("hd", dict(m=None), EARG, T_NULL), ("hd", dict(psi=None), EARG, T_NULL), ("hd", dict(G=None), EARG, T_NULL), ("hd", dict(psi=None, m="@bare"), EARG, T_NULL),
     ("hd", dict(dtype=3), EARG, T_DTYPE), ("hd", dict(dtype=3, m="@bare"), EARG, T_TABLES_CTX), ("hd", dict(dtype=3, cut=0), EARG, T_DTYPE),
     ("hd", dict(side=3), EARG, "side must be SD_CUT_A, SD_CUT_B or SD_CUT_AUTO"), ("hd", dict(cut=0), EARG, "the cut must be in 1..L-1"),
     ("hd", dict(cut=6), EARG, "the cut must be in 1..L-1"), ("hd", dict(cut=6, n=19), EARG, "the cut must be in 1..L-1"))

T_PERM_SHARDED = "site permutations need an unsharded model"
common("sd_site_permute", tables=T_TABLES_CTX, sharded=T_PERM_SHARDED)
rows("sd_site_permute",
     ("hd", dict(m=None), EARG, T_NULL), ("hd", dict(psi=None), EARG, T_NULL), ("hd", dict(perm=None), EARG, T_NULL), ("hd", dict(out=None), EARG, T_NULL),
     ("hd", dict(out=None, m="@bare"), EARG, T_NULL), ("hd", dict(dtype=3), EARG, T_DTYPE), ("hd", dict(dtype=3, m="@bare"), EARG, T_TABLES_CTX),
     ("hd", dict(dtype=3, m="@sharded"), EARG, T_DTYPE), ("hd", dict(perm=_ints(1, 1, 2, 3, 4, 5)), EARG, "perm must be a bijection of 1..L"),
     ("hd", dict(perm=_ints(0, 1, 2, 3, 4, 5)), EARG, "perm must be a bijection of 1..L"), ("hd", dict(perm=_ints(1, 1, 2, 3, 4, 5), n=19), EARG, "perm must be a bijection of 1..L"),
     ("hd", dict(perm=_ints(1, 1, 2, 3, 4, 5), m="@sharded"), EARG, T_PERM_SHARDED),
     ("hd", dict(out=SELF), EARG, T_OVERLAP), ("hd", dict(out=PART), EARG, T_OVERLAP), ("hd", dict(out=("@", "psi", -16 * 19)), EARG, T_OVERLAP),
     ("hd", dict(out=SELF, n=19), EDIM, T_LEN))

T_SITES = "the sites must be distinct, in 1..L, and 1 <= n_sites <= L - 1"
common("sd_subsystem_gram", tables=T_TABLES_CTX, sharded=T_PERM_SHARDED)
rows("sd_subsystem_gram",
     ("hd", dict(m=None), EARG, T_NULL), ("hd", dict(psi=None), EARG, T_NULL), ("hd", dict(sites=None), EARG, T_NULL), ("hd", dict(G=None), EARG, T_NULL),
     ("hd", dict(sites=_ints(2, 2)), EARG, T_SITES), ("hd", dict(sites=_ints(2, 7)), EARG, T_SITES), ("hd", dict(n_sites=0), EARG, T_SITES),
     ("hd", dict(sites=_ints(1, 2, 3, 4, 5, 6), n_sites=6), EARG, T_SITES), ("hd", dict(sites=_ints(2, 2), G=None), EARG, T_NULL),
     ("hd", dict(sites=_ints(2, 2), m="@bare"), EARG, T_SITES), ("hd", dict(dtype=3), EARG, T_DTYPE), ("hd", dict(dtype=3, side=3), EARG, T_DTYPE),
     ("hd", dict(side=3), EARG, "side must be SD_CUT_A, SD_CUT_B or SD_CUT_AUTO"), ("hd", dict(side=3, n=19), EARG, "side must be SD_CUT_A, SD_CUT_B or SD_CUT_AUTO"),
     ("hd", dict(sites=_ints(1, 2), m="@sharded"), EARG, T_PERM_SHARDED))

for nm in ("sd_magnetization", "sd_connected_correlations", "sd_structure_factor"):
    rows(nm,
         ("hd", dict(m=None), EARG, T_NULL), ("hd", dict(psi=None), EARG, T_NULL), ("hd", dict(out=None), EARG, T_NULL), ("hd", dict(n=19), EDIM, T_LEN),
         ("hd", dict(psi=None, n=19), EARG, T_NULL), ("h", dict(dtype=3), EARG, T_BAD), ("h", dict(dtype=3, n=19), EARG, T_BAD),
         ("hd", dict(m="@sharded"), EARG, "observables need an unsharded model"), ("d", dict(m="@sharded", n=19), EARG, "observables need an unsharded model"),
         ("h", dict(m="@sharded", n=19), EDIM, T_LEN))
rows("sd_structure_factor", ("hd", dict(q=None), 0, ""))


@pytest.fixture(scope="module")
def env6(pkg):
    e = Env(pkg, 6, 3)
    e.sharded = pkg.XXZChain(6, Jxy=0.8, Jz=0.7, hz=0.0, nup=3, boundary="periodic")
    e.sharded.set_shard(0, 2)
    e.bare = pkg.XXZChain(6, Jxy=0.8, Jz=0.7, hz=0.0, nup=3, boundary="periodic", ctx=None)
    return e


def same_bits(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_refusals(env6, name):
    """every row of REFUSALS for this entry: status and text, then the valid call again, with the bits it gave before"""
    mine = [r for r in REFUSALS if r[0] == name]
    assert mine
    good = {dev: run(env6, name, dev, C128) for dev in (False, True)}
    for dev in good:
        assert good[dev][0] == 0, (name, dev, good[dev][1])
    failures = []
    for k, (_, forms, over, status, text) in enumerate(mine):
        for dev in (False, True):
            if ("d" if dev else "h") not in forms:
                continue
            rc, msg, _ = run(env6, name, dev, C128, **dict(over))
            if rc != status or (status != 0 and msg != text):
                failures.append((k, "dev" if dev else "host", over, (rc, msg), (status, text)))
            for form in (dev, not dev):
                again = run(env6, name, form, C128)
                if again[0] != 0 or not same_bits(again[2], good[form][2]):
                    failures.append((k, "the valid call after the refusal", over, again[:2]))
    assert not failures, failures


# ---- 2. host form == device form ----
SHAPES = {"tiled": (10, 5, 252, "tiled"), "per_row": (13, 1, 13, "generic"), "full": (7, None, 128, "generic")}


@pytest.fixture(scope="module", params=sorted(SHAPES))
def env(pkg, request):
    L, nup, N, path = SHAPES[request.param]
    e = Env(pkg, L, nup, seed=23)
    assert e.N == N and e.m.device_path == path, (e.N, e.m.device_path)
    return e


@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_host_form_equals_device_form(env, name):
    for dt in ENTRIES[name][2]:
        h = run(env, name, False, dt)
        d = run(env, name, True, dt)
        assert h[0] == 0 and d[0] == 0, (name, dt, h[:2], d[:2])
        for a in h[2]:
            assert not np.isnan(a.view(np.float64) if a.dtype.kind in "fc" else a.astype(np.float64)).any(), (name, dt, "the host form left an output unwritten")
        assert same_bits(h[2], d[2]), (name, dt)


# ---- 3. empty inputs ----
def test_empty_inputs(env6):
    e = env6
    for dev in (False, True):
        for dt in BOTH:
            # the empty list of dressed currents: J = 0, so the write form writes zeros and the bracket is zero
            rc, msg, (out,) = run(e, "sd_dcurrent_apply", dev, dt, n_terms=0, terms=None)
            assert rc == 0 and not out.any() and out.shape == (e.N,), (dev, dt, msg)
            rc, msg, (br,) = run(e, "sd_dcurrent_bracket", dev, dt, n_terms=0, terms=None)
            assert rc == 0 and br.tolist() == [0.0, 0.0], (dev, dt, msg)
            # the empty operator string: out = 0 psi + b y, and without y zeros
            rc, msg, (out,) = run(e, "sd_opstring_apply", dev, dt, n_terms=0, terms=None, y=None)
            assert rc == 0 and not out.any(), (dev, dt, msg)
            rc, msg, (out,) = run(e, "sd_opstring_apply", dev, dt, n_terms=0, terms=None, b_re=1.0, b_im=0.0)
            assert rc == 0 and out.tobytes() == e.host[dt, 1].tobytes(), (dev, dt, msg)
            # no operator: nothing is written, with or without a place to write to
            rc, msg, (ex,) = run(e, "sd_opstring_expect", dev, dt, n_terms=0, terms=None)
            assert rc == 0 and np.isnan(ex).all(), (dev, dt, msg)
            assert run(e, "sd_opstring_expect", dev, dt, n_terms=0, terms=None, out=None)[0] == 0
            # no shots: nothing is written
            rc, msg, (rws, cfg) = run(e, "sd_sample_configurations", dev, dt, shots=0)
            assert rc == 0 and (rws == -1).all() and (cfg == 2 ** 63).all(), (dev, dt, msg)
            assert run(e, "sd_sample_configurations", dev, dt, shots=0, rows=None, cfg=None)[0] == 0
            # no exponents: the five fixed figures alone
            rc, msg, (mo,) = run(e, "sd_basis_moments", dev, dt, nq=0, q=None)
            assert rc == 0 and not np.isnan(mo[:5]).any() and np.isnan(mo[5:]).all(), (dev, dt, msg)
            # no drive: the diagonal operator is zero (out = y), the driven one is H0
            rc, msg, (out,) = run(e, "sd_diag_apply", dev, dt, K=0, drives=None, coef=None)
            assert rc == 0 and out.tobytes() == e.host[dt, 1].tobytes(), (dev, dt, msg)
            rc, msg, (out,) = run(e, "sd_diag_apply", dev, dt, K=0, drives=None, coef=None, y=None)
            assert rc == 0 and not out.any(), (dev, dt, msg)
    # the device write form of the empty operator string queues its kernel and returns without waiting for it (no table went to the
    # pool): the result is complete once the stream has drained, which Env.call does before it reads
    rc, msg, (a,) = run(e, "sd_opstring_apply", True, C128, n_terms=0, terms=None)
    rc2, _, (b,) = run(e, "sd_opstring_apply", False, C128, n_terms=0, terms=None)
    assert rc == 0 and rc2 == 0 and a.tobytes() == b.tobytes(), msg
