"""The vector kernels of csrc/kernels_blas1.hip one launcher at a time, through tests/blas1_shim.cpp (a host unit that forwards to
the sd_k_* launchers; the link against libspindyn.so is the signature check).  The recursion tests see these kernels only through
whole ground-state runs at |dE0| <= 1e-10 and 1e-6 on the vector, where a skipped column of the re-orthogonalisation, a misfiled
check dot, a repair read from the wrong column or a dropped column of the eigenvector sum change nothing that is looked at.

Yardsticks (tests/blas1_ref.py, proven on the CPU by tests/test_blas1_ref_host.py):
  bit for bit   the per-element arithmetic the kernel comments fix (x - c*v in column order, (w - a*vj) - b*vjm1, w - d*vjm1, w / b,
                s += V*c from 0.0, the component-wise complex accumulation) with the coefficients the device itself summed, read
                back from the caller-owned partial lists and summed in the kernels' fixed order (sum_cols)
  fsum          every reduced value against math.fsum of the kernel's own terms, bar n 2^-53 sum |term| (any order of additions)
  bounded       the chains whose coefficients stay in the context's scratch (mgs, bgs; gs_chain past 16 projected columns, and all
                others as well) against the chain in np.longdouble under chain_bound(), which is a condition, not a measurement,
                and must itself stay <= 1e-8 max|w_ref|: nine orders below a skipped column or element (inputs with O(1)
                coefficients on orthonormal columns)
Every output, scratch list and padding region is NaN before the call; a NaN where a value is due, or a value where none is due, fails.

Shapes: N in {1, 2, 3, 511, 512, 513, 1025} for single blocks and tails (no more columns than N: there are no more orthonormal
ones), all four alignment forms -- (a) aligned bases, even ld; (b) odd ld; (c) w one double past an aligned base; (d) ld = N + 3
with NaN rows -- and 1, 2, 8, 9, 10, 16, 17, 18, 25, 26 columns; then the sizes that cross the launchers' caps, asserted per cell:
1024 blocks of 256 pairs (N = 524 801, 524 802), 2048 for k_gs_scale (1 048 579), 16384 blocks of 256 items (4 194 563 items;
8 389 123 doubles for the chains that count pairs).

Figures on an MI355X.  379 vector comparisons bit for bit, 0 elements differ.  fsum checks (5803): largest error / bar 0.60 at N = 3,
where the bar is 1.7 ulp; at the cap sizes 5.9e-6 (gs_chain alpha and check dots, 1.8e-15 against 3.0e-10), 5.7e-6 (gs_update),
3.5e-7 (mgs / bgs slot, 2.2e-16 against 6.4e-10), 1.4e-9 (mdot), 7.0e-10 (dotu, dot_to), 2.4e-7 (nrm2sq_to).  Bounded comparisons:
largest error / bound 0.14 (N = 3, ncols = 2: 2.1e-16 against 1.4e-15); the cap sizes are in the docstrings of their tests.
Run time on an MI355X: 195 cells in 29 s, most of it the host arithmetic of the references; the cap cells take 0.3 - 1.0 s
(gs_chain), 1.0 - 5.4 s (mgs / bgs at 8 389 123 x 10: the first cell pays for the QR and the longdouble chain, 5.4 s), 1.2 s
(mdot, 571 MB), 1.4 s (complex dots), under 0.9 s (all others)."""
import ctypes as C
import functools
import gc
import math
from types import SimpleNamespace

import numpy as np
import pytest

import blas1_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
U = 2.0 ** -53
BS = 256
GS_BLOCKS, GS_SCALE_BLOCKS, RED_BLOCKS = 1024, 2048, 16384      # caps of csrc/kernels_blas1.hip
CAP = RED_BLOCKS * BS
SMALL = [1, 2, 3, 511, 512, 513, 1025]
NCOLS = [1, 2, 8, 9, 10, 16, 17, 18, 25, 26]
N_GS_WRAP = [524_801, 524_802]
N_SCALE_WRAP = 1_048_579
N_CAP = 4_194_563
N_CHAIN_CAP = 8_389_123
FORMS = ["a", "b", "c", "d"]


@pytest.fixture(scope="module")
def e(pkg, tmp_path_factory):
    import torch
    shim = R.build_shim(pkg, tmp_path_factory.mktemp("blas1_shim"))
    ctx = pkg.default_context()
    yield SimpleNamespace(pkg=pkg, shim=shim, ctx=ctx, torch=torch, dev=torch.device("cuda", ctx.device))
    _chain_inputs.cache_clear()
    _chain_ref.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


def call(e, name, *args):
    e.ctx.set_stream(e.torch.cuda.current_stream().cuda_stream)
    e.pkg.check(getattr(e.shim, name)(e.ctx.h, *args), e.ctx.h)


def nans(e, n, cplx=False):
    t = e.torch
    return t.full((n,), complex(NAN, NAN) if cplx else NAN, dtype=t.complex128 if cplx else t.float64, device=e.dev)


class Vec:
    """a device vector `off` elements past an aligned base with NaN before it and behind it; .t is the view the kernel gets"""

    def __init__(self, e, data=None, n=None, off=0, cplx=False):
        self.e = e
        if data is not None:
            data = np.array(data)                                             # a copy: the shared inputs are read-only
            n, cplx = len(data), np.iscomplexobj(data)
        self.n, self.off = n, off
        self.buf = nans(e, off + n + 3, cplx)
        assert self.buf.data_ptr() % 256 == 0
        self.t = self.buf[off:off + n]
        if data is not None:
            self.t.copy_(e.torch.from_numpy(data))
        self.ptr = self.t.data_ptr()

    def get(self):
        """the vector on the host; the guards must still be NaN"""
        h = self.buf.cpu().numpy()
        assert np.isnan(h[:self.off]).all() and np.isnan(h[self.off + self.n:]).all(), "a guard element was written"
        return h[self.off:self.off + self.n].copy()


def columns(e, V, N, ld):
    """V (ncols, N) on the host -> a device matrix of ncols columns `ld` doubles apart, rows N..ld-1 NaN"""
    t = e.torch.full((V.shape[0], ld), NAN, dtype=e.torch.float64, device=e.dev)
    t[:, :N] = e.torch.from_numpy(np.array(V[:, :N]))
    assert t.data_ptr() % 16 == 0
    return t


def chain_layout(N, form):
    """-> (ld, offset of w) of an alignment form"""
    even = N if N % 2 == 0 else N + 1
    odd = N if N % 2 == 1 else N + 1
    return {"a": (even, 0), "b": (odd, 0), "c": (even, 1), "d": (N + 3, 0)}[form]


def takes_the_16_byte_loop(N, form):
    ld, off = chain_layout(N, form)
    return ld % 2 == 0 and off == 0


def same_bits(what, got, want):
    bad = np.nonzero(~(got == want))[0]                                       # a NaN on either side is a difference
    print(f"{what}: {len(bad)} of {len(got)} elements differ from the restatement")
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), got[bad[:4]].tolist(), want[bad[:4]].tolist())


def same_bits_c(what, got, want):
    same_bits(what + " re", np.ascontiguousarray(got.real), np.ascontiguousarray(want.real))
    same_bits(what + " im", np.ascontiguousarray(got.imag), np.ascontiguousarray(want.imag))


def sum_check(what, got, terms):
    """|got - fsum(terms)| <= n 2^-53 sum |term_i|: the worst case of any order of n - 1 double additions of these terms"""
    exact = math.fsum(terms.tolist())
    bar = len(terms) * U * math.fsum(np.abs(terms).tolist())
    print(f"{what}: |got - fsum| = {abs(got - exact):.2e} (bound {bar:.2e}, |sum| {abs(exact):.2e})")
    assert abs(got - exact) <= bar, (what, got, exact, bar)                   # a NaN fails: the comparison is False


def pair_terms(x, y, paired):
    """the terms a Float64 reduction adds: one per 16-byte pair (x0*y0 + x1*y1) and one per tail element, or one per element"""
    if not paired:
        return x * y
    n2 = len(x) // 2
    return np.concatenate([x[0:2 * n2:2] * y[0:2 * n2:2] + x[1:2 * n2:2] * y[1:2 * n2:2], x[2 * n2:] * y[2 * n2:]])


# ---- inputs of the chains: orthonormal columns, O(1) coefficients ----
@functools.lru_cache(maxsize=2)
def _chain_inputs(N, kmax):
    """V: min(kmax, N) orthonormal columns (rows of the array) from a host QR of a seeded normal matrix; a: |a_k| in [0.5, 2] with
    random signs; r: a unit-norm random vector; noise for the check vector"""
    rng = np.random.default_rng(1000 + N % 9973 + kmax)
    k = min(kmax, N)
    V = np.ascontiguousarray(np.linalg.qr(rng.standard_normal((N, k)))[0].T)
    a = rng.uniform(0.5, 2.0, k) * rng.choice([-1.0, 1.0], k)
    r = rng.standard_normal(N)
    r /= np.linalg.norm(r)
    noise = 1e-3 * rng.standard_normal(N) / math.sqrt(N)
    for x in (V, a, r, noise):
        x.setflags(write=False)
    return V, a, r, noise


def chain_w(N, kmax, ncols):
    V, a, r, noise = _chain_inputs(N, kmax)
    w = a[:ncols] @ V[:ncols] + r                                             # every coefficient O(1): a skipped column costs O(1)
    y = np.arange(1.0, ncols + 1.0) @ V[:ncols] + noise                       # every column its own overlap: a misfiled index shows
    return V, w, y


@functools.lru_cache(maxsize=8)
def _chain_ref(N, kmax, ncols, block):
    """the longdouble chain and the bound, computed once per shape and shared by the alignment forms"""
    V, w, _ = chain_w(N, kmax, ncols)
    ref = (R.bgs_longdouble if block == 8 else R.mgs_longdouble)(w, V, ncols)[0]
    bound = R.chain_bound(w, V, ncols, block)
    top = float(np.abs(ref).max())
    ref_hi = ref.astype(np.float64)
    ref_lo = (ref - ref_hi.astype(R.LD)).astype(np.float64)
    for x in (ref_hi, ref_lo, bound):
        x.setflags(write=False)
    return ref_hi, ref_lo, bound, top


def bounded(what, got, N, kmax, ncols, block):
    """|got - ref| <= chain_bound elementwise, and the bound itself <= 1e-8 max|w_ref| (a condition on the inputs)"""
    ref_hi, ref_lo, bound, top = _chain_ref(N, kmax, ncols, block)
    err = np.abs((got - ref_hi) - ref_lo)                                     # got - ref_hi is exact or rounds far below the bound
    worst = int(np.argmax(np.where(np.isnan(err), np.inf, err) / bound))
    print(f"{what}: max |got - longdouble| = {np.nanmax(err):.2e}, bound there {bound[int(np.nanargmax(err))]:.2e}, largest "
          f"error / bound = {err[worst] / bound[worst]:.2e}; max bound / max|w_ref| = {bound.max() / top:.2e} (cap 1e-8)")
    assert bound.max() <= 1e-8 * top, (what, bound.max(), top)
    bad = np.nonzero(~(err <= bound))[0]
    assert len(bad) == 0, (what, len(bad), bad[:8].tolist(), err[bad[:4]].tolist(), bound[bad[:4]].tolist())
    return float(np.nanmax(err)), float(err[worst] / bound[worst])


# ---- sd_k_gs_chain ----
def run_gs_chain(e, N, kmax, ncols, form, y_mode):
    """one call of sd_k_gs_chain on the inputs of (N, ncols) in one alignment form; y_mode: "mix" (every column its own overlap),
    None (no check vector) or an integer k (y = column k)"""
    V, w, y_mix = chain_w(N, kmax, ncols)
    ld, off = chain_layout(N, form)
    nb = e.shim.b1_gs_blocks(N)
    assert nb == min(GS_BLOCKS, max(1, (N // 2 + BS - 1) // BS))
    nproj, npass = ncols - 1, max(ncols - 2, 0) // 8 + 2
    passes = (nproj + 7) // 8                                                # passes that carry check dots
    y = None if y_mode is None else (y_mix if y_mode == "mix" else V[y_mode].copy())
    dV, dw = columns(e, V[:ncols], N, ld), Vec(e, w, off=off)
    dy = None if y is None else Vec(e, y)
    scratch, alpha, chk = Vec(e, n=(2 + npass) * nb * 8), Vec(e, n=nb * 8), Vec(e, n=8 * npass)
    call(e, "b1_gs_chain", dw.ptr, dV.data_ptr(), ld, ncols, N, None if dy is None else dy.ptr, scratch.ptr, alpha.ptr, chk.ptr)
    e.torch.cuda.synchronize()
    got, sc, al, ck = dw.get(), scratch.get(), alpha.get(), chk.get()
    what = f"gs_chain N={N} ncols={ncols} form={form} y={y_mode}"
    assert e.torch.isnan(dV[:, N:]).all() and np.array_equal(dV[:, :N].cpu().numpy(), V[:ncols])               # V is read only
    # (1) the projection, bit for bit, from the coefficients the device summed (both ping-pong lists survive up to 16 columns)
    if nproj <= 16:
        x = w.copy()
        for blk, c0 in enumerate(range(0, nproj, 8)):
            nc1 = min(8, nproj - c0)
            lst = sc[blk * nb * 8:(blk + 1) * nb * 8]
            assert not np.isnan(lst).any()                                    # all 8 columns of a list are written
            cf = [R.sum_cols(lst, nb, 8, c) for c in range(nc1)]
            x = R.proj(x, cf, V[c0:c0 + nc1])
        same_bits(what, got, x)
        if nproj <= 8:
            assert np.isnan(sc[nb * 8:2 * nb * 8]).all()                       # the second list is not needed: not touched
    # (2) against the chain in longdouble, for every column count
    fig = bounded(what, got, N, kmax, ncols, 8)
    # (3) alpha: the column-0 partials against V[:,ncols-1] . w_new of the kernel's own w_new
    assert not np.isnan(al).any() and not al.reshape(nb, 8)[:, 1:].any()       # columns 1..7 of the list: exact zeros
    sum_check(what + " alpha", R.sum_cols(al, nb, 8, 0), pair_terms(V[ncols - 1], got, takes_the_16_byte_loop(N, form)))
    # (4) the check dots: pass p, column c -> chk[8 p + c]
    if y is None or nproj == 0:
        assert np.isnan(ck).all(), "check dots were written without a check vector (or without a projected column)"
        assert np.isnan(sc[2 * nb * 8:]).all()
    else:
        assert not np.isnan(ck[:8 * passes]).any() and np.isnan(ck[8 * passes:]).all()
        assert not ck[nproj:8 * passes].any()                                 # the columns a ragged pass does not have: exact zeros
        for k in range(nproj):
            sum_check(f"{what} chk[{k}]", float(ck[k]), pair_terms(V[k], y, takes_the_16_byte_loop(N, form)))
        if y_mode == "mix":                                                   # each entry is its own column's overlap, k + 1
            assert np.abs(ck[:nproj] - np.arange(1.0, nproj + 1.0)).max() <= 1e-2
        else:
            want = np.zeros(nproj)
            want[y_mode] = 1.0
            assert np.abs(ck[:nproj] - want).max() <= 1e-9, (y_mode, ck[:nproj].tolist())
    return fig


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", SMALL)
def test_gs_chain_single_blocks_and_tails(e, N, form):
    """sd_k_gs_chain at every column count and alignment form: bit-identical to the restatement up to 16 projected columns, under
    the longdouble bound at all, alpha and every check dot against fsum, the check dots at chk[8 p + c] and nowhere else."""
    for ncols in [c for c in NCOLS if c <= N]:
        run_gs_chain(e, N, 26, ncols, form, "mix")
    for ncols in [c for c in (1, 9, 18) if c <= N]:
        run_gs_chain(e, N, 26, ncols, form, None)
    for ncols, k in [(10, 0), (10, 7), (10, 8), (26, 15), (26, 16), (26, 24)]:
        if ncols <= N:
            run_gs_chain(e, N, 26, ncols, form, k)                            # y = one column: 1 at its own index, 0 elsewhere


@pytest.mark.parametrize("ncols", [9, 17, 26])
@pytest.mark.parametrize("N,form", [(524_801, "a"), (524_801, "b"), (524_802, "a"), (524_802, "c")])
def test_gs_chain_past_1024_blocks(e, N, form, ncols):
    """The 1024-block passes wrap (N / 2 > 262 144 pairs; in the scalar forms every block makes five passes).  On an MI355X, over the
    twelve cells: max |got - longdouble| 2.3e-17 where the bound is 6.4e-12, largest error / bound 6.5e-6, largest bound
    1.09e-9 max|w_ref| (cap 1e-8); ncols <= 17 also bit-identical to the restatement."""
    assert (N // 2 + BS - 1) // BS > GS_BLOCKS
    run_gs_chain(e, N, 26, ncols, form, "mix")
    if ncols == 17 and form == "a":
        run_gs_chain(e, N, 26, ncols, form, None)
        run_gs_chain(e, N, 26, ncols, form, 8)


# ---- sd_k_gs_update (k_gs_update + k_gs_correct) and sd_k_gs_scale ----
def partial_list(rng, nb, total, positive=False):
    """a synthetic [nb][8] partial list: column 0 random with a sum near `total`, NaN in every column the consumer must not read"""
    lst = np.full((nb, 8), NAN)
    col = rng.uniform(0.5, 1.5, nb) if positive else rng.standard_normal(nb) + 0.3
    lst[:, 0] = col * (total / col.sum())
    return lst


@pytest.mark.parametrize("form", ["a", "c", "v"])
@pytest.mark.parametrize("N", SMALL + N_GS_WRAP)
def test_gs_update_and_correction(e, N, form):
    """w = (w - alpha vj) - beta vjm1 with alpha and beta from synthetic partial lists, then the k = j-1 repair w -= d vjm1 with d
    from column 1 of the update's own list (read back): scalars and w bit for bit, d and both |w|^2 lists against fsum.
    form a: aligned; c: w one double past an aligned base; v: vjm1 (or vj without it) one double past."""
    if N in N_GS_WRAP:
        assert (N // 2 + BS - 1) // BS > GS_BLOCKS
    rng = np.random.default_rng(N + ord(form))
    nb = e.shim.b1_gs_blocks(N)
    w, vj, vjm1 = (rng.standard_normal(N) for _ in range(3))
    w, vj, vjm1 = 3.0 * w / np.linalg.norm(w), vj / np.linalg.norm(vj), vjm1 / np.linalg.norm(vjm1)
    alpha_l, n2_l = partial_list(rng, nb, 1.3), partial_list(rng, nb, 0.6, positive=True)
    paired = form == "a"
    for have in (True, False):
        dw = Vec(e, w, off=1 if form == "c" else 0)
        dvj = Vec(e, vj, off=1 if form == "v" and not have else 0)
        dvm = Vec(e, vjm1, off=1 if form == "v" else 0) if have else None
        dal, dn2 = Vec(e, alpha_l.reshape(-1)), Vec(e, n2_l.reshape(-1))
        st, n2_out, upd = Vec(e, n=5), Vec(e, n=nb * 8), Vec(e, n=nb * 8)
        call(e, "b1_gs_update", dw.ptr, dvj.ptr, dvm.ptr if have else None, N, dal.ptr, dn2.ptr if have else None,
             st.ptr + 8, st.ptr + 24, n2_out.ptr, upd.ptr)
        e.torch.cuda.synchronize()
        got, s, out, u = dw.get(), st.get(), n2_out.get().reshape(nb, 8), upd.get().reshape(nb, 8)
        what = f"gs_update N={N} form={form} vjm1={have}"
        a = R.sum_cols(alpha_l, nb, 8, 0)
        assert s[1] == a and np.isnan(s[[0, 2, 4]]).all(), (what, s, a)
        if not have:
            assert np.isnan(s[3]) and np.isnan(u).all()                        # store_beta and the scratch list are not written
            w1 = R.update(w, a, vj)
            same_bits(what, got, w1)
            assert not np.isnan(out[:, :2]).any() and np.isnan(out[:, 2:]).all() and not out[:, 1].any()
            sum_check(what + " |w|^2", R.sum_cols(out, nb, 8, 0), pair_terms(w1, w1, paired))
            continue
        b = math.sqrt(R.sum_cols(n2_l, nb, 8, 0))
        assert s[3] == b, (what, s, b)
        w1 = R.update(w, a, vj, b, vjm1)
        assert not np.isnan(u[:, :2]).any() and np.isnan(u[:, 2:]).all()
        d = R.sum_cols(u, nb, 8, 1)
        sum_check(what + " d = vjm1 . w", d, pair_terms(vjm1, w1, paired))
        sum_check(what + " |w|^2 before the repair", R.sum_cols(u, nb, 8, 0), pair_terms(w1, w1, paired))
        w2 = R.correct(w1, d, vjm1)
        same_bits(what, got, w2)
        assert not np.isnan(out[:, 0]).any() and np.isnan(out[:, 1:]).all()
        sum_check(what + " |w|^2", R.sum_cols(out, nb, 8, 0), pair_terms(w2, w2, paired))
        left = math.fsum((vjm1 * got).tolist()) / math.fsum((vjm1 * vjm1).tolist())
        print(f"{what}: vjm1 component after the repair {left:.2e} (before {d:.2e})")
        assert abs(left) <= 1e-12 * abs(d) + 1e-13                          # roundings of w: 2u |w|_2 = 7e-16


@pytest.mark.parametrize("form", ["a", "c", "v"])
@pytest.mark.parametrize("N", SMALL + [N_SCALE_WRAP])
def test_gs_scale(e, N, form):
    """vnext = w / sqrt(sum of the |w|^2 partials), bit for bit; form a: aligned, c: w one double past, v: vnext one double past"""
    if N == N_SCALE_WRAP:
        assert (N // 2 + BS - 1) // BS > GS_SCALE_BLOCKS
    rng = np.random.default_rng(N + 7 * ord(form))
    nb = e.shim.b1_gs_blocks(N)
    w = rng.standard_normal(N)
    n2_l = partial_list(rng, nb, 0.37, positive=True)
    dw, dv = Vec(e, w, off=1 if form == "c" else 0), Vec(e, n=N, off=1 if form == "v" else 0)
    dn2, st = Vec(e, n2_l.reshape(-1)), Vec(e, n=3)
    call(e, "b1_gs_scale", dv.ptr, dw.ptr, N, dn2.ptr, st.ptr + 8)
    e.torch.cuda.synchronize()
    b = math.sqrt(R.sum_cols(n2_l, nb, 8, 0))
    s = st.get()
    assert s[1] == b and np.isnan(s[[0, 2]]).all()
    same_bits(f"gs_scale N={N} form={form}", dv.get(), R.scale(w, b))
    assert np.array_equal(dw.get(), w)


# ---- sd_k_mgs_chain and sd_k_bgs_chain ----
SLOT = 6


def run_ctx_chain(e, name, N, kmax, ncols, form):
    V, w, _ = chain_w(N, kmax, ncols)
    ld, off = chain_layout(N, form)
    dV = columns(e, V[:ncols], N, ld)
    res = []
    for _ in range(2):
        dw = Vec(e, w, off=off)
        call(e, f"b1_{name}_chain", dw.ptr, dV.data_ptr(), ld, ncols, N, SLOT)
        out = np.full(3, NAN)
        call(e, "b1_read_scalars", SLOT, 1, out.ctypes.data)
        assert np.isnan(out[1:]).all()
        res.append((dw.get(), float(out[0])))
    what = f"{name}_chain N={N} ncols={ncols} form={form}"
    assert np.array_equal(res[0][0], res[1][0]) and res[0][1] == res[1][1], what + ": two calls, different bits"
    got, slot = res[0]
    fig = bounded(what, got, N, kmax, ncols, 8 if name == "bgs" else 1)
    # k_sub_dot takes its 16-byte loop on the alignment of the columns it touches alone (ld does not enter)
    paired = takes_the_16_byte_loop(N, form) if name == "bgs" else (off == 0 and (ld % 2 == 0 or ncols == 1))
    sum_check(what + " slot", slot, pair_terms(V[ncols - 1], got, paired))
    return fig


@pytest.mark.parametrize("name", ["mgs", "bgs"])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", SMALL)
def test_ctx_chains_single_blocks_and_tails(e, N, form, name):
    for ncols in [c for c in NCOLS if c <= N]:
        run_ctx_chain(e, name, N, 26, ncols, form)


@pytest.mark.parametrize("form", ["a", "b"])
@pytest.mark.parametrize("name", ["mgs", "bgs"])
def test_ctx_chains_past_16384_blocks(e, name, form):
    """Their grids count pairs: N / 2 > 16384 * 256.  On an MI355X: max |got - longdouble| 2.8e-18 where the bound is
    1.1e-11, largest error / bound 5.0e-7; the bound is 4.72e-9 (mgs) and 5.56e-9 (bgs) of max|w_ref| (cap 1e-8)."""
    N = N_CHAIN_CAP
    assert (N // 2 + BS - 1) // BS > RED_BLOCKS
    run_ctx_chain(e, name, N, 10, 10, form)


# ---- sd_k_mdot ----
def mdot(e, dV, ld, ncols, dy, N):
    out = np.full(ncols + 2, NAN)
    call(e, "b1_mdot", dV.data_ptr(), ld, ncols, dy.data_ptr(), N, out.ctypes.data)
    assert np.isnan(out[ncols:]).all() and not np.isnan(out[:ncols]).any()
    return out[:ncols]


@pytest.mark.parametrize("pad", [0, 3])
@pytest.mark.parametrize("N", [1, 255, 256, 257, 1000])
def test_mdot_groups_of_16(e, N, pad):
    rng = np.random.default_rng(N + pad)
    V, y = rng.standard_normal((33, N)), rng.standard_normal(N)
    ld = N + pad
    dV, dy = columns(e, V, N, ld), Vec(e, y)
    probe = e.torch.zeros(N, dtype=e.torch.float64, device=e.dev)
    for ncols in (1, 15, 16, 17, 32, 33):
        got = mdot(e, dV, ld, ncols, dy.t, N)
        for c in range(ncols):
            sum_check(f"mdot N={N} ld={ld} ncols={ncols} column {c}", float(got[c]), V[c] * y)
        for i in sorted({0, N // 2, N - 1}):
            probe[i] = 1.0
            g = mdot(e, dV, ld, ncols, probe, N)
            assert np.array_equal(g, V[:ncols, i]), (N, ld, ncols, i)         # y = e_i picks V[c][i], exactly, for every column
            probe[i] = 0.0


def cap_probes(items):
    """item 0, the last item of the first pass, the first of the second, one in the last partial block, the last"""
    assert items > CAP
    last_block = (items - 1) // BS * BS
    assert last_block >= CAP and items - last_block < BS
    return [0, CAP - 1, CAP, last_block + (items - last_block) // 2, items - 1]


def test_mdot_past_16384_blocks(e):
    t, N, ncols = e.torch, N_CAP, 17
    g = t.Generator(device=e.dev).manual_seed(17)
    dV = t.randn((ncols, N), generator=g, dtype=t.float64, device=e.dev)
    dy = t.randn(N, generator=g, dtype=t.float64, device=e.dev)
    got = mdot(e, dV, N, ncols, dy, N)
    y = dy.cpu().numpy()
    for c in (0, 15, 16):                                                     # both groups; fsum of 4.2 M terms is the cost here
        sum_check(f"mdot N={N} column {c}", float(got[c]), dV[c].cpu().numpy() * y)
    # the other columns: against the device's own float64 dot, at the same bar from a norm bound (Cauchy-Schwarz)
    rest = (dV @ dy).cpu().numpy()
    bar = 2 * N * U * float(t.linalg.norm(dV, dim=1).max()) * float(t.linalg.norm(dy))
    assert np.abs(got - rest).max() <= bar, (got.tolist(), rest.tolist(), bar)
    dy.zero_()
    for i in cap_probes(N):
        dy[i] = 1.0
        assert np.array_equal(mdot(e, dV, N, ncols, dy, N), dV[:, i].cpu().numpy()), i
        dy[i] = 0.0


# ---- sd_k_gemv_cols ----
def run_gemv(e, V, coef, N):
    dV, dy = e.torch.from_numpy(V).to(e.dev).contiguous(), Vec(e, n=N)                      # y is NaN: the first group must not read it
    c = np.ascontiguousarray(coef)
    call(e, "b1_gemv_cols", dy.ptr, dV.data_ptr(), N, len(c), c.ctypes.data)
    e.torch.cuda.synchronize()
    same_bits(f"gemv_cols N={N} ncols={len(c)}", dy.get(), R.gemv_cols(V, c))


@pytest.mark.parametrize("ncols", [1, 2, 255, 256, 257, 513])
def test_gemv_cols_groups_of_256(e, ncols):
    rng = np.random.default_rng(ncols)
    run_gemv(e, rng.standard_normal((ncols, 1000)), rng.uniform(0.5, 2.0, ncols) * rng.choice([-1.0, 1.0], ncols), 1000)


def test_gemv_cols_past_16384_blocks(e):
    rng = np.random.default_rng(3)
    assert N_CAP > CAP
    run_gemv(e, rng.standard_normal((3, N_CAP)), np.array([1.25, -0.7, 0.9]), N_CAP)


# ---- sd_k_ccombine ----
def crandn(rng, n):
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def run_ccombine(e, cols, cr, ci, N):
    dcols = [Vec(e, x) for x in cols]
    dy = Vec(e, n=N, cplx=True)                                               # y is NaN: the first group must not read it
    ptrs = (C.c_void_p * max(len(cols), 1))(*[d.ptr for d in dcols])
    cr, ci = np.ascontiguousarray(cr), np.ascontiguousarray(ci)
    call(e, "b1_ccombine", dy.ptr, C.addressof(ptrs), N, len(cols), cr.ctypes.data, ci.ctypes.data)
    e.torch.cuda.synchronize()
    got = dy.get()
    if not cols:
        assert got.tobytes() == np.zeros(N, dtype=np.complex128).tobytes()   # exact zeros, signs included
        return
    same_bits_c(f"ccombine N={N} ncols={len(cols)}", got, R.ccombine(cols, cr, ci))


@pytest.mark.parametrize("ncols", [0, 1, 15, 16, 17, 32, 33])
def test_ccombine_groups_of_16(e, ncols):
    rng = np.random.default_rng(50 + ncols)
    run_ccombine(e, [crandn(rng, 1000) for _ in range(ncols)], rng.standard_normal(ncols), rng.standard_normal(ncols), 1000)


def test_ccombine_past_16384_blocks(e):
    rng = np.random.default_rng(4)
    assert N_CAP > CAP
    run_ccombine(e, [crandn(rng, N_CAP) for _ in range(2)], np.array([0.8, -1.1]), np.array([-0.3, 0.45]), N_CAP)


# ---- the elementwise launchers ----
def cap_asserted(items):
    if items > 2000:
        assert items > CAP
    return items


@pytest.mark.parametrize("N,off", [(1026, 0), (1025, 0), (1025, 1), (N_CAP, 0), (N_CAP - 1, 1)])
def test_cheb_init_and_promote(e, N, off):
    """ComplexF64 elements: even and odd counts, and vectors one ELEMENT (16 bytes, the type's alignment) past an aligned base;
    the Float64 input of k_promote also one double past it."""
    cap_asserted(N)
    rng = np.random.default_rng(N + off)
    x0, x1 = crandn(rng, N), crandn(rng, N)
    c0, c1 = 0.3 - 0.2j, -0.11 + 0.23j
    d0, d1 = Vec(e, x0, off=off), Vec(e, x1, off=off)
    for have1 in (0, 1):
        dy = Vec(e, n=N, off=off, cplx=True)
        call(e, "b1_cheb_init", dy.ptr, d0.ptr, d1.ptr if have1 else None, N, c0.real, c0.imag, c1.real, c1.imag, have1)
        e.torch.cuda.synchronize()
        same_bits_c(f"cheb_init N={N} off={off} have1={have1}", dy.get(), R.cheb_init(x0, x1, c0, c1, have1))
    xr = rng.standard_normal(2 * N)
    for nc in (1, 2):
        dx, dy = Vec(e, xr[:nc * N], off=off), Vec(e, n=N, off=off, cplx=True)
        call(e, "b1_promote", dy.ptr, dx.ptr, nc, N)
        e.torch.cuda.synchronize()
        got, want = dy.get(), R.promote(xr[:nc * N], nc)
        assert got.tobytes() == want.tobytes(), f"promote N={N} off={off} nc={nc}"


@pytest.mark.parametrize("n,off", [(1026, 0), (1025, 0), (1026, 1), (2 * N_CAP, 0), (N_CAP, 0), (N_CAP + 1, 1)])
def test_sub2_and_scale_div(e, n, off):
    """Float64: aligned even n (16-byte kernel, n / 2 items), odd n and a base one double past alignment (scalar kernel, n items)"""
    cap_asserted(n // 2 if (n % 2 == 0 and off == 0) else n)
    rng = np.random.default_rng(n + off)
    w, v, u = rng.standard_normal(n), rng.standard_normal(n), rng.standard_normal(n)
    a, b = 1.7, -0.31
    dv, du = Vec(e, v), Vec(e, u)
    for have_u in (True, False):
        dw = Vec(e, w, off=off)
        call(e, "b1_sub2", dw.ptr, dv.ptr, du.ptr if have_u else None, n, a, b)
        e.torch.cuda.synchronize()
        same_bits(f"sub2 n={n} off={off} u={have_u}", dw.get(), R.update(w, a, v, b, u) if have_u else R.update(w, a, v))
    dw, dy = Vec(e, w, off=off), Vec(e, n=n)
    call(e, "b1_scale_div", dy.ptr, dw.ptr, n, b)                              # out of place
    call(e, "b1_scale_div", dw.ptr, dw.ptr, n, b)                              # in place
    e.torch.cuda.synchronize()
    same_bits(f"scale_div n={n} off={off} out of place", dy.get(), R.scale(w, b))
    same_bits(f"scale_div n={n} off={off} in place", dw.get(), R.scale(w, b))
    assert np.array_equal(dv.get(), v) and np.array_equal(du.get(), u)


# ---- reductions into a slot or to a device address ----
def read_slot(e, slot):
    out = np.full(4, NAN)
    call(e, "b1_read_scalars", slot, 2, out.ctypes.data)
    assert np.isnan(out[2:]).all()
    return float(out[0]), float(out[1])


def test_imag_count_on_both_sides_of_the_wrap(e):
    N = N_CAP
    x = e.torch.ones(N, dtype=e.torch.complex128, device=e.dev)                # real parts non-zero, imaginary parts zero
    call(e, "b1_imag_count", x.data_ptr(), N, 2)
    assert read_slot(e, 2) == (0.0, 0.0)
    rows = cap_probes(N) + list(range(1000, 1100)) + list(range(CAP + 7, CAP + 50))
    x[e.torch.tensor(rows, device=e.dev)] = complex(0.0, -1e-300)             # any non-zero imaginary part counts, however small
    call(e, "b1_imag_count", x.data_ptr(), N, 2)
    assert read_slot(e, 2) == (float(len(set(rows))), 0.0)
    small = e.torch.zeros(1025, dtype=e.torch.complex128, device=e.dev)
    small[1024] = 1j
    call(e, "b1_imag_count", small.data_ptr(), 1025, 2)
    assert read_slot(e, 2) == (1.0, 0.0)


@pytest.mark.parametrize("N", [1025, N_CAP])
def test_complex_dots(e, N):
    """sd_k_dotu (no conjugation, into a slot) and sd_k_dot_to with nc = 2 (conj(x) y, to a device address in a NaN buffer)"""
    cap_asserted(N)
    rng = np.random.default_rng(N)
    x, y = crandn(rng, N), crandn(rng, N)
    dx, dy = Vec(e, x), Vec(e, y)
    xr, xi, yr, yi = x.real, x.imag, y.real, y.imag
    call(e, "b1_dotu", dx.ptr, dy.ptr, N, 4)
    re, im = read_slot(e, 4)
    sum_check(f"dotu N={N} re", re, xr * yr - xi * yi)
    sum_check(f"dotu N={N} im", im, xr * yi + xi * yr)
    dst = Vec(e, n=8)
    call(e, "b1_dot_to", 2, dx.ptr, dy.ptr, N, dst.ptr + 3 * 8)
    e.torch.cuda.synchronize()
    d = dst.get()
    assert np.isnan(d[[0, 1, 2, 5, 6, 7]]).all()                              # the neighbours stay NaN
    sum_check(f"dot_to c128 N={N} re", float(d[3]), xr * yr + xi * yi)
    sum_check(f"dot_to c128 N={N} im", float(d[4]), xr * yi - xi * yr)


@pytest.mark.parametrize("n,off", [(1025, 0), (1026, 1), (2 * N_CAP + 1, 0), (N_CAP + 1, 1)])
def test_real_dot_and_norm_to_a_device_address(e, n, off):
    """sd_k_dot_to with nc = 1 and sd_k_nrm2sq_to: pairs and a tail element when aligned, element by element one double past"""
    paired = off == 0
    cap_asserted(n // 2 if paired else n)
    rng = np.random.default_rng(n + off)
    x, y = rng.standard_normal(n), rng.standard_normal(n)
    dx, dy, dst = Vec(e, x, off=off), Vec(e, y, off=off), Vec(e, n=8)
    call(e, "b1_dot_to", 1, dx.ptr, dy.ptr, n, dst.ptr + 2 * 8)
    call(e, "b1_nrm2sq_to", dx.ptr, n, dst.ptr + 5 * 8)
    e.torch.cuda.synchronize()
    d = dst.get()
    assert np.isnan(d[[0, 1, 4, 7]]).all() and d[3] == 0.0 and d[6] == 0.0     # (sum, 0) pairs; the neighbours stay NaN
    sum_check(f"dot_to f64 n={n} off={off}", float(d[2]), pair_terms(x, y, paired))
    sum_check(f"nrm2sq_to n={n} off={off}", float(d[5]), pair_terms(x, x, paired))
