"""The Lanczos fold family of csrc/kernels_blas1.hip one launcher at a time, through tests/blas1_shim.cpp: sd_k_lanczos_fold (the
streaming form), sd_k_lanczos_fold_p (the launch-bound, batched form), sd_k_lanczos_fold_scalars_p and sd_k_lanczos_fold_scalars --
twelve update kernels (form 0 / 1 / 2, with and without u_prev) and the two that file the last step's scalars.  The recursion tests
see them only through whole recursions under a tolerance, where forms 0 and 1 (which differ in rounding order alone), a lane of the
paired loop that read the wrong array once, or a list summed in another order change nothing that is looked at.

Yardsticks (tests/fold_ref.py, proven on the CPU by tests/test_fold_ref_host.py):
  bit for bit   t against fold_elem fed the alpha read back from store_alpha and the device's own square roots; the stored alpha
                against dot / nc (a true division), for the launch-bound form with dot and nc summed in the block's order
                (sum_list256); the |w|^2 partials of sd_k_lanczos_fold_p against fold_p_partials; the two scalar kernels against
                what the update kernels stored from the same inputs
  fsum          n2_out[0] of the streaming form against math.fsum of the restatement's own terms, bar N 2^-53 sum |term| (any
                order of N - 1 additions: a condition, not a measurement); n2_out[1] is exactly 0.0
  sqrt          no restatement takes a square root: b_c and b_p are the device's own, from store_bc of sd_k_lanczos_fold_scalars
                (one thread through the same fold_resolve).  Separately every stored b_c is compared with np.sqrt of the same
                double: at most 1 ulp apart, the exact ones counted.
Every output, list tail, gap between the vectors of a batch and guard is NaN before the call; uc and up must come back unchanged.

Shapes.  Streaming form (stride = nb 256, nb = min(ceil(N / 256), 16384), CAP = 16384 * 256): N in {1, 2, 3, 255, 256, 257, 1025}
is the tail branch alone with up to 5 blocks; CAP + 1 is the smallest N at which a lane (lane 0) enters the paired loop; 2 CAP the
smallest at which every lane pairs and none has a tail; 2 CAP + 1 the smallest with a pair and then a tail in one lane; 3 CAP + 3
the smallest with a second paired trip (lanes 0-2) next to pair + tail (all others).  Launch-bound form: N in {1, 2, 3, 255, 256,
257, 2047, 2048, 2049, 4097} with nb = sd_k_lanczos_fold_blocks(N) (1 to 3 blocks) and with nb = 1 (the grid-stride loop wraps up to
17 times), N = 524 293 with the cap of 256 blocks (eight trips and a ragged ninth); lists of 1, 63, 64, 65 (one wave and its edge),
255, 256, 257 (one entry per thread and the second trip), 1000 and 4096 dot pairs and 1, 2, 255, 256, 257 |w|^2 pairs; batches of 1
and 3 with bstride in {N, N + 3} and store_stride in {2, 7}.  Scalars in two regimes (fold_ref.norms): |u|^2 = O(N), the squared
norms of the normal vectors they go with, everywhere; and O(1), where alpha, beta and the three terms of the update are of one
size, at every size up to CAP + 1 (streaming) and 524 293 (launch-bound).

Figures on an MI355X.  72 cells; 1769 vector comparisons bit for bit over 408 804 614 components, 0 differ; every stored alpha, b_c
and |w|^2 partial equal to its restatement.  fsum checks (122): largest error / bar 0.46 at N = 3, where the bar is 3.9e-15 (two
ulp of the sum); 7.5e-3 at N = 257; at the cap sizes at most 3.6e-7 (3.7e-9 against 1.1e-2).  Square roots: 3429, all equal to
np.sqrt of the same double, none 1 ulp off.  Run time: 23 s in all; per group 0.1 s (tail branch), 4.7 s (CAP + 1, six cells of two
regimes), 7.2 s (3 CAP + 3, six cells, 1.0 - 1.7 s each: host arithmetic on 12.6 M elements and one fsum), 3.8 s (2 CAP, 2 CAP + 1),
3.3 s (null scalars), 0.7 s (launch-bound sizes and layouts, 704 calls), 0.3 s (256 blocks), 0.3 s (producer and consumer), 0.1 s
or less (all others)."""
import functools
import gc
import math
import time
from types import SimpleNamespace

import numpy as np
import pytest

import blas1_ref as R
import fold_ref as F
from test_gpu_blas1_kernels import NAN, U, Vec, call, same_bits

pytestmark = pytest.mark.gpu

BS, RED_BLOCKS = 256, 16384                                                  # caps of csrc/kernels_blas1.hip
CAP = RED_BLOCKS * BS
SMALL = [1, 2, 3, 255, 256, 257, 1025]
SMALL_P = [1, 2, 3, 255, 256, 257, 2047, 2048, 2049, 4097]
N_P_CAP = 524_293
NDOT = [1, 63, 64, 65, 255, 256, 257, 1000, 4096]
NN2 = [1, 2, 255, 256, 257]
VARIANTS = [(form, have_u) for form in (0, 1, 2) for have_u in (False, True)]
TWO = [(1, True), (2, False)]
DOT = F.DOT
TALLY = SimpleNamespace(vectors=0, elements=0, fsum=0, fsum_worst=0.0, sqrt=0, sqrt_exact=0, seconds={})


@pytest.fixture(scope="module")
def e(pkg, tmp_path_factory):
    import torch
    shim = R.build_shim(pkg, tmp_path_factory.mktemp("fold_shim"))
    ctx = pkg.default_context()
    yield SimpleNamespace(pkg=pkg, shim=shim, ctx=ctx, torch=torch, dev=torch.device("cuda", ctx.device))
    _vectors.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()
    print(f"\nfold kernels: {TALLY.vectors} vector comparisons bit for bit over {TALLY.elements} components; {TALLY.fsum} fsum checks, "
          f"largest error / bar {TALLY.fsum_worst:.2e}; {TALLY.sqrt} square roots, {TALLY.sqrt_exact} equal to np.sqrt, the others "
          f"1 ulp off; seconds per group: " + ", ".join(f"{k} {v:.1f}" for k, v in TALLY.seconds.items()))


@pytest.fixture(autouse=True)
def _timed(request):
    t0 = time.perf_counter()
    yield
    name = request.function.__name__
    TALLY.seconds[name] = TALLY.seconds.get(name, 0.0) + time.perf_counter() - t0


@functools.lru_cache(maxsize=4)
def _vectors(N, seed):
    return F.vectors(N, seed)


def bits_c(what, got, want):
    """complex vectors, bit for bit in both components (a NaN on either side is a difference)"""
    same_bits(what + " re", np.ascontiguousarray(got.real), np.ascontiguousarray(want.real))
    same_bits(what + " im", np.ascontiguousarray(got.imag), np.ascontiguousarray(want.imag))
    TALLY.vectors += 1
    TALLY.elements += 2 * len(got)


def same_layout(what, got, want):
    """small arrays of scalars: the same bits where a value is due and NaN everywhere else"""
    assert np.array_equal(got, want, equal_nan=True), (what, got.tolist(), want.tolist())


def sqrt_check(x, got):
    """the device's square roots against np.sqrt of the same doubles: at most 1 ulp apart"""
    x, got = np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(got, dtype=np.float64))
    ref = np.sqrt(x)
    dist = np.abs(got.view(np.int64) - ref.view(np.int64))                    # positive finite doubles: the distance in ulps
    TALLY.sqrt += len(x)
    TALLY.sqrt_exact += int((dist == 0).sum())
    print(f"sqrt: {int((dist == 0).sum())} of {len(x)} equal to np.sqrt, largest distance {int(dist.max())} ulp")
    assert np.isfinite(got).all() and (got >= 0).all() and (dist <= 1).all(), (x.tolist(), got.tolist(), ref.tolist())


def dev_sqrt(e, values):
    """the device's own sqrt of every value: store_bc of sd_k_lanczos_fold_scalars, one launch per value"""
    values = np.asarray(values, dtype=np.float64)
    src, dot, sa, out = Vec(e, values), Vec(e, np.array(DOT)), Vec(e, n=2), Vec(e, n=len(values))
    for k in range(len(values)):
        call(e, "b1_lanczos_fold_scalars", 0, dot.ptr, src.ptr + 8 * k, sa.ptr, out.ptr + 8 * k)
    e.torch.cuda.synchronize()
    got = out.get()
    sqrt_check(values, got)
    return got


def norm_check(what, got, terms):
    """|got - fsum(terms)| <= N 2^-53 sum |term|: the worst case of any order of N - 1 double additions (the terms are >= 0)"""
    assert (terms >= 0).all()
    exact = math.fsum(terms.tolist())
    bar = len(terms) * U * exact
    err = abs(got - exact)
    TALLY.fsum += 1
    TALLY.fsum_worst = max(TALLY.fsum_worst, err / bar if bar > 0 else 0.0)
    print(f"{what}: |got - fsum| = {err:.2e} (bar {bar:.2e}, |sum| {exact:.2e})")
    assert err <= bar, (what, got, exact, bar)                                # a NaN fails: the comparison is False


# ---- sd_k_lanczos_fold ----
def run_fold(e, N, form, have_u, c_null=False, p_null=False, balanced=False):
    """one call of sd_k_lanczos_fold (and one of sd_k_lanczos_fold_scalars on the same scalars) against the restatement"""
    t, uc, up = _vectors(N, 1)
    n2c, n2p = F.norms(N, balanced)
    dT, dC, dP = Vec(e, t), Vec(e, uc), Vec(e, up) if have_u else None
    dot, dn2c, dn2p = Vec(e, np.array(DOT)), Vec(e, np.array([n2c])), Vec(e, np.array([n2p]))
    sa, sb, n2o, sa2, sb2 = Vec(e, n=2), Vec(e, n=1), Vec(e, n=2), Vec(e, n=2), Vec(e, n=1)
    pc, pp = None if c_null else dn2c.ptr, None if p_null else dn2p.ptr
    call(e, "b1_lanczos_fold", dT.ptr, dC.ptr, dP.ptr if have_u else None, N, form, dot.ptr, pc, pp, sa.ptr, sb.ptr, n2o.ptr)
    call(e, "b1_lanczos_fold_scalars", form, dot.ptr, pc, sa2.ptr, sb2.ptr)
    e.torch.cuda.synchronize()
    what = f"fold N={N} form={form} u={have_u} n2c={'null' if c_null else 'set'} n2p={'null' if p_null else 'set'} balanced={balanced}"
    got, al, bc, n2 = dT.get(), sa.get(), sb.get(), n2o.get()
    assert np.array_equal(dC.get(), uc) and (not have_u or np.array_equal(dP.get(), up)), "uc or up was written"
    for v, x in ((dot, DOT), (dn2c, [n2c]), (dn2p, [n2p])):
        assert np.array_equal(v.get(), np.array(x)), "an input scalar was written"
    # alpha: a true division, the imaginary part in form 2 alone; b_c only where there is an n2c
    ar, ai = F.alpha(form, DOT, None if c_null else n2c)
    same_layout(what + " alpha", al, np.array([ar, ai if form == 2 else NAN]))
    assert np.isnan(bc[0]) if c_null else bc[0] > 0
    if not c_null:
        sqrt_check(n2c, bc[0])
    same_layout(what + " fold_scalars alpha", sa2.get(), al)                  # sd_k_lanczos_fold_scalars: the same bits
    same_layout(what + " fold_scalars b_c", sb2.get(), bc)
    bp = 1.0 if p_null or not have_u else float(dev_sqrt(e, [n2p])[0])
    want = F.fold_elem(form, t, uc, up if have_u else None, al[0], al[1] if form == 2 else 0.0, 1.0 if c_null else bc[0], bp)
    bits_c(what, got, want)
    norm_check(what + " n2_out[0]", float(n2[0]), F.norm_terms(want))
    assert n2[1] == 0.0 and not np.signbit(n2[1])                             # the launcher's comment: n2_out[1] = 0


@pytest.mark.parametrize("N", SMALL)
def test_fold_tail_branch_alone(e, N):
    """all six kernels below the cap, where the paired loop is not entered: single elements, one block and its edges, five blocks"""
    for form, have_u in VARIANTS:
        for balanced in (False, True):
            run_fold(e, N, form, have_u, balanced=balanced)


@pytest.mark.parametrize("form,have_u", VARIANTS)
def test_fold_one_lane_pairs(e, form, have_u):
    """N = CAP + 1: lane 0 makes one paired trip (elements 0 and CAP), every other lane takes the tail alone"""
    for balanced in (False, True):
        run_fold(e, CAP + 1, form, have_u, balanced=balanced)


@pytest.mark.parametrize("form,have_u", VARIANTS)
def test_fold_second_paired_trip(e, form, have_u):
    """N = 3 CAP + 3: lanes 0-2 make two paired trips and no tail, all others a pair and then the tail"""
    run_fold(e, 3 * CAP + 3, form, have_u)


@pytest.mark.parametrize("form,have_u", TWO)
@pytest.mark.parametrize("N", [2 * CAP, 2 * CAP + 1])
def test_fold_exact_boundaries_of_the_paired_loop(e, N, form, have_u):
    """N = 2 CAP: every lane one pair and no tail; 2 CAP + 1: lane 0 a pair and then a tail, all others the pair alone"""
    run_fold(e, N, form, have_u)


@pytest.mark.parametrize("c_null,p_null", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("N", [257, CAP + 1])
def test_fold_null_scalars_stand_for_a_normalised_vector(e, N, c_null, p_null):
    """a null n2c: nc = b_c = 1.0 and store_bc is left alone; a null n2p: b_p = 1.0"""
    run_fold(e, N, 1, True, c_null, p_null)
    run_fold(e, N, 2, not c_null, c_null, p_null)


# ---- sd_k_lanczos_fold_p, sd_k_lanczos_fold_scalars_p ----
def batch_vec(e, vecs, N, bstride):
    """the vectors of a batch `bstride` elements apart in one device buffer, NaN in the gaps"""
    h = np.full((len(vecs) - 1) * bstride + N, complex(NAN, NAN))
    for q, v in enumerate(vecs):
        h[q * bstride:q * bstride + N] = v
    return Vec(e, h)


def batch_get(dv, batch, N, bstride):
    """-> the vectors of a batch on the host; gaps and guards must still be NaN"""
    h = dv.get()
    gaps = np.ones(len(h), dtype=bool)
    for q in range(batch):
        gaps[q * bstride:q * bstride + N] = False
    assert np.isnan(h[gaps]).all(), "a gap between the vectors of a batch was written"
    return [h[q * bstride:q * bstride + N] for q in range(batch)]


def lists_for(N, batch, ndot, nn2, zero_c=(), balanced=False):
    """distinct lists per vector: dot pairs (both components finite and non-zero), |u_cur|^2 and |u_prev|^2 pairs (p, 0.0)"""
    dotp = np.concatenate([F.dot_list(ndot, q) for q in range(batch)])
    n2c, n2p = F.norms(N, balanced)
    n2cp = np.concatenate([F.n2_list(nn2, q, 0.0 if q in zero_c else n2c) for q in range(batch)])
    n2pp = np.concatenate([F.n2_list(nn2, 3 + q, n2p) for q in range(batch)])
    return dotp, n2cp, n2pp


def restate_fold_p(e, vecs, N, nb, form, have_u, ndot, nn2, dotp, n2cp, n2pp):
    """-> per vector (alpha_re, alpha_im, nc, b_c, b_p, w, partials) from the restatement; n2cp / n2pp None: null"""
    batch = len(vecs)
    d = [(F.sum_list256(dotp[2 * ndot * q:], ndot, 0), F.sum_list256(dotp[2 * ndot * q:], ndot, 1)) for q in range(batch)]
    nc = [None if n2cp is None else F.sum_list256(n2cp[2 * nn2 * q:], nn2, 0) for q in range(batch)]
    npv = [None if n2pp is None else F.sum_list256(n2pp[2 * nn2 * q:], nn2, 0) for q in range(batch)]
    roots = dev_sqrt(e, [x for x in nc + npv if x is not None]).tolist() if n2cp is not None or n2pp is not None else []
    bc = [1.0 if x is None else roots.pop(0) for x in nc]
    bp = [1.0 if x is None else roots.pop(0) for x in npv]
    out = []
    for q, (t, uc, up) in enumerate(vecs):
        ar, ai = F.alpha(form, d[q], nc[q])
        w = F.fold_elem(form, t, uc, up if have_u else None, ar, ai, bc[q], bp[q])
        out.append(SimpleNamespace(ar=ar, ai=ai, nc=nc[q], bc=bc[q], bp=bp[q], w=w, partials=F.fold_p_partials(w, N, nb)))
    return out


def run_fold_p(e, N, nb, form, have_u, batch, bstride, sstride, ndot, nn2, c_null=False, p_null=False, zero_c=(), balanced=False):
    """one call of sd_k_lanczos_fold_p (and one of sd_k_lanczos_fold_scalars_p on the same lists) against the restatement;
    -> (restatement per vector, the outputs as they came back)"""
    vecs = [_vectors(N, 10 + q) for q in range(batch)]
    dotp, n2cp, n2pp = lists_for(N, batch, ndot, nn2, zero_c, balanced)
    dT, dC = batch_vec(e, [v[0] for v in vecs], N, bstride), batch_vec(e, [v[1] for v in vecs], N, bstride)
    dP = batch_vec(e, [v[2] for v in vecs], N, bstride) if have_u else None
    ddot, dc, dp = Vec(e, dotp), Vec(e, n2cp), Vec(e, n2pp)
    nsa = (batch - 1) * sstride + 2
    sa, sb, sa2, sb2, n2o = Vec(e, n=nsa), Vec(e, n=nsa), Vec(e, n=nsa), Vec(e, n=nsa), Vec(e, n=2 * nb * batch + 6)
    pc, pp = None if c_null else dc.ptr, None if p_null else dp.ptr
    call(e, "b1_lanczos_fold_p", dT.ptr, dC.ptr, dP.ptr if have_u else None, N, batch, bstride, form, ddot.ptr, ndot, pc, pp, nn2,
         sa.ptr, sb.ptr, sstride, n2o.ptr, nb)
    call(e, "b1_lanczos_fold_scalars_p", batch, form, ddot.ptr, ndot, pc, nn2, sa2.ptr, sb2.ptr, sstride)
    e.torch.cuda.synchronize()
    what = (f"fold_p N={N} nb={nb} form={form} u={have_u} batch={batch} bstride={bstride} store_stride={sstride} ndot={ndot} nn2={nn2}"
            f" n2c={'null' if c_null else 'set'} n2p={'null' if p_null else 'set'} balanced={balanced}")
    got, al, bc, n2 = batch_get(dT, batch, N, bstride), sa.get(), sb.get(), n2o.get()
    for dv, k in ((dC, 1), (dP, 2)):
        if dv is not None:
            assert all(np.array_equal(g, v[k]) for g, v in zip(batch_get(dv, batch, N, bstride), vecs)), "uc or up was written"
    for v, x in ((ddot, dotp), (dc, n2cp), (dp, n2pp)):
        assert np.array_equal(v.get(), x), "an input list was written"
    ref = restate_fold_p(e, vecs, N, nb, form, have_u, ndot, nn2, dotp, None if c_null else n2cp, None if p_null else n2pp)
    want_al, want_bc, want_n2 = np.full(nsa, NAN), np.full(nsa, NAN), np.full(2 * nb * batch + 6, NAN)
    for q, r in enumerate(ref):
        want_al[q * sstride] = r.ar
        if form == 2:
            want_al[q * sstride + 1] = r.ai
        if not c_null:
            want_bc[q * sstride] = r.bc
        want_n2[2 * nb * q:2 * nb * (q + 1):2] = r.partials                   # nb pairs per vector at 2 (nb q + b) ...
        want_n2[2 * nb * q + 1:2 * nb * (q + 1):2] = 0.0                       # ... second components exactly 0.0, NaN behind them
    if not zero_c:
        same_layout(what + " alpha", al, want_al)
        same_layout(what + " b_c", bc, want_bc)
        same_layout(what + " n2out", n2, want_n2)
        for q, r in enumerate(ref):
            bits_c(f"{what} q={q}", got[q], r.w)
    same_layout(what + " fold_scalars_p alpha", sa2.get(), al)                # sd_k_lanczos_fold_scalars_p: the same bits
    same_layout(what + " fold_scalars_p b_c", sb2.get(), bc)
    return ref, SimpleNamespace(t=got, alpha=al, bc=bc, n2=n2, sstride=sstride)


LAYOUTS = [(1, 0, 2), (1, 3, 7), (3, 0, 7), (3, 3, 2)]                        # batch, bstride - N, store_stride


@pytest.mark.parametrize("one_block", [False, True])
@pytest.mark.parametrize("N", SMALL_P)
def test_fold_p_sizes_layouts_and_list_lengths(e, N, one_block):
    """every size with the launcher's own block count and with one block (the grid-stride loop wraps), in every layout of a batch;
    all six kernels up to N = 257, two above; the list lengths rotate through all of theirs"""
    nb = 1 if one_block else e.shim.b1_lanczos_fold_blocks(N)
    assert one_block or nb == min(256, max(1, -(-N // 2048)))
    k = SMALL_P.index(N) + 3 * one_block
    for form, have_u in (VARIANTS if N <= 257 else TWO):
        for batch, gap, sstride in LAYOUTS:
            for balanced in (False, True):
                run_fold_p(e, N, nb, form, have_u, batch, N + gap, sstride, NDOT[k % len(NDOT)], NN2[k % len(NN2)], balanced=balanced)
            k += 1


@pytest.mark.parametrize("ndot", NDOT)
def test_fold_p_every_list_length(e, ndot):
    """every pair of list lengths, a batch of 3, complex alpha (both components of the dot lists are summed)"""
    for nn2 in NN2:
        run_fold_p(e, 257, 2, 2, True, 3, 260, 7, ndot, nn2)
    run_fold_p(e, 257, 2, 0, True, 3, 257, 2, ndot, NN2[NDOT.index(ndot) % len(NN2)])


@pytest.mark.parametrize("form,have_u", TWO)
def test_fold_p_at_the_cap_of_256_blocks(e, form, have_u):
    """N = 524 293: sd_k_lanczos_fold_blocks is at its cap, every thread makes eight trips and five threads a ninth"""
    assert e.shim.b1_lanczos_fold_blocks(N_P_CAP) == 256 and -(-N_P_CAP // (256 * BS)) == 9 and N_P_CAP % (256 * BS) == 5
    run_fold_p(e, N_P_CAP, 256, form, have_u, 3, N_P_CAP + 3, 7, 4096, 256)
    run_fold_p(e, N_P_CAP, 256, form, have_u, 1, N_P_CAP, 2, 1000, 257, balanced=True)


@pytest.mark.parametrize("c_null,p_null", [(False, True), (True, False), (True, True)])
def test_fold_p_null_lists_stand_for_normalised_vectors(e, c_null, p_null):
    """a null n2cp: nc = b_c = 1.0 for every vector and no store_bc slot is written; a null n2pp: b_p = 1.0 (the first two steps)"""
    for form, have_u in ((0, True), (2, not c_null)):
        run_fold_p(e, 257, 2, form, have_u, 3, 260, 7, 65, 255, c_null, p_null)
        run_fold_p(e, 2049, 1, form, have_u, 1, 2049, 2, 257, 2, c_null, p_null)


@pytest.mark.parametrize("N", [4097, N_P_CAP])
@pytest.mark.parametrize("form", [0, 2])
def test_fold_p_producer_meets_consumer(e, N, form):
    """two consecutive steps of a batch of 3 with the buffers rotated as lanczos_fused rotates them: the |w|^2 partials the first
    step wrote are the n2cp list of the second (nn2 = nb), its n2cp list the second's n2pp.  The second step is bit for bit the
    restatement fed with the FIRST STEP'S RESTATED partials."""
    batch, bstride, sstride, ndot = 3, N + 3, 7, 1000
    nb = e.shim.b1_lanczos_fold_blocks(N)
    vecs = [_vectors(N, 10 + q) for q in range(batch)]
    dotp1, n2cp, n2pp = lists_for(N, batch, ndot, nb)
    dotp2 = np.concatenate([F.dot_list(ndot, 7 + q) for q in range(batch)])
    bufs = [batch_vec(e, [v[k] for v in vecs], N, bstride) for k in range(3)]
    t, ucur, uprev = bufs
    d1, d2, dc, dp = Vec(e, dotp1), Vec(e, dotp2), Vec(e, n2cp), Vec(e, n2pp)
    nsa = (batch - 1) * sstride + 2
    sa1, sb1, sa2, sb2 = (Vec(e, n=nsa) for _ in range(4))
    n2a, n2b = Vec(e, n=2 * nb * batch), Vec(e, n=2 * nb * batch)
    call(e, "b1_lanczos_fold_p", t.ptr, ucur.ptr, uprev.ptr, N, batch, bstride, form, d1.ptr, ndot, dc.ptr, dp.ptr, nb, sa1.ptr, sb1.ptr,
         sstride, n2a.ptr, nb)
    t, ucur, uprev = uprev, t, ucur                                           # { old = uprev; uprev = ucur; ucur = t; t = old; }
    call(e, "b1_lanczos_fold_p", t.ptr, ucur.ptr, uprev.ptr, N, batch, bstride, form, d2.ptr, ndot, n2a.ptr, dc.ptr, nb, sa2.ptr, sb2.ptr,
         sstride, n2b.ptr, nb)
    e.torch.cuda.synchronize()
    step1 = restate_fold_p(e, vecs, N, nb, form, True, ndot, nb, dotp1, n2cp, n2pp)
    list1 = np.zeros(2 * nb * batch)
    list1[0::2] = np.concatenate([r.partials for r in step1])
    same_layout("the first step's n2out", n2a.get(), list1)
    vecs2 = [(v[2], r.w, v[1]) for v, r in zip(vecs, step1)]                   # t = the old u_prev, u_cur = w of step 1, u_prev = the old u_cur
    step2 = restate_fold_p(e, vecs2, N, nb, form, True, ndot, nb, dotp2, list1, n2cp)
    want_al, want_bc, list2 = np.full(nsa, NAN), np.full(nsa, NAN), np.zeros(2 * nb * batch)
    for q, r in enumerate(step2):
        want_al[q * sstride:q * sstride + (2 if form == 2 else 1)] = [r.ar, r.ai][:2 if form == 2 else 1]
        want_bc[q * sstride] = r.bc
        assert r.bp == step1[q].bc                                            # the same list, summed and rooted twice
    list2[0::2] = np.concatenate([r.partials for r in step2])
    same_layout("the second step's alpha", sa2.get(), want_al)
    same_layout("the second step's b_c", sb2.get(), want_bc)
    same_layout("the second step's n2out", n2b.get(), list2)
    for q, (g, g1, g0) in enumerate(zip(batch_get(t, batch, N, bstride), batch_get(ucur, batch, N, bstride),
                                        batch_get(uprev, batch, N, bstride))):
        bits_c(f"producer/consumer N={N} form={form} step 2 q={q}", g, step2[q].w)
        bits_c(f"producer/consumer N={N} form={form} step 1 q={q}", g1, step1[q].w)
        assert np.array_equal(g0, vecs[q][1])


@pytest.mark.parametrize("form,have_u", [(1, True), (2, True), (0, False)])
def test_fold_p_a_broken_column_stays_in_its_own_slots(e, form, have_u):
    """a batch of 3 whose middle vector has an n2cp list summing to 0.0 (a recursion that broke down: nc = b_c = 0, alpha = dot / 0):
    vectors 0 and 2 give the bits of the same call with a healthy middle vector, in t, n2out, alpha and b_c; the middle vector's
    t, partials and alpha are non-finite, its b_c is the 0.0 the recursion reads as the breakdown, and nothing else is touched"""
    N, nb, batch, bstride, sstride = 2049, 2, 3, 2052, 7
    ref, good = run_fold_p(e, N, nb, form, have_u, batch, bstride, sstride, 257, 256)
    _, bad = run_fold_p(e, N, nb, form, have_u, batch, bstride, sstride, 257, 256, zero_c=(1,))
    for q in (0, 2):
        bits_c(f"broken column form={form} u={have_u}: vector {q}", bad.t[q], good.t[q])
        bits_c(f"broken column form={form} u={have_u}: vector {q} against the restatement", bad.t[q], ref[q].w)
    mine = np.zeros(len(good.alpha), dtype=bool)
    mine[sstride:sstride + 2] = True
    same_layout("alpha of the healthy vectors", bad.alpha[~mine], good.alpha[~mine])
    same_layout("b_c of the healthy vectors", bad.bc[~mine], good.bc[~mine])
    mid = np.zeros(len(good.n2), dtype=bool)
    mid[2 * nb:4 * nb] = True
    same_layout("n2out of the healthy vectors", bad.n2[~mid], good.n2[~mid])
    assert not np.isfinite(bad.t[1].real).any() and not np.isfinite(bad.t[1].imag).any()
    assert not np.isfinite(bad.n2[2 * nb:4 * nb:2]).any() and not bad.n2[2 * nb + 1:4 * nb:2].any()
    assert np.isinf(bad.alpha[sstride]) and (np.isinf(bad.alpha[sstride + 1]) if form == 2 else np.isnan(bad.alpha[sstride + 1]))
    assert bad.bc[sstride] == 0.0 and np.isnan(bad.bc[sstride + 1])
