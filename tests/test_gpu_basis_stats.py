"""S^z-basis statistics: sd_basis_moments, sd_counting_statistics, sd_sample_configurations (host and _dev forms) and
the Python mirror (statistics.py) against tests/basis_stats_ref.py (proven on the CPU by tests/test_basis_stats_ref_host.py), against
exact states and against the library's own independent kernels.

Tolerances.  Sums of w = |psi|^2, the bins of P and sum w^q for integer q: elementwise |got - ref| <= 1e-12 x (the sum of the terms'
magnitudes) -- 1e-12 <psi|psi> for P.  Every entry is a sum of at most N bounded non-negative terms and the blocked sums are accurate
to a few tens of eps at these N: the bar and the argument of tests/test_gpu_pair_correlations.py.  Non-integer q and the Shannon sum:
the vectors are normalised first, so w < 1 and every term of sum w ln w has one sign; the device's pow / log add a few ulp (1e-16)
per term to sums without cancellation, three orders inside the same 1e-12 relative bar.  max w is compared with ==: both sides form
re * re + im * im in two roundings.
Snapshots, the interval rule (basis_stats_ref): with C the restatement's cumulative sum over all rows and t_k = u_k C[N-1], the row r
of EVERY shot k must satisfy C[r-1] - delta <= t_k <= C[r] + delta, delta = 1e-12 C[N-1], and w[r] > 0.  delta covers the difference
between the library's summation order and the restatement's; a row displaced by a chunk, or by one row of typical weight 1/N >> delta
at these sizes, fails.  No statistical test: the uniforms are pinned bit for bit on the host (tests/test_basis_stats_host.py).

Shapes: the small ones are those of tests/test_gpu_pair_correlations.py (every shape asserts its sd_model_path, so that the tiled, the
per-row and the full-basis row modes are known to run), the grid-wrap ones those of tests/test_gpu_operator_grids.py."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

import basis_stats_ref as BR
from test_gpu_operator_grids import XXZ, Shape, assert_crosses_the_caps, fill_randn
from test_gpu_pair_correlations import SMALL, build

pytestmark = pytest.mark.gpu

_dp, _u64p, _i64p = C.POINTER(C.c_double), C.POINTER(C.c_uint64), C.POINTER(C.c_int64)
# constants of kernels_basis_stats.hip
MOMENT_MAX_BLOCKS = 1024      # SD_MOMENT_MAX_BLOCKS: row blocks of 256 rows
COUNT_MAX_BLOCKS = 1024       # SD_COUNT_MAX_BLOCKS: row blocks (tiles, or blocks of 256 rows)
COUNT_LDS_BINS = 36           # SD_COUNT_LDS_BINS: bins of a mask chunk
SAMPLE_CHUNK = 1024           # SD_SAMPLE_CHUNK: rows of a sampling chunk
SAMPLE_MAX_BLOCKS = 512       # SD_SAMPLE_MAX_BLOCKS: workgroups of the chunk sums, four chunks per workgroup and trip
SAMPLE_SEG = 1024             # SD_SAMPLE_SEG: chunk weights of a scan segment
SAMPLE_SHOT_BLOCKS = 32       # SD_SAMPLE_SHOT_BLOCKS: workgroups of 64 shots

QS = [0.5, 2.0, 3.0, 2.5]
SMALL_NAMES = ["L2n1-open", "L2n1-periodic", "L4n2-open", "L4n2-periodic", "L12n6-open", "L12n6-periodic", "L16n3-open",
               "L16n3-periodic", "J1J2-L14n7", "L14n7-suffix8", "L13n1-per-row", "full-L10"]


def _args(pkg, m, psi, n, dtype):
    """(entry-point suffix, leading arguments) for a host or a device psi"""
    import torch
    n = len(psi) if n is None else n
    if isinstance(psi, torch.Tensor):
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        code = (pkg._lib.SD_C128 if psi.is_complex() else pkg._lib.SD_F64) if dtype is None else dtype
        return "_dev", (m.ctx.h, m.h, code, psi.data_ptr(), n)
    code = (pkg._lib.SD_C128 if np.iscomplexobj(psi) else pkg._lib.SD_F64) if dtype is None else dtype
    return "", (m.ctx.h, m.h, code, psi.ctypes.data, n)


def raw_moments(pkg, m, psi, qs, n=None, dtype=None, nq=None):
    """status and the 5 + nq doubles of sd_basis_moments[_dev] called directly"""
    q = np.asarray(list(qs) + [2.0] * 10, dtype=np.float64)       # room for an nq past the list
    nq = len(qs) if nq is None else nq
    out = np.full(5 + max(nq, 0) + 4, np.nan)
    sfx, lead = _args(pkg, m, psi, n, dtype)
    rc = getattr(pkg.lib(), "sd_basis_moments" + sfx)(*lead, q.ctypes.data_as(_dp), nq, out.ctypes.data_as(_dp))
    return rc, out[:5 + max(nq, 0)]


def raw_counting(pkg, m, psi, masks, n=None, dtype=None, K=None):
    mk = np.asarray(list(masks) + [0], dtype=np.uint64)
    K = len(masks) if K is None else K
    out = np.full((max(K, 1), m.L + 1), np.nan)
    sfx, lead = _args(pkg, m, psi, n, dtype)
    rc = getattr(pkg.lib(), "sd_counting_statistics" + sfx)(*lead, mk.ctypes.data_as(_u64p), K, out.ctypes.data_as(_dp))
    return rc, out


def raw_sample(pkg, m, psi, shots, seed, n=None, dtype=None, want_rows=True):
    rows = np.full(max(shots, 1), -9, dtype=np.int64)
    cfg = np.full(max(shots, 1), 2 ** 64 - 1, dtype=np.uint64)
    sfx, lead = _args(pkg, m, psi, n, dtype)
    rc = getattr(pkg.lib(), "sd_sample_configurations" + sfx)(*lead, shots, seed, rows.ctypes.data_as(_i64p) if want_rows else None,
                                                              cfg.ctypes.data_as(_u64p))
    return rc, rows[:max(shots, 0)], cfg[:max(shots, 0)]


def normalised(x):
    import torch
    return x / torch.linalg.vector_norm(x)


def check_moments(tag, got, ref, qs):
    """the raw result row against the restatement; prints every figure before it asserts"""
    rel = [abs(got[0] - ref["W"]) / ref["W"], abs(got[1] - ref["wlnw"]) / max(abs(ref["wlnw"]), 1e-300)]
    rel += [abs(got[5 + k] - ref["sums"][k]) / ref["sums"][k] for k in range(len(qs))]
    print(f"{tag}: relative errors W {rel[0]:.2e} wlnw {rel[1]:.2e} " + " ".join(f"q={q}: {e:.2e}" for q, e in zip(qs, rel[2:])) + " (bar 1e-12)")
    assert max(rel) <= 1e-12, (tag, rel)
    assert got[2] == ref["wmax"] and got[3] == ref["argmax"] and got[4] == 0.0, (tag, got[2:5], ref["wmax"], ref["argmax"])


def small_masks(L):
    """all single sites, all cuts, one scattered mask, the empty and the full mask"""
    return [1 << i for i in range(L)] + [(1 << k) - 1 for k in range(1, L)] + [0b1001011010011010110101 & ((1 << L) - 1), 0, (1 << L) - 1]


def check_counting(tag, P, ref, L, nup, masks, W):
    err = np.abs(P - ref).max()
    print(f"{tag}: counting {err:.2e} (bar {1e-12 * W:.2e})")
    assert P.shape == ref.shape and err <= 1e-12 * W, (tag, err)
    for k, mask in enumerate(masks):
        lo, hi = BR.reachable(L, nup, mask)
        assert all(P[k, m] == 0.0 and math.copysign(1.0, P[k, m]) == 1.0 for m in range(L + 1) if m < lo or m > hi), (tag, mask)


# ---- 1. small shapes: both dtypes, host and device forms, every row mode ----
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("name", SMALL_NAMES)
def test_moments_and_counting_small(pkg, name, cplx):
    import torch
    L, nup, boundary, ls, path = SMALL[name]
    m = build(pkg, L, nup, boundary, ls)
    assert pkg.lib().sd_model_path(m.h) == path
    if ls is not None:
        assert len(m.local_tiles()[0]) == 2 ** (L - ls)
    psi = normalised(fill_randn(pkg, m, m.N, cplx, 777 + 5 * L + (nup or 0)))
    host = psi.cpu().numpy()
    ref = BR.moments(psi, QS)
    masks = small_masks(L)
    refP = BR.counting(psi, L, nup, masks)
    for x in (psi, host):
        tag = f"{name} {'c128' if cplx else 'f64'} {'dev' if x is psi else 'host'}"
        rc, got = raw_moments(pkg, m, x, QS)
        assert rc == 0
        check_moments(tag, got, ref, QS)
        rc, P = raw_counting(pkg, m, x, masks)
        assert rc == 0
        check_counting(tag, P, refP, L, nup, masks, ref["W"])
        # the Python mirror.  S_q = ln(sum w^q / W^q) / (1 - q): relative errors of 1e-12 in the two sums give (1 + q) 1e-12 / |1 - q|,
        # at most 3e-12 for the exponents here; Shannon and S_inf likewise 2e-12 (1 + |S|)
        S = pkg.participation_entropy(x, m, QS + [1, math.inf])
        want = [BR.entropy(ref, q, k) for k, q in enumerate(QS)] + [BR.entropy(ref, 1), BR.entropy(ref, math.inf)]
        assert S.shape == (6,) and np.abs(S - np.array(want)).max() <= 3e-12 * (1.0 + max(abs(v) for v in want)), (tag, S, want)
        assert pkg.participation_entropy(x, m, 2) == S[1] and isinstance(pkg.participation_entropy(x, m), float)
        assert abs(pkg.inverse_participation_ratio(x, m) - ref["sums"][1] / ref["W"] ** 2) <= 3e-12 * ref["sums"][1]
        cfg, row, prob = pkg.most_probable_configuration(x, m)
        assert row == ref["argmax"] and cfg == int(m.states_range(row, 1)[0]) and abs(prob - ref["wmax"] / ref["W"]) <= 1e-12
        Pn = pkg.counting_statistics(x, m, [[i + 1 for i in range(L) if (mk >> i) & 1] for mk in masks[:L + 2]])
        assert np.abs(Pn - refP[:L + 2] / ref["W"]).max() <= 2e-12
    # the tie rule: every row of the uniform state attains the maximum, the lowest one is returned
    uni = torch.full((m.N,), 0.25 + (0.5j if cplx else 0.0), dtype=psi.dtype, device=psi.device)
    rc, got = raw_moments(pkg, m, uni, [])
    assert rc == 0 and got[3] == 0.0 and got[2] == (0.3125 if cplx else 0.0625)
    assert pkg.most_probable_configuration(uni, m)[1] == 0


def test_exact_states_through_the_library(pkg):
    """a basis state: S_q = 0.0 exactly and a one-hot P; the uniform state: S_q = ln N; the L = 2 singlet: P = (1/2, 1/2)"""
    m = pkg.XXZChain(12, nup=6, boundary="periodic", **XXZ)
    psi = np.zeros(m.N)
    psi[100] = 1.0
    assert np.array_equal(pkg.participation_entropy(psi, m, [0.5, 1, 2, 3, 2.5, math.inf]), np.zeros(6))
    cfg = int(m.states_range(100, 1)[0])
    P = pkg.cut_counting_statistics(psi, m)
    want = np.zeros((11, 13))
    for k in range(1, 12):
        want[k - 1, bin(cfg & ((1 << k) - 1)).count("1")] = 1.0
    assert np.array_equal(P, want)
    assert pkg.number_entropy(psi, m, [1, 2, 3]) == 0.0
    uni = np.full(m.N, 1.0 / math.sqrt(m.N))
    assert np.abs(pkg.participation_entropy(uni, m, [0.5, 1, 2, math.inf]) - math.log(m.N)).max() <= 1e-12
    s2 = pkg.XXZChain(2, nup=1, **XXZ)
    P = pkg.counting_statistics(np.array([1.0, -1.0]) / math.sqrt(2.0), s2, [[1], [2]])
    assert np.abs(P - np.array([[0.5, 0.5, 0.0], [0.5, 0.5, 0.0]])).max() <= 1e-15
    assert abs(pkg.number_entropy(np.array([1.0, -1.0]), s2, [1]) - math.log(2.0)) <= 1e-15


# ---- 2. identities against the library's independent kernels ----
@pytest.mark.parametrize("name", ["L12n6-periodic", "L16n3-open", "L13n1-per-row", "full-L10"])
def test_identities_against_the_other_kernels(pkg, name):
    """psi normalised.  Every identity compares combinations of at most |A|^2 sums of non-negative terms bounded by <psi|psi> = 1, each
    accurate to 1e-12 on either side: bars 1e-12 for single sums, 1e-12 |A| for the mean, 1e-11 |A|^2 for the variance (which also
    subtracts the squared mean)."""
    L, nup, boundary, ls, path = SMALL[name]
    m = build(pkg, L, nup, boundary, ls)
    psi = normalised(fill_randn(pkg, m, m.N, True, 31 + L))
    subsystems = [[i] for i in range(1, L + 1)] + [list(range(1, k + 1)) for k in range(2, L)] + [[1, 3, 4, L]]
    P = pkg.counting_statistics(psi, m, subsystems, normalize=False)
    sz = pkg.magnetization_per_site(psi, m)
    G = pkg.correlation_matrix(psi, m, "+-")
    Zc = pkg.correlation_matrix(psi, m, "zz", connected=True)
    mvals = np.arange(L + 1)
    assert np.abs(P.sum(axis=1) - 1.0).max() <= 1e-12
    for k, A in enumerate(subsystems):
        x = mvals - 0.5 * len(A)
        mean = float((x * P[k]).sum())
        assert abs(mean - sum(sz[i - 1] for i in A)) <= 1e-12 * len(A), (A, mean)
        var = float((x * x * P[k]).sum()) - mean * mean
        want = sum(Zc[i - 1, j - 1] for i in A for j in A)
        assert abs(var - want) <= 1e-11 * len(A) ** 2, (A, var, want)
        kap = pkg.magnetization_cumulants(P[k], A, order=2)
        assert abs(kap[0] - mean) <= 1e-13 * len(A) and abs(kap[1] - var) <= 1e-12 * len(A) ** 2
    assert np.abs(P[:L, 1] - np.diagonal(G).real).max() <= 1e-12


# ---- 3. the grid-wrap shapes ----
class Shapes:
    def __init__(self, pkg):
        self.pkg, self.store = pkg, {}

    def get(self, name):
        if name not in self.store:
            self.store.clear()
            gc.collect()
            self.store[name] = Shape(self.pkg, name)
        return self.store[name]


@pytest.fixture(scope="module")
def shapes(pkg):
    import torch
    st = Shapes(pkg)
    yield st
    st.store.clear()
    gc.collect()
    torch.cuda.empty_cache()


def vectors(sh):
    """F is the Float64 shape of this module"""
    return (sh.psi_r,) if sh.name == "F" else (sh.psi_r, sh.psi_c)


def chunks_of(pkg, m, masks):
    """bins of the mask chunks the launcher forms: consecutive masks while their reachable bins fit COUNT_LDS_BINS"""
    out, cur = [], 0
    lo, nb = C.c_int(), C.c_int()
    for mk in masks:
        assert pkg.lib().sd_counting_range(m.h, mk, C.byref(lo), C.byref(nb)) == 0
        if cur + nb.value > COUNT_LDS_BINS:
            out.append(cur)
            cur = 0
        cur += nb.value
    return out + [cur]


@pytest.mark.parametrize("name", ["T-periodic", "Ts", "R-periodic", "F"])
def test_grid_wrap_moments(pkg, shapes, name):
    sh = shapes.get(name)
    assert_crosses_the_caps(sh)
    assert sh.N > MOMENT_MAX_BLOCKS * 256                       # the grid-stride loop runs again
    for x in vectors(sh):
        psi = normalised(x)
        ref = BR.moments(psi, QS)
        rc, got = raw_moments(pkg, sh.m, psi, QS)
        assert rc == 0
        check_moments(f"{name} {'c128' if psi.is_complex() else 'f64'}", got, ref, QS)
        rc, again = raw_moments(pkg, sh.m, psi, QS)
        assert rc == 0 and np.array_equal(got.view(np.uint64), again.view(np.uint64))       # same call twice: equal bits
        # the maximum in a late row: a one-pass grid does not reach it
        row = sh.N - 3
        probe = psi.clone()
        probe[row] = 2.0
        rc, got = raw_moments(pkg, sh.m, probe, [])
        assert rc == 0 and got[2] == 4.0 and got[3] == row


@pytest.mark.parametrize("name", ["T-periodic", "Ts", "R-periodic", "F"])
def test_grid_wrap_counting(pkg, shapes, name):
    sh = shapes.get(name)
    assert_crosses_the_caps(sh)
    L = sh.L
    if sh.path == 1:
        assert len(sh.tiles[0]) > COUNT_MAX_BLOCKS               # a workgroup takes a second and later tile
    else:
        assert sh.N > COUNT_MAX_BLOCKS * 256                     # the grid-stride loop runs again
    rng = np.random.default_rng(50 + L)
    scattered = [int(x) for x in rng.integers(1, 1 << min(L, 30), 6)]
    masks = [(1 << k) - 1 for k in range(1, L)] + scattered
    ch = chunks_of(pkg, sh.m, masks)
    while ch[-1] > COUNT_LDS_BINS // 2:                          # ... until the last chunk is a ragged one
        masks.append(int(rng.integers(1, 1 << min(L, 30))))
        ch = chunks_of(pkg, sh.m, masks)
    print(f"{name}: {len(masks)} masks in chunks of {ch} bins")
    assert len(ch) >= 3 and max(ch) <= COUNT_LDS_BINS and ch[-1] <= COUNT_LDS_BINS // 2 < max(ch[:-1])    # three or more chunks, a ragged last one
    for x in vectors(sh):
        psi = normalised(x)
        ref = BR.counting(psi, L, sh.nup, masks, s=sh.s)
        rc, P = raw_counting(pkg, sh.m, psi, masks)
        assert rc == 0
        check_counting(f"{name} {'c128' if psi.is_complex() else 'f64'}", P, ref, L, sh.nup, masks, 1.0)
        assert np.abs(ref).max() > 1e-3                          # a real comparison, not zeros against zeros
        rc, again = raw_counting(pkg, sh.m, psi, masks)
        assert rc == 0 and np.array_equal(P.view(np.uint64), again.view(np.uint64))          # same call twice: equal bits


@pytest.mark.parametrize("name", ["T-periodic", "Ts", "R-periodic", "F"])
def test_grid_wrap_snapshots(pkg, shapes, name):
    """4096 snapshots cross the shot grid's cap on every shape; the chunk sums' grid wraps where the shape has more than
    SAMPLE_MAX_BLOCKS * 4 chunks (T, R, F) and the scan has a second segment there.  Ts (345 chunks) is here for a row count that
    is no multiple of the chunk; the sampler never reads the tile plan, so its short tiles do not enter."""
    import torch
    sh = shapes.get(name)
    assert_crosses_the_caps(sh)
    shots = 4096
    assert shots > SAMPLE_SHOT_BLOCKS * 64
    nchunks = -(-sh.N // SAMPLE_CHUNK)
    if name == "Ts":
        assert sh.N % SAMPLE_CHUNK != 0 and nchunks > 1
    else:
        assert nchunks > SAMPLE_MAX_BLOCKS * 4 and nchunks > SAMPLE_SEG
    for x in vectors(sh):
        w = BR.weights(x)
        cum = torch.cumsum(w, 0)
        rc, rows, cfg = raw_sample(pkg, sh.m, x, shots, 99 + sh.L)
        assert rc == 0
        worst, bad = BR.snapshot_violation(rows, x, 99 + sh.L, cum=cum, w=w)
        print(f"{name} {'c128' if x.is_complex() else 'f64'}: worst excess {worst:.3e} delta, {bad} bad rows, {len(np.unique(rows))} distinct")
        assert bad == 0 and worst <= 1.0
        assert np.array_equal(cfg.astype(np.int64), sh.s[torch.from_numpy(rows).to(sh.dev)].cpu().numpy())
        assert rows.max() > sh.N // 2 > rows.min()                # both halves of the vector are reached
        rc, rows2, cfg2 = raw_sample(pkg, sh.m, x, shots, 99 + sh.L)
        assert rc == 0 and np.array_equal(rows, rows2) and np.array_equal(cfg, cfg2)


# ---- 4. rows past 2^31 ----
def test_rows_past_2_31(pkg):
    """B: L = 34, nup = 17, Float64, 2.33e9 rows: moments, one cut mask (the restatement forms the configurations slab by slab) and
    256 snapshots against torch.cumsum on the device."""
    import torch
    L, nup = 34, 17
    m = pkg.XXZChain(L, nup=nup, boundary="open", **XXZ)
    N = m.N
    assert N > 2 ** 31 and m.device_path == "tiled" and len(m.local_tiles()[0]) > COUNT_MAX_BLOCKS
    assert -(-N // SAMPLE_CHUNK) > SAMPLE_SEG * 256             # the scan's per-segment kernels run past their first workgroup
    gc.collect()
    torch.cuda.empty_cache()
    pkg.default_context().release_scratch()
    free, _ = torch.cuda.mem_get_info()
    if free < 6 * 8 * N + (3 << 30):
        pytest.skip("not enough device memory")
    psi = fill_randn(pkg, m, N, False, 20261020)
    psi /= torch.linalg.vector_norm(psi)
    qs = [2.0, 0.5]
    ref = BR.moments(psi, qs)
    rc, got = raw_moments(pkg, m, psi, qs)
    assert rc == 0
    check_moments("B f64", got, ref, qs)
    probe_row = N - 5
    keep = float(psi[probe_row].item())
    psi[probe_row] = 0.5
    rc, got = raw_moments(pkg, m, psi, [])
    assert rc == 0 and got[2] == 0.25 and got[3] == probe_row and probe_row > 2 ** 31
    psi[probe_row] = keep
    mask = (1 << (L // 2)) - 1
    refP = BR.counting(psi, L, nup, [mask])
    rc, P = raw_counting(pkg, m, psi, [mask])
    assert rc == 0
    check_counting("B f64", P, refP, L, nup, [mask], ref["W"])
    w = BR.weights(psi)
    cum = torch.cumsum(w, 0)
    rc, rows, cfg = raw_sample(pkg, m, psi, 256, 5)
    assert rc == 0
    worst, bad = BR.snapshot_violation(rows, psi, 5, cum=cum, w=w)
    print(f"B: worst excess {worst:.3e} delta, {bad} bad rows, largest row {rows.max()}")
    assert bad == 0 and worst <= 1.0 and rows.max() > 2 ** 31
    dev = torch.device("cuda", m.ctx.device)
    assert np.array_equal(cfg.astype(np.int64), BR.RR.unrank_t(torch.from_numpy(rows).to(dev), L, nup).cpu().numpy())
    del psi, w, cum
    torch.cuda.empty_cache()


# ---- 5. snapshots ----
def test_snapshots_depend_on_psi_seed_and_shots_alone(pkg):
    import torch
    L, nup = 14, 7
    m = build(pkg, L, nup, "periodic", None)
    m8 = build(pkg, L, nup, "periodic", 8)
    assert len(m8.local_tiles()[0]) == 2 ** (L - 8) != len(m.local_tiles()[0])
    assert m.N % SAMPLE_CHUNK != 0 and m.N > 3 * SAMPLE_CHUNK                  # N is no multiple of a chunk
    for cplx in (False, True):
        psi = fill_randn(pkg, m, m.N, cplx, 4 + cplx)
        host = psi.cpu().numpy()
        seed, shots = 2 ** 63 + 17, 2 ** 16
        rc, rows, cfg = raw_sample(pkg, m, psi, shots, seed)
        assert rc == 0
        worst, bad = BR.snapshot_violation(rows, psi, seed)
        print(f"c128={cplx}: worst excess {worst:.3e} delta over {shots} shots, {len(np.unique(rows))} of {m.N} rows drawn")
        assert bad == 0 and worst <= 1.0
        assert np.array_equal(cfg, m.states_range(0, m.N)[rows])                 # configs[k] is the configuration of rows[k]
        for other, mm in ((host, m), (psi, m8), (host, m8), (psi, m)):           # host form, the other plan, the call repeated
            rc, r2, c2 = raw_sample(pkg, mm, other, shots, seed)
            assert rc == 0 and np.array_equal(rows, r2) and np.array_equal(cfg, c2)
        for fewer in (1, 63, 64, 2049):                                          # shot k of a call is shot k of a longer call
            rc, r2, c2 = raw_sample(pkg, m, psi, fewer, seed)
            assert rc == 0 and np.array_equal(rows[:fewer], r2) and np.array_equal(cfg[:fewer], c2)
        rc, _r, c2 = raw_sample(pkg, m, psi, 100, seed, want_rows=False)         # rows_out may be NULL
        assert rc == 0 and np.array_equal(c2, cfg[:100])
        rc, r3, _c = raw_sample(pkg, m, psi, 100, seed + 1)
        assert rc == 0 and not np.array_equal(r3, rows[:100])                    # another seed, another stream
        c4, r4 = pkg.sample_configurations(psi, m, 100, seed=seed, return_rows=True)
        assert np.array_equal(c4, cfg[:100]) and np.array_equal(r4, rows[:100]) and c4.dtype == np.uint64
        assert np.array_equal(pkg.sample_configurations(host, m, 100, seed=seed), cfg[:100])
        sp = pkg.snapshot_spins(c4, L)
        assert sp.shape == (100, L) and np.all(sp.sum(axis=1) == nup - L / 2)
    rc, rows, cfg = raw_sample(pkg, m, psi, 0, 1)                                # shots = 0 writes nothing
    assert rc == 0 and len(pkg.sample_configurations(psi, m, 0)) == 0


def test_snapshots_of_sparse_states_never_return_a_zero_weight_row(pkg):
    import torch
    L, nup = 14, 7
    m = build(pkg, L, nup, "periodic", None)
    N = m.N
    shots = 4096
    # a basis state: every shot is its row
    neel = np.asarray(pkg.neel_state(m))
    (row,) = np.nonzero(neel)[0]
    for x in (neel, neel.astype(np.complex128) * 1j):
        rc, rows, cfg = raw_sample(pkg, m, x, shots, 3)
        assert rc == 0 and np.all(rows == row) and np.all(cfg == m.states_range(int(row), 1)[0])
    # three basis states with weights 0.5 / 0.3 / 0.2, in three different chunks
    three = np.zeros(N)
    picks = [5, SAMPLE_CHUNK + 700, N - 1]
    three[picks] = np.sqrt([0.5, 0.3, 0.2])
    rc, rows, _ = raw_sample(pkg, m, three, shots, 4)
    worst, bad = BR.snapshot_violation(rows, three, 4)
    assert rc == 0 and bad == 0 and worst <= 1.0 and set(rows.tolist()) == set(picks)
    # a vector whose last 2000 rows are zero (the last chunk and part of the one before hold nothing)
    tail = fill_randn(pkg, m, N, False, 8)
    tail[N - 2000:] = 0.0
    for x in (tail, tail.cpu().numpy()):
        rc, rows, _ = raw_sample(pkg, m, x, shots, 5)
        worst, bad = BR.snapshot_violation(rows, tail, 5)
        assert rc == 0 and bad == 0 and worst <= 1.0 and rows.max() < N - 2000
    # ... and whose first rows are zero too, with single rows of weight left between runs of zeros
    gaps = fill_randn(pkg, m, N, False, 12)
    gaps[:1500] = 0.0
    gaps[2048:3072:2] = 0.0
    gaps[3300:] = 0.0
    rc, rows, _ = raw_sample(pkg, m, gaps, shots, 6)
    worst, bad = BR.snapshot_violation(rows, gaps, 6)
    assert rc == 0 and bad == 0 and worst <= 1.0 and rows.min() >= 1500 and rows.max() < 3300
    # N smaller than a chunk
    tiny = pkg.XXZChain(8, nup=4, boundary="open", **XXZ)
    assert tiny.N < SAMPLE_CHUNK
    for cplx in (False, True):
        psi = fill_randn(pkg, tiny, tiny.N, cplx, 9)
        rc, rows, cfg = raw_sample(pkg, tiny, psi, shots, 7)
        worst, bad = BR.snapshot_violation(rows, psi, 7)
        assert rc == 0 and bad == 0 and worst <= 1.0 and np.array_equal(cfg, tiny.states_range(0, tiny.N)[rows])
    one = pkg.XXZChain(6, nup=6, **XXZ)
    rc, rows, cfg = raw_sample(pkg, one, np.array([0.3]), 10, 1)
    assert rc == 0 and np.all(rows == 0) and np.all(cfg == 63)
    full = pkg.XXZChain(10, nup=None, boundary="periodic", **XXZ)
    psi = fill_randn(pkg, full, full.N, True, 10)
    rc, rows, cfg = raw_sample(pkg, full, psi, shots, 8)
    worst, bad = BR.snapshot_violation(rows, psi, 8)
    assert rc == 0 and bad == 0 and worst <= 1.0 and np.array_equal(cfg.astype(np.int64), rows)     # rows are configurations


# ---- 6. statuses ----
def test_statuses(pkg):
    E = pkg._lib
    L = 12
    m = pkg.XXZChain(L, nup=6, boundary="periodic", **XXZ)
    psi = fill_randn(pkg, m, m.N, True, 99)
    host = psi.cpu().numpy()
    sharded = pkg.XXZChain(L, nup=6, boundary="periodic", **XXZ)
    sharded.set_shard(0, 2)
    for x in (psi, host):
        assert raw_moments(pkg, sharded, x, QS)[0] == E.SD_EARG
        assert raw_counting(pkg, sharded, x, [3])[0] == E.SD_EARG
        assert raw_sample(pkg, sharded, x, 4, 1)[0] == E.SD_EARG
        assert raw_moments(pkg, m, x, QS, n=m.N - 1)[0] == E.SD_EDIM
        assert raw_counting(pkg, m, x, [3], n=m.N + 1)[0] == E.SD_EDIM
        assert raw_sample(pkg, m, x, 4, 1, n=m.N - 1)[0] == E.SD_EDIM
        assert raw_moments(pkg, m, x, QS, dtype=3)[0] == E.SD_EARG
        assert raw_counting(pkg, m, x, [1 << L])[0] == E.SD_EARG and raw_counting(pkg, m, x, [3, 1 << 63])[0] == E.SD_EARG
        assert raw_counting(pkg, m, x, [], K=0)[0] == E.SD_EARG
        assert raw_counting(pkg, m, x, [1] * 257)[0] == E.SD_EARG and raw_counting(pkg, m, x, [1] * 256)[0] == 0
        for bad in ([2.0, 1.0], [0.0], [-1.5], [math.inf], [math.nan]):
            assert raw_moments(pkg, m, x, bad)[0] == E.SD_EARG, bad
        assert raw_moments(pkg, m, x, [2.0] * 9)[0] == E.SD_EARG and raw_moments(pkg, m, x, [2.0] * 8)[0] == 0
        assert raw_moments(pkg, m, x, [], nq=-1)[0] == E.SD_EARG
        assert raw_sample(pkg, m, x, -1, 1)[0] == E.SD_EARG
        zero = x * 0.0
        assert raw_sample(pkg, m, zero, 4, 1)[0] == E.SD_EZERO
        rc, got = raw_moments(pkg, m, zero, [2.0])
        assert rc == 0 and np.array_equal(got, np.zeros(6))
    full = pkg.XXZChain(10, nup=None, boundary="periodic", **XXZ)
    assert raw_counting(pkg, full, np.ones(full.N), [(1 << 10) - 1])[0] == 0          # 11 bins
    with pytest.raises(pkg.ZeroNormError):
        pkg.sample_configurations(host * 0.0, m, 3)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.counting_statistics(host[:-1], m, [[1]])
    # the Python layer refuses before any launch
    for call in (lambda: pkg.counting_statistics(host, m, [[0]]), lambda: pkg.counting_statistics(host, m, [[L + 1]]),
                 lambda: pkg.counting_statistics(host, m, [[2, 2]]), lambda: pkg.counting_statistics(host, m, []),
                 lambda: pkg.participation_entropy(host, m, 0), lambda: pkg.participation_entropy(host, m, [2, -1]),
                 lambda: pkg.sample_configurations(host, m, -1), lambda: pkg.sample_configurations(host, m, 2.5),
                 lambda: pkg.number_entropy(host, sharded, [1])):
        with pytest.raises(pkg.ArgumentError):
            call()
    # more than 256 subsystems run in several calls
    many = [[1 + (k % L)] for k in range(300)]
    P = pkg.counting_statistics(host, m, many)
    assert P.shape == (300, L + 1) and np.array_equal(P[0], P[L]) and np.array_equal(P[299], P[299 - 24 * L])
