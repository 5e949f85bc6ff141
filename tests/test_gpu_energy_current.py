"""The energy current: sd_dcurrent_apply / sd_dcurrent_bracket, their Python mirror and the ("energy_current", .)
operator of the typicality driver, against tests/ecurrent_ref.py (proven on the CPU by tests/test_ecurrent_ref_host.py).

The write form is compared bit for bit -- real and imaginary parts as IEEE doubles under == -- on ALL rows: the library is built
without contraction and the row form fixes every operation and its order.  Bracket sums differ from an exactly rounded sum
(math.fsum) of the same products only by the reduction tree: about 23 levels of 1.1e-16, hence the bar 1e-13 sum |bra[s] (J ket)[s]|.
Small shapes are those of tests/test_gpu_pair_correlations.py, grid-wrap shapes those of tests/test_gpu_operator_grids.py.

The two-site shapes take the list of the open geometry: their one bond has delta = 1 = L/2, which a ring refuses."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

import ecurrent_ref as ER
import typicality_ref as TR
from test_gpu_operator_grids import SPECS, XXZ, Shape, assert_crosses_the_caps, fill_randn, j1j2, nan_complex
from test_gpu_pair_correlations import SMALL, build

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)


def geometry(L, boundary):
    return "open" if boundary == "open" or L == 2 else "periodic"


def hand_list(L):
    """a reversed pair (i > j); a k = 0 term between two dressed terms of one group; a long pair (2, L - 1), which straddles the
    prefix / suffix cut of every tiled plan with a prefix of two sites or more"""
    if L == 2:
        return np.array([(2, 1, 0, 0.3), (1, 2, 0, -0.4)], dtype=ER.DTERM)
    if L == 4:
        return np.array([(3, 2, 1, 0.3), (2, 3, 1, 0.7), (2, 3, 0, -0.4), (2, 3, 4, 1.1)], dtype=ER.DTERM)
    return np.array([(L - 1, 2, 1, 0.3), (2, L - 1, 3, 0.7), (2, L - 1, 0, -0.4), (2, L - 1, L, 1.1), (1, 2, 0, 0.25), (1, 2, L, 0.5),
                     (L, 1, 3, -0.6)], dtype=ER.DTERM)


def same_bits(got, want):
    return bool(np.all(got.real == want.real) and np.all(got.imag == want.imag))


def raw_apply(pkg, m, psi, terms, out, n=None, n_terms=None, dtype=None):
    """status of sd_dcurrent_apply[_dev] called directly, so that the caller owns (and pre-fills) the output"""
    import torch
    tl = np.ascontiguousarray(terms, dtype=ER.DTERM)
    n = len(psi) if n is None else n
    nt = len(tl) if n_terms is None else n_terms
    tp = tl.ctypes.data if len(tl) else None
    if isinstance(psi, torch.Tensor):
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        code = (pkg._lib.SD_C128 if psi.is_complex() else pkg._lib.SD_F64) if dtype is None else dtype
        rc = pkg.lib().sd_dcurrent_apply_dev(m.ctx.h, m.h, code, psi.data_ptr(), n, tp, nt, out.data_ptr())
        torch.cuda.synchronize()
        return rc
    code = (pkg._lib.SD_C128 if np.iscomplexobj(psi) else pkg._lib.SD_F64) if dtype is None else dtype
    return pkg.lib().sd_dcurrent_apply(m.ctx.h, m.h, code, psi.ctypes.data, n, tp, nt, out.ctypes.data)


def raw_bracket(pkg, m, bra, ket, terms, n=None, dtype=None):
    import torch
    tl = np.ascontiguousarray(terms, dtype=ER.DTERM)
    out = np.full(2, np.nan)
    n = len(ket) if n is None else n
    tp = tl.ctypes.data if len(tl) else None
    if isinstance(bra, torch.Tensor):
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        code = (pkg._lib.SD_C128 if bra.is_complex() else pkg._lib.SD_F64) if dtype is None else dtype
        rc = pkg.lib().sd_dcurrent_bracket_dev(m.ctx.h, m.h, code, bra.data_ptr(), ket.data_ptr(), n, tp, len(tl), out.ctypes.data_as(_dp))
    else:
        code = (pkg._lib.SD_C128 if np.iscomplexobj(bra) else pkg._lib.SD_F64) if dtype is None else dtype
        rc = pkg.lib().sd_dcurrent_bracket(m.ctx.h, m.h, code, bra.ctypes.data, ket.ctypes.data, n, tp, len(tl), out.ctypes.data_as(_dp))
    return rc, complex(out[0], out[1])


def fsum_bracket(bra, jket):
    """(exactly rounded sum of conj(bra[s]) jket[s], sum of |bra[s] jket[s]|)"""
    br, bi = (bra.real, bra.imag) if np.iscomplexobj(bra) else (bra, np.zeros(len(bra)))
    re = math.fsum(br * jket.real) + math.fsum(bi * jket.imag)
    im = math.fsum(br * jket.imag) - math.fsum(bi * jket.real)
    return complex(re, im), float(np.abs(bra * jket).sum())


# ---- 1. the write form is the row loop, bit for bit, on all rows ----
def check_all_rows(pkg, m, L, nup, terms, seed):
    N = m.N
    for cplx in (False, True):
        psi = fill_randn(pkg, m, N, cplx, seed + cplx)
        host = psi.cpu().numpy()
        want = ER.apply_rows(terms, host, L, nup)
        got_d = pkg.energy_current(psi, m, terms)
        got_h = pkg.energy_current(host, m, terms)
        assert got_h.dtype == np.complex128 and got_h.shape == (N,)
        assert same_bits(got_d.cpu().numpy(), want), f"device input, {'c128' if cplx else 'f64'}"
        assert same_bits(got_h, want), f"host input, {'c128' if cplx else 'f64'}"
        if not cplx:
            assert np.all(got_h.real == 0.0)
    return want


@pytest.mark.parametrize("name", list(SMALL))
def test_write_form_small(pkg, name):
    L, nup, boundary, ls, path = SMALL[name]
    m = build(pkg, L, nup, boundary, ls)
    assert pkg.lib().sd_model_path(m.h) == path
    terms = pkg.energy_current_terms(m, geometry(L, boundary))
    ref_terms = ER.energy_current_terms(L, m.hopping_list, m.zz_list, m.onsite_field, geometry(L, boundary) == "periodic")
    assert np.array_equal(terms, ref_terms)
    assert len(terms) > 0
    want = check_all_rows(pkg, m, L, nup, terms, 77 + L)
    if m.N > 1:
        assert np.abs(want).max() > 0
    check_all_rows(pkg, m, L, nup, hand_list(L), 99 + L)
    empty = np.zeros(0, dtype=ER.DTERM)
    psi = fill_randn(pkg, m, m.N, True, 5)
    out = nan_complex(m.N, psi.device)
    assert raw_apply(pkg, m, psi, empty, out) == 0 and not out.cpu().numpy().any()
    assert not pkg.energy_current(psi.cpu().numpy(), m, []).any()
    assert raw_bracket(pkg, m, psi, psi, empty) == (0, 0j)
    # terms=None is the model's own list
    assert same_bits(pkg.energy_current(psi, m, boundary=geometry(L, boundary)).cpu().numpy(),
                     pkg.energy_current(psi, m, terms).cpu().numpy())


@pytest.mark.parametrize("L,nup", [(12, 0), (12, 12), (2, 0), (2, 2), (13, 0), (13, 13)])
def test_polarised_sectors(pkg, L, nup):
    m = pkg.XXZChain(L, nup=nup, boundary="open", **XXZ)
    assert m.N == 1
    for terms in (pkg.energy_current_terms(m, "open"), hand_list(L)):
        want = check_all_rows(pkg, m, L, nup, terms, 3)
        assert not want.any()
        psi = fill_randn(pkg, m, 1, True, 8)
        assert raw_bracket(pkg, m, psi, psi, terms) == (0, 0j)


def test_bracket_and_hermiticity_small(pkg):
    for name in ("L16n8-periodic", "J1J2-L14n7", "L14n7-suffix8", "L13n1-per-row", "full-L10", "L2n1-open"):
        L, nup, boundary, ls, _path = SMALL[name]
        m = build(pkg, L, nup, boundary, ls)
        for terms in (pkg.energy_current_terms(m, geometry(L, boundary)), hand_list(L)):
            phi, psi = fill_randn(pkg, m, m.N, True, 31), fill_randn(pkg, m, m.N, True, 32)
            phr = fill_randn(pkg, m, m.N, False, 33)
            ph, ps, pr = phi.cpu().numpy(), psi.cpu().numpy(), phr.cpu().numpy()
            jps, jph = ER.apply_rows(terms, ps, L, nup), ER.apply_rows(terms, ph, L, nup)
            want, bar = fsum_bracket(ph, jps)
            back, bar2 = fsum_bracket(ps, jph)
            a = pkg.energy_current_expectation(phi, psi, m, terms)
            b = pkg.energy_current_expectation(psi, phi, m, terms)
            print(f"{name}: |<phi|J|psi> - fsum| = {abs(a - want):.2e} (bar {1e-13 * bar:.2e}), "
                  f"|a - conj b| = {abs(a - b.conjugate()):.2e} (bar {1e-13 * (bar + bar2):.2e})")
            assert abs(a - want) <= 1e-13 * bar and abs(b - back) <= 1e-13 * bar2
            assert abs(a - b.conjugate()) <= 1e-13 * (bar + bar2)                       # Hermitian
            assert bar > 0                                                              # not a vacuous zero
            assert pkg.energy_current_expectation(ph, ps, m, terms) == a                # host input: the same bits
            wr, bar_r = fsum_bracket(pr, jps)                                           # a Float64 bra
            assert abs(pkg.energy_current_expectation(phr, psi, m, terms) - wr) <= 1e-13 * bar_r
            assert pkg.energy_current_expectation(pr, ps, m, terms) == pkg.energy_current_expectation(phr, psi, m, terms)


# ---- 2. the grid-wrap shapes ----
@pytest.fixture(scope="module")
def big(pkg):
    import torch
    store = {}
    yield store
    store.clear()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ["T-periodic", "Ts", "R-periodic", "Rg", "F"])
def test_grid_wrap(pkg, big, name):
    import torch
    big.clear()
    gc.collect()
    torch.cuda.empty_cache()
    sh = Shape(pkg, name)
    big[name] = sh
    assert_crosses_the_caps(sh)
    m, N = sh.m, sh.N
    terms = pkg.energy_current_terms(m, "periodic")
    assert len(terms) == (4 * sh.L if SPECS[name][2] is not None else 546)
    ref = ER.apply_rows_t(terms, [sh.psi_r, sh.psi_c], sh.s, sh.rows, sh.L, sh.nup)
    for psi, (re, im) in zip((sh.psi_r, sh.psi_c), ref):
        out = nan_complex(N, sh.dev)
        assert raw_apply(pkg, m, psi, terms, out) == 0
        bad = (out.real != re) | (out.imag != im)
        assert not bool(bad.any()), f"{name}: {int(bad.sum())} of {N} rows differ; first {bad.nonzero().flatten()[:8].tolist()}"
    re, im = ref[1]
    assert float(re.abs().max()) > 0
    jket = torch.complex(re, im)
    # probe bras e_r pick one row exactly: every other term is an exact zero
    probes = sh.probe_rows()
    for r in (probes[-1], probes[len(probes) // 2], probes[-2]):
        bra = torch.zeros(N, dtype=torch.complex128, device=sh.dev)
        bra[r] = 1.0
        rc, got = raw_bracket(pkg, m, bra, sh.psi_c, terms)
        want = complex(jket[r].item())
        assert rc == 0 and got.real == want.real and got.imag == want.imag, (name, r, got, want)
    del bra
    bra = sh.bra_c(pkg)
    want, bar = fsum_bracket(bra.cpu().numpy(), jket.cpu().numpy())
    rc, got = raw_bracket(pkg, m, bra, sh.psi_c, terms)
    print(f"{name}: |bracket - fsum| = {abs(got - want):.2e} (bar {1e-13 * bar:.2e})")
    assert rc == 0 and abs(got - want) <= 1e-13 * bar
    assert raw_bracket(pkg, m, bra, sh.psi_c, terms) == (0, got)                        # equal bits on repeat
    big.clear()


# ---- 4. conservation against the hot path ----
def one_norms(m, terms):
    """row-sum bounds of H and of the list, from the lists"""
    h1 = sum(abs(t) for _i, _j, t in m.hopping_list) + sum(abs(v) for _i, _j, v in m.zz_list) / 4 + np.abs(m.onsite_field).sum() / 2
    return float(h1), ER.row_sum_bound(terms)


def commutator_inf(pkg, m, terms, seed):
    import torch
    psi = fill_randn(pkg, m, m.N, True, seed)
    hpsi, hj = torch.empty_like(psi), torch.empty_like(psi)
    pkg.apply_H(hpsi, psi, m)
    jpsi = pkg.energy_current(psi, m, terms)
    pkg.apply_H(hj, jpsi, m)
    jh = pkg.energy_current(hpsi, m, terms)
    torch.cuda.synchronize()
    return float((hj - jh).abs().max()), float(psi.abs().max())


def test_energy_current_commutes_with_the_apply_on_the_xxz_ring(pkg, big):
    L, nup = SPECS["T-periodic"][:2]
    m = pkg.XXZChain(L, nup=nup, boundary="periodic", Jxy=XXZ["Jxy"], Jz=XXZ["Jz"], hz=0.0)
    assert pkg.lib().sd_model_path(m.h) == 1 and m.N == 5_200_300
    terms = pkg.energy_current_terms(m, "periodic")
    assert len(terms) == 3 * L
    h1, j1 = one_norms(m, terms)
    d, pmax = commutator_inf(pkg, m, terms, 71)
    print(f"XXZ ring L={L}: |[H, J_E] psi|_inf = {d:.2e} (bar {1e-12 * h1 * j1 * pmax:.2e})")
    assert d <= 1e-12 * h1 * j1 * pmax


def test_second_neighbours_break_the_conservation(pkg):
    L = 20
    hop, zz, _f = j1j2(L)
    m = pkg.build_model(L, nup=10, hopping=hop, zz=zz, onsite_field=np.zeros(L))
    terms = pkg.energy_current_terms(m, "periodic")
    d, pmax = commutator_inf(pkg, m, terms, 72)
    print(f"J1-J2 ring L={L}: |[H, J_E] psi|_inf = {d:.2e} (at least {1e-3 * pmax:.2e})")
    assert d >= 1e-3 * pmax


# ---- 5. typicality ----
class DenseOp:
    """an operator of typicality_ref.dqt_sample from its dense matrix on the basis"""

    def __init__(self, M):
        self.M = M

    def apply(self, psi):
        return self.M @ psi

    def bracket(self, bra, ket):
        return np.array([np.vdot(bra, self.M @ ket)])


def ring_or_line(pkg, L, nup, boundary, hz=0.2):
    m = pkg.XXZChain(L, nup=nup, boundary=boundary, Jxy=1.0, Jz=0.8, hz=hz)
    states, index = TR.basis(L, nup)
    H = TR.hamiltonian(L, nup, m.hopping_list, m.zz_list, m.onsite_field, states, index)
    return m, H, states


@pytest.mark.parametrize("method", ["chebyshev", "krylov"])
@pytest.mark.parametrize("beta", [0.0, 1.0])
@pytest.mark.parametrize("boundary", ["periodic", "open"])
def test_typicality_against_dense(pkg, boundary, beta, method):
    L, nup = 10, 5
    m, H, states = ring_or_line(pkg, L, nup, boundary)
    terms = ER.energy_current_terms(L, m.hopping_list, m.zz_list, m.onsite_field, boundary == "periodic")
    op = DenseOp(TR.project(ER.kron_terms(L, terms), states))
    Hd = H.toarray()
    w = np.linalg.eigvalsh(Hd)
    Eb = (w[0] - 0.05, w[-1] + 0.05)
    rng = np.random.default_rng(21)
    r = rng.standard_normal(m.N) + 1j * rng.standard_normal(m.N)
    times = [0.0, 0.4, 0.8, 1.2, 1.6]
    num_d, ln_d, en_d = TR.dqt_dense(Hd, op, op, beta, r, times)
    num_r, ln_r, en_r = TR.dqt_sample(H, op, op, beta, r, times, method=method, Ebounds=Eb, kry_m=30)
    kw = dict(method=method, kry_m=30)
    if method == "chebyshev":
        kw["Ebounds"] = Eb
    A = ("energy_current", boundary)
    got = pkg.typicality_correlation_function(m, beta, A, A, times, r=r, **kw)
    assert got.shape == (len(times),)
    num = got.num[0].reshape(-1, 1)
    scale = ER.row_sum_bound(terms) ** 2
    hs = np.abs(w[[0, -1]]).max()
    e_num, r_num = np.abs(num - num_d).max(), np.abs(num_r - num_d).max()
    e_den, r_den = abs(np.expm1(2 * (got.log_norm[0] - ln_d))), abs(np.expm1(2 * (ln_r - ln_d)))
    e_en, r_en = abs(got.energy[0] - en_d), abs(en_r - en_d)
    print(f"{boundary} beta={beta} {method}: num {e_num:.2e} (ref {r_num:.2e}, base {1e-12 * scale:.2e}), den {e_den:.2e}, energy {e_en:.2e}")
    assert np.abs(num_d).max() > 1e-2
    assert e_num <= 2 * r_num + 1e-12 * scale
    assert e_den <= 2 * r_den + 1e-12
    assert e_en <= 2 * r_en + 1e-12 * hs


def test_energy_current_correlations_stay_flat_on_the_xxz_ring_only(pkg):
    L, nup, beta = 16, 8, 0.5
    times = 0.4 * np.arange(10)
    A = ("energy_current", "periodic")
    ring = pkg.XXZChain(L, nup=nup, boundary="periodic", Jxy=1.0, Jz=1.0, hz=0.0)
    Cr = np.asarray(pkg.typicality_correlation_function(ring, beta, A, A, times, seed=3))
    bar = 1e-12 * ER.row_sum_bound(pkg.energy_current_terms(ring, "periodic")) ** 2
    spread = np.abs(Cr - Cr[0]).max()
    print(f"XXZ ring: C(0) = {Cr[0]:.6f}, spread {spread:.2e} (bar {bar:.2e})")
    assert abs(Cr[0]) > 0.1 and spread <= bar
    hop, zz, _f = j1j2(L)
    jj = pkg.build_model(L, nup=nup, hopping=hop, zz=zz, onsite_field=np.zeros(L))
    Cj = np.asarray(pkg.typicality_correlation_function(jj, beta, A, A, times, seed=3))
    spread = np.abs(Cj - Cj[0]).max()
    print(f"J1-J2 ring: C(0) = {Cj[0]:.6f}, spread {spread:.2e} (at least {1e-3 * abs(Cj[0]):.2e})")
    assert spread >= 1e-3 * abs(Cj[0])


def raw_dqt(pkg, m, A_kind, A_param, wA, B_kind, B_param, wB):
    t = np.array([0.0, 0.1])
    num = np.empty(2 * len(t))
    den, en, ln = C.c_double(), C.c_double(), C.c_double()
    p = lambda w: None if w is None else w.ctypes.data_as(_dp)      # noqa: E731
    return pkg.lib().sd_dqt_correlations(m.ctx.h, m.h, 0.5, None, 1, B_kind, B_param, p(wB), A_kind, A_param, p(wA),
                                         t.ctypes.data_as(_dp), len(t), 0, 0, 30, 0.0, 0.0, num.ctypes.data_as(_dp),
                                         C.byref(den), C.byref(en), C.byref(ln))


def test_typicality_refusals(pkg):
    E = pkg._lib
    m = pkg.XXZChain(10, nup=5, boundary="periodic", **XXZ)
    w = np.ones(len(m.hopping_list))
    assert raw_dqt(pkg, m, 4, 1.0, None, 4, 1.0, None) == 0
    assert raw_dqt(pkg, m, 4, 1.0, w, 4, 1.0, None) == E.SD_EARG                        # w must be NULL
    assert raw_dqt(pkg, m, 4, 1.0, None, 4, 1.0, w) == E.SD_EARG
    assert raw_dqt(pkg, m, 4, 2.0, None, 4, 1.0, None) == E.SD_EARG                     # the geometry is 0 or 1
    assert raw_dqt(pkg, m, 3, 0.0, w, 4, 0.0, None) == 0                                # mixed with the spin current
    assert raw_dqt(pkg, m, 4, 1.0, None, 4, 1.0, None) == 0
    with pytest.raises(pkg.ArgumentError):
        pkg.typicality_correlation_function(m, 0.5, ("energy_current", "ring"), ("Sz", 1), [0.0])


# ---- 6. refusals ----
def test_refusals(pkg):
    import torch
    E = pkg._lib
    L = 12
    m = pkg.XXZChain(L, nup=6, boundary="periodic", **XXZ)
    psi = fill_randn(pkg, m, m.N, True, 99)
    host = psi.cpu().numpy()
    good = pkg.energy_current_terms(m, "periodic")
    want = ER.apply_rows(good, host, L, 6)

    def still_usable():
        assert same_bits(pkg.energy_current(psi, m, good).cpu().numpy(), want)

    def bad_list(i, j, k, c):
        tl = good.copy()
        tl[len(tl) // 2] = (i, j, k, c)
        return tl

    bad_lists = [bad_list(3, 3, 0, 1.0), bad_list(3, 4, 3, 1.0), bad_list(3, 4, 4, 1.0),           # i == j, k in {i, j}
                 bad_list(0, 4, 0, 1.0), bad_list(3, L + 1, 0, 1.0), bad_list(-1, 4, 5, 1.0),     # a site outside 1..L
                 bad_list(3, 4, L + 1, 1.0), bad_list(3, 4, -1, 1.0),
                 bad_list(3, 4, 5, float("nan")), bad_list(3, 4, 0, float("inf"))]                 # a non-finite c
    for x in (psi, host):
        out = torch.empty_like(psi) if x is psi else np.empty_like(host)
        assert raw_apply(pkg, m, x, good, out) == 0 and raw_bracket(pkg, m, x, x, good)[0] == 0
        for tl in bad_lists:
            assert raw_apply(pkg, m, x, tl, out) == E.SD_EARG
            assert raw_bracket(pkg, m, x, x, tl)[0] == E.SD_EARG
            still_usable()
        assert raw_apply(pkg, m, x, good, out, n_terms=-1) == E.SD_EARG
        assert raw_apply(pkg, m, x, np.resize(good, 4097), out) == E.SD_EARG
        assert raw_apply(pkg, m, x, np.resize(good, 4096), out) == 0
        assert raw_apply(pkg, m, x, good, out, n=m.N - 1) == E.SD_EDIM and raw_bracket(pkg, m, x, x, good, n=m.N + 1)[0] == E.SD_EDIM
        assert raw_apply(pkg, m, x, good, out, dtype=3) == E.SD_EARG and raw_bracket(pkg, m, x, x, good, dtype=0)[0] == E.SD_EARG
        still_usable()
    assert raw_apply(pkg, m, psi, good, psi) == E.SD_EARG                                          # out aliasing psi on the device
    still_usable()
    with pytest.raises(pkg.ArgumentError):
        pkg.energy_current(psi, m, [(1, 1, 0, 1.0)])
    with pytest.raises(pkg.ArgumentError):
        pkg.energy_current(psi, m, boundary="ring")
    with pytest.raises(pkg.DimensionMismatch):
        pkg.energy_current(host[:-1], m, good)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.energy_current_expectation(psi[:-1].contiguous(), psi, m, good)
    with pytest.raises(pkg.ArgumentError):
        pkg.energy_current_expectation(host, psi, m, good)
    # a sharded model
    sharded = pkg.XXZChain(L, nup=6, boundary="periodic", **XXZ)
    sharded.set_shard(0, 2)
    out = torch.empty_like(psi)
    assert raw_apply(pkg, sharded, psi, good, out) == E.SD_EARG and raw_apply(pkg, sharded, host, good, np.empty_like(host)) == E.SD_EARG
    assert raw_bracket(pkg, sharded, psi, psi, good)[0] == E.SD_EARG
    # a model without device tables
    bare = pkg.XXZChain(L, nup=6, boundary="periodic", ctx=None, **XXZ)
    assert pkg.lib().sd_dcurrent_apply(m.ctx.h, bare.h, E.SD_C128, host.ctypes.data, m.N, good.ctypes.data, len(good),
                                       np.empty_like(host).ctypes.data) == E.SD_EARG
    still_usable()
