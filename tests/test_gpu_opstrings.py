"""Operator strings: sd_opstring_apply[_dev], sd_opstring_expect[_dev] and the Python layer (operators.py) against
tests/opstring_ref.py (proven on the CPU by tests/test_opstring_ref_host.py), against the library's own independent kernels, and
against dense exact diagonalisation.

The write form is compared bit for bit -- real and imaginary parts as IEEE doubles under == -- on ALL rows: the library is built
without contraction and the row form fixes every operation and its order.  Expectations differ from an exactly rounded sum
(math.fsum) of the same products only by the reduction tree: about 23 levels of 1.1e-16, hence the bar 1e-13 sum |bra[s] (O ket)[s]|
(the bar and the reason of tests/test_gpu_energy_current.py).  Ties to the library's other kernels sum the same terms in another
order; with T contributing terms of magnitudes a_t in a row, each side is within (T - 1) 2^-53 sum a_t of the exact row sum plus one
rounding per product, so the rows are compared to (T + 2) 2^-53 sum a_t.  Small shapes are those of
tests/test_gpu_pair_correlations.py, grid-wrap shapes those of tests/test_gpu_operator_grids.py; every shape asserts its
sd_model_path, so the three row modes (tile tables, rank walk, full basis) are all known to run."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

import opstring_ref as OR
from test_gpu_operator_grids import SPECS, Shape, assert_crosses_the_caps, fill_randn, nan_complex
from test_gpu_pair_correlations import SMALL, build

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
U = 2.0 ** -53
OPS_TILE_BLOCKS, OPS_ROW_BLOCKS, OPS_RED_BLOCKS = 4096, 8192, 2048      # the launchers' caps (kernels_opstring.hip)


def to_pkg(pkg, terms):
    return [pkg.Term(P, M, Z, complex(c), op) for P, M, Z, c, op in terms]


def hand_list(L, ls):
    """a diagonal group, a two-term group with different Z, the reversed pair, a four-site string that straddles the prefix / suffix
    cut (the plan's suffix holds `ls` sites, 12 by default), a string on sites (1, L), complex coefficients"""
    b = OR.bit
    far = b(L) if L >= 4 else 0
    tl = [(0, 0, b(1) | b(2), 0.7 + 0j, 0), (0, 0, b(L), -0.3 + 0j, 0), (0, 0, 0, 0.11 + 0j, 0)]            # diagonal, three terms
    if L >= 3:
        tl += [(b(2), b(3), b(1), 0.5 + 0j, 0), (b(2), b(3), far, -1.25 + 0j, 0),                             # one group, two Z
               (b(3), b(2), 0, 0.9 + 0j, 0)]                                                                  # the reversed pair
    if L >= 4:
        cut = min(max(L - (12 if ls is None else ls), 2), L - 2)              # sites cut-1, cut | cut+1, cut+2
        rest = [s for s in range(1, L + 1) if not cut - 1 <= s <= cut + 2]
        z = b(rest[0]) if rest else 0
        tl += [(b(cut - 1) | b(cut + 1), b(cut) | b(cut + 2), z, -0.6 + 0.2j, 0),
               (b(cut) | b(cut + 2), b(cut - 1) | b(cut + 1), z, -0.6 - 0.2j, 0)]
    tl += [(b(1), b(L), 0, 0.4 - 0.8j, 0), (b(L), b(1), 0, 0.4 + 0.8j, 0)]                                    # sites (1, L), complex
    return tl


def real_part_list(terms):
    return [t for t in terms if complex(t[3]).imag == 0.0]


def bits_equal(got, want):
    return bool(np.array_equal(got.real, want.real) and np.array_equal(got.imag, want.imag))


def nan_host(n, cplx=True):
    return np.full(n, np.nan + 1j * np.nan, dtype=np.complex128) if cplx else np.full(n, np.nan)


def nan_dev(n, dev, cplx=True):
    import torch
    return nan_complex(n, dev) if cplx else torch.full((n,), float("nan"), dtype=torch.float64, device=dev)


def check_write_form(pkg, m, L, nup, terms, psis_dev, s=None):
    """operator_apply on device and host vectors, Float64 and ComplexF64, NaN-filled outputs, against the restatement bit for bit;
    then the Float64 output of the real sublist"""
    import torch
    tp, rl = to_pkg(pkg, terms), real_part_list(terms)
    for psi in psis_dev:
        host = psi.cpu().numpy()
        want = OR.apply_rows(terms, host, L, nup, s=s)
        out = nan_dev(len(psi), psi.device)
        assert pkg.operator_apply(psi, m, tp, out=out) is out
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        bad = (got.real != want.real) | (got.imag != want.imag)
        assert not bad.any(), f"{int(bad.sum())} of {len(bad)} rows differ; first rows {np.nonzero(bad)[0][:8].tolist()}"
        hout = nan_host(len(host))
        pkg.operator_apply(host, m, tp, out=hout)
        assert bits_equal(hout, want)
        if not psi.is_complex():                              # a Float64 psi, real coefficients: a Float64 output
            wr = OR.apply_rows(rl, host, L, nup, s=s).real
            o2 = nan_dev(len(psi), psi.device, cplx=False)
            pkg.operator_apply(psi, m, to_pkg(pkg, rl), out=o2)
            assert np.array_equal(o2.cpu().numpy(), wr)
            assert pkg.operator_apply(host, m, to_pkg(pkg, rl)).dtype == np.float64
            assert np.array_equal(pkg.operator_apply(host, m, to_pkg(pkg, rl)), wr)


# ---- 1. the write form, all rows, bit for bit ----
@pytest.mark.parametrize("name", list(SMALL))
def test_write_form_small(pkg, name):
    L, nup, boundary, ls, path = SMALL[name]
    m = build(pkg, L, nup, boundary, ls)
    assert pkg.lib().sd_model_path(m.h) == path
    terms = hand_list(L, ls)
    assert len(OR.groups(terms)) >= (6 if L >= 4 else 3)
    psis = [fill_randn(pkg, m, m.N, False, 11 + L), fill_randn(pkg, m, m.N, True, 12 + L)]
    check_write_form(pkg, m, L, nup, terms, psis)


class Big:
    """the grid-wrap shapes, built once: the model, its vectors, the rows' configurations on the host, and the restatement's results"""

    def __init__(self, pkg):
        self.pkg, self.store = pkg, {}

    def get(self, name):
        if name not in self.store:
            sh = Shape(self.pkg, name)
            sh.s_host = sh.s.cpu().numpy().astype(np.uint64)
            sh.ls = SPECS[name][3]
            self.store[name] = sh
        return self.store[name]


@pytest.fixture(scope="module")
def big(pkg):
    import torch
    st = Big(pkg)
    yield st
    st.store.clear()
    gc.collect()
    torch.cuda.empty_cache()


def assert_wraps(sh):
    assert_crosses_the_caps(sh)
    if sh.path == 1:
        assert len(sh.tiles[0]) > OPS_TILE_BLOCKS
    else:
        assert (sh.N + 255) // 256 > OPS_ROW_BLOCKS


@pytest.mark.parametrize("name", ["Ts", "R-open", "F"])
def test_write_form_where_the_grid_wraps(pkg, big, name):
    import torch
    sh = big.get(name)
    assert_wraps(sh)
    m, L, nup = sh.m, sh.L, sh.nup
    terms = hand_list(L, sh.ls)
    tp = to_pkg(pkg, terms)
    for psi in (sh.psi_r, sh.psi_c):
        want = OR.apply_rows(terms, psi.cpu().numpy(), L, nup, s=sh.s_host)
        out = nan_complex(sh.N, sh.dev)
        pkg.operator_apply(psi, m, tp, out=out)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        bad = (got.real != want.real) | (got.imag != want.imag)
        assert not bad.any(), f"{name}: {int(bad.sum())} of {sh.N} rows differ; first rows {np.nonzero(bad)[0][:8].tolist()}"
        del out, got, want
    if name == "F":                                           # a sector-changing S^+_i against the one-site kernel
        for site in (1, 12, L):
            host = sh.psi_c.cpu().numpy()
            want = pkg.create_spin_operator(site, "plus")(host, m)
            out = nan_complex(sh.N, sh.dev)
            pkg.operator_apply(sh.psi_c, m, pkg.op_string(1.0, ("+", site)), out=out)
            assert bits_equal(out.cpu().numpy(), want), site
            del out, want


# ---- 2. the fused form ----
@pytest.mark.parametrize("name", ["L4n2-periodic", "L16n8-periodic", "L14n7-suffix8", "L13n1-per-row", "full-L10", "Ts"])
def test_fused_form(pkg, big, name):
    import torch
    if name in SMALL:
        L, nup, boundary, ls, path = SMALL[name]
        m = build(pkg, L, nup, boundary, ls)
        s = None
    else:
        sh = big.get(name)
        m, L, nup, ls, path, s = sh.m, sh.L, sh.nup, sh.ls, sh.path, sh.s_host
    assert pkg.lib().sd_model_path(m.h) == path
    terms = hand_list(L, ls)
    tp, b = to_pkg(pkg, terms), 0.3 - 1.7j
    for cplx in (False, True):
        psi = fill_randn(pkg, m, m.N, cplx, 21 + L)
        y = fill_randn(pkg, m, m.N, True, 22 + L)
        want = OR.fused(OR.apply_rows(terms, psi.cpu().numpy(), L, nup, s=s), y.cpu().numpy(), b)
        out = nan_complex(m.N, y.device)
        pkg.operator_apply(psi, m, tp, y=y, b=b, out=out)
        assert bits_equal(out.cpu().numpy(), want)
        hout = pkg.operator_apply(psi.cpu().numpy(), m, tp, y=y.cpu().numpy(), b=b)
        assert bits_equal(hout, want)
        yy = y.clone()
        assert pkg.operator_apply(psi, m, tp, y=yy, b=b, out=yy) is yy      # out = y: the same bits
        torch.cuda.synchronize()
        assert bits_equal(yy.cpu().numpy(), want)
    # Float64 throughout: real coefficients, real b
    rl = real_part_list(terms)
    psi, y = fill_randn(pkg, m, m.N, False, 23 + L), fill_randn(pkg, m, m.N, False, 24 + L)
    want = OR.fused(OR.apply_rows(rl, psi.cpu().numpy(), L, nup, s=s), y.cpu().numpy(), -0.75, real=True)
    out = nan_dev(m.N, y.device, cplx=False)
    pkg.operator_apply(psi, m, to_pkg(pkg, rl), y=y, b=-0.75, out=out)
    assert np.array_equal(out.cpu().numpy(), want)
    pkg.operator_apply(psi, m, to_pkg(pkg, rl), y=y, b=-0.75, out=y)
    assert np.array_equal(y.cpu().numpy(), want)
    # an empty list: out = b y
    yc = fill_randn(pkg, m, m.N, True, 25 + L)
    got = pkg.operator_apply(fill_randn(pkg, m, m.N, True, 26 + L), m, [], y=yc, b=b)
    assert bits_equal(got.cpu().numpy(), OR.fused(np.zeros(m.N, dtype=np.complex128), yc.cpu().numpy(), b))
    assert not pkg.operator_apply(psi, m, []).cpu().numpy().any()


# ---- 3. expectations ----
def many_operators(L, K, big_shape):
    """K operators; on the large shapes each is one six-site group of two terms (1/64 of a full basis' rows contribute: the
    restatement's exactly rounded sums are what takes the time there), on the small ones a four-site group, a diagonal group and a hop"""
    b = OR.bit
    tl = []
    for k in range(K):
        n = 6 if big_shape else 4
        if L >= n:
            a = [(k + d) % L + 1 for d in range(n)] if k % 2 else [(3 * k + d * (L // n)) % L + 1 for d in range(n)]
            assert len(set(a)) == n
            rest = [s for s in range(1, L + 1) if s not in a]
            z = b(rest[k % len(rest)]) if rest else 0
            P, M = sum(b(x) for x in a[0::2]), sum(b(x) for x in a[1::2])
            tl += [(P, M, 0, complex(0.3 + 0.1 * k, 0.2 - 0.05 * k), k), (P, M, z, complex(-0.4, 0.1 * k), k)]
        if not big_shape:
            i, j = k % L + 1, (k + 1) % L + 1
            tl += [(0, 0, b(i), complex(0.1 * (k + 1), 0.0), k), (0, 0, b(i) | b(j), complex(0.0, 0.3), k)]
            if i != j:
                tl += [(b(i), b(j), 0, complex(0.5, -0.1 * k), k)]
    return tl


def check_expectations(pkg, m, L, nup, bra, ket, s, big_shape):
    full = many_operators(L, 17, big_shape)
    hb, hk = bra.cpu().numpy(), ket.cpu().numpy()
    ref, ref_self = OR.expectations(full, [hb, hk], hk, L, nup, s=s)
    for K in (1, 9, 17):
        tp = to_pkg(pkg, [t for t in full if t[4] < K])
        got = pkg.operator_expectations(ket, m, tp, bra=bra)
        assert len(got) == K
        for k in range(K):
            val, scale = ref[k]
            assert scale > 0 or L < 4
            assert abs(got[k] - val) <= 1e-13 * scale, (K, k, got[k], val, scale)
        again = pkg.operator_expectations(ket, m, tp, bra=bra)
        assert bits_equal(again, got)                                                       # equal bits on a repeated call
        own = pkg.operator_expectations(ket, m, tp)
        assert bits_equal(own, pkg.operator_expectations(ket, m, tp, bra=ket))              # bra NULL is bra = ket
        for k in range(K):
            assert abs(own[k] - ref_self[k][0]) <= 1e-13 * ref_self[k][1]
        if not big_shape:
            assert bits_equal(pkg.operator_expectations(hk, m, tp, bra=hb), got)            # host input
    # Hermitian operators, O + O^+ of operators of the list (all 17 on the small shapes, the first 3 on the large ones, where the
    # restatement is what takes the time): the imaginary part is rounding
    part = [t for t in full if t[4] < (3 if big_shape else 17)]
    herm = part + OR.adjoint(part)
    hv = pkg.operator_expectations(ket, m, to_pkg(pkg, herm))
    href = OR.expectations(herm, hk, hk, L, nup, s=s)
    assert len(hv) == len(href) == (3 if big_shape else 17)
    for k in range(len(hv)):
        assert abs(hv[k].imag) <= 1e-13 * href[k][1] and abs(hv[k] - href[k][0]) <= 1e-13 * href[k][1]


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("name", list(SMALL))
def test_expectations_small(pkg, name, cplx):
    L, nup, boundary, ls, path = SMALL[name]
    m = build(pkg, L, nup, boundary, ls)
    assert pkg.lib().sd_model_path(m.h) == path
    bra, ket = fill_randn(pkg, m, m.N, cplx, 31 + L), fill_randn(pkg, m, m.N, cplx, 32 + L)
    check_expectations(pkg, m, L, nup, bra, ket, None, False)


@pytest.mark.parametrize("name", ["Ts", "F"])
def test_expectations_where_the_grid_wraps(pkg, big, name):
    sh = big.get(name)
    assert_wraps(sh)
    assert (len(sh.tiles[0]) if sh.path == 1 else (sh.N + 255) // 256) > OPS_RED_BLOCKS
    check_expectations(pkg, sh.m, sh.L, sh.nup, sh.bra_c(pkg), sh.psi_c, sh.s_host, True)


# ---- 4. ties to independent kernels of the library ----
TIES = ["L12n6-periodic", "L16n3-open", "J1J2-L14n7", "L14n7-suffix8", "L13n1-per-row", "full-L10"]


def assert_rows_within(got, want, terms, host, L, nup, what):
    """|got - want| per row against (T + 2) 2^-53 sum |terms of that row|"""
    _o, cnt, mag = OR.apply_rows(terms, host, L, nup, contributions=True)
    bar = (cnt + 2) * U * mag
    d = np.abs(got - want)
    assert (d <= bar).all(), (what, int((d > bar).sum()), float((d / np.maximum(bar, 1e-300)).max()))
    assert mag.max() > 0


@pytest.mark.parametrize("name", TIES)
def test_tie_to_apply_H(pkg, name):
    import torch
    L, nup, boundary, ls, path = SMALL[name]
    m = build(pkg, L, nup, boundary, ls)
    terms = pkg.hamiltonian_terms(m)
    ref_terms = OR.hamiltonian_terms(m.hopping_list, m.zz_list, m.onsite_field)
    for cplx in (False, True):
        psi = fill_randn(pkg, m, m.N, cplx, 41 + L)
        want = torch.empty_like(psi)
        pkg.apply_H(want, psi, m)
        got = pkg.operator_apply(psi, m, terms)
        assert got.dtype == psi.dtype                                       # a real list on a real vector stays real
        assert_rows_within(got.cpu().numpy(), want.cpu().numpy(), ref_terms, psi.cpu().numpy(), L, nup, name)


@pytest.mark.parametrize("name", TIES)
def test_tie_to_energy_current_and_bond_operator(pkg, name):
    L, nup, boundary, ls, path = SMALL[name]
    m = build(pkg, L, nup, boundary, ls)
    psi = fill_randn(pkg, m, m.N, True, 51 + L)
    host = psi.cpu().numpy()
    dterms = pkg.energy_current_terms(m, "open")
    assert len(dterms) > 0
    strings = OR.from_ecurrent(dterms)
    got = pkg.operator_apply(psi, m, to_pkg(pkg, strings))
    assert_rows_within(got.cpu().numpy(), pkg.energy_current(psi, m, dterms).cpu().numpy(), strings, host, L, nup, name)
    for (i, j, xy, zz) in [(1, 2, 1.0, 1.0), (L, 3, 0.7, -1.1)]:
        bs = OR.from_bond(i, j, xy, zz)
        got = pkg.operator_apply(psi, m, to_pkg(pkg, bs))
        assert_rows_within(got.cpu().numpy(), pkg.bond_operator(psi, m, i, j, xy, zz).cpu().numpy(), bs, host, L, nup, (name, i, j))


@pytest.mark.parametrize("name", TIES)
def test_tie_to_correlation_matrix(pkg, name):
    """<S^z_i S^z_j> and <S^+_i S^-_j> as K strings in one pass against the pair kernel: both sums are within 1e-13 sum |products| of
    the exact sum (the bar of the expectations), so they agree to twice that"""
    L, nup, boundary, ls, path = SMALL[name]
    m = build(pkg, L, nup, boundary, ls)
    psi = fill_randn(pkg, m, m.N, True, 61 + L)
    host = psi.cpu().numpy()
    pairs = [(i, j) for i in range(1, L + 1) for j in range(1, L + 1) if i != j][:120]
    zz = [(0, 0, OR.bit(i) | OR.bit(j), 1.0 + 0j, k) for k, (i, j) in enumerate(pairs)]
    pm = [(OR.bit(i), OR.bit(j), 0, 1.0 + 0j, k) for k, (i, j) in enumerate(pairs)]
    Z, G = pkg.correlation_matrix(psi, m, "zz"), pkg.correlation_matrix(psi, m, "+-")
    for tl, M in ((zz, Z), (pm, G)):
        got = pkg.operator_expectations(psi, m, to_pkg(pkg, tl))
        ref = OR.expectations(tl, host, host, L, nup)
        for k, (i, j) in enumerate(pairs):
            assert abs(got[k] - M[i - 1, j - 1]) <= 2e-13 * ref[k][1], (name, i, j)
            assert abs(got[k] - ref[k][0]) <= 1e-13 * ref[k][1]


# ---- 5. physics ----
def kron_site(D, op, site, L):
    """op on 1-based `site` as a sparse Kronecker chain over the full 2^L space (site 1 is the rightmost factor, as oracle/dense.py's
    site_op, whose dense products take minutes at L = 12)"""
    import scipy.sparse as sp
    out = sp.identity(1, format="csr", dtype=np.complex128)
    for s in range(L, 0, -1):
        out = sp.kron(out, sp.csr_matrix((op if s == site else D.I2).astype(np.complex128)), format="csr")
    return out


def test_chiral_hamiltonian_against_dense_ed(pkg, D):
    """J1-J2 ring with J_chi sum_i S_i . (S_i+1 x S_i+2) at L = 12, nup = 6 through operator_hamiltonian: the ground-state energy and the
    chirality against dense eigh of the Kronecker operators.  Bar: 1e-10 max|E|, the bar of lowest_level against dense ED in
    tests/test_gpu_symmetry.py (its other branch, ten times the error of a plain call, is smaller at this shape); the chirality is
    bounded by 3/8 per triangle, below max|E|, so the same bar holds for it.  J2 = 0.5, J_chi = 1.5: below J_chi of about 1 the ring's
    ground state is the non-chiral singlet of J_chi = 0; here the chiral level lies 0.43 below the next one."""
    L, nup, J2, Jchi = 12, 6, 0.5, 1.5
    site = lambda i: (i - 1) % L + 1          # noqa: E731
    hop = [(i, site(i + 1), 0.5) for i in range(1, L + 1)] + [(i, site(i + 2), J2 / 2) for i in range(1, L + 1)]
    zz = [(i, site(i + 1), 1.0) for i in range(1, L + 1)] + [(i, site(i + 2), J2) for i in range(1, L + 1)]
    triples = [(i, site(i + 1), site(i + 2)) for i in range(1, L + 1)]
    m = pkg.build_model(L, nup=nup, hopping=hop, zz=zz, onsite_field=np.zeros(L))
    one = {"x": 0.5 * (D.SP + D.SM), "y": (D.SP - D.SM) / 2j, "z": D.SZ, "+": D.SP, "-": D.SM}
    S = {(k, i): kron_site(D, one[k], i, L) for k in one for i in range(1, L + 1)}
    st = D.sector_states(L, nup).astype(np.int64)
    sector = lambda A: A[st][:, st].toarray()          # noqa: E731
    chis = []
    for (i, j, k) in triples:
        A = 0
        for perm, sign in OR.EPS:
            a, b, c = ("xyz"[q] for q in perm)
            A = A + sign * (S[(a, i)] @ S[(b, j)] @ S[(c, k)])
        chis.append(A)
    chi = sector(sum(chis[1:], chis[0]))
    assert np.abs(chi - chi.conj().T).max() <= 1e-14
    H0 = 0
    for i, j, t in hop:
        H0 = H0 + t * (S[("+", i)] @ S[("-", j)] + S[("-", i)] @ S[("+", j)])
    for i, j, v_ in zz:
        H0 = H0 + v_ * (S[("z", i)] @ S[("z", j)])
    H0 = sector(H0)
    w, v = np.linalg.eigh(H0 + Jchi * chi)
    assert w[1] - w[0] > 0.05                                                # a unique ground state: its chirality is defined
    bar = 1e-10 * np.abs(w).max()
    terms = []
    for t in triples:
        terms += pkg.chirality_terms(*t, coeff=Jchi)
    terms = pkg.operator_simplify(terms)
    E0, psi = pkg.operator_groundstate(m, terms)
    want_chi = np.vdot(v[:, 0], chi @ v[:, 0]).real
    got_chi = pkg.scalar_chirality(psi, m, triples)
    print(f"E0 = {E0:.12f} (dense {w[0]:.12f}), sum chi = {got_chi.sum():.12f} (dense {want_chi:.12f}), bar {bar:.2e}")
    assert abs(E0 - w[0]) <= bar
    assert abs(got_chi.sum() - want_chi) <= bar and abs(want_chi) > 0.1
    assert np.abs(got_chi - got_chi.mean()).max() <= bar                     # translation invariant: every triangle alike
    # lanczos_extremal through the solvers' applyH= argument sees the same lowest level
    lo, _hi = pkg.lanczos_extremal(pkg.operator_hamiltonian(m, terms), m, lanc_m=200)
    assert abs(lo - w[0]) <= bar
    # J_chi = 0: a real ground state has no chirality
    E00, psi0 = pkg.operator_groundstate(m, [])
    assert psi0.dtype == np.float64 and abs(E00 - np.linalg.eigvalsh(H0)[0]) <= bar
    assert np.abs(pkg.scalar_chirality(psi0, m, triples)).max() <= 1e-12
    # chirality correlations of disjoint triangles against the dense product
    far = [b for b in range(1, L) if not set(triples[0]) & set(triples[b])]
    Cm = pkg.chirality_correlations(psi, m, triples, pairs=[(0, b) for b in far])
    for b in far:
        want = np.vdot(v[:, 0], sector(chis[0] @ chis[b]) @ v[:, 0]).real
        assert abs(Cm[0, b] - want) <= bar and Cm[b, 0] == Cm[0, b]
    assert np.isnan(Cm[0, 0]) and np.isnan(Cm[1, 2])
    with pytest.raises(pkg.ArgumentError):
        pkg.chirality_correlations(psi, m, triples)                          # neighbouring triangles share sites


@pytest.mark.parametrize("name", ["L12n6-periodic", "L13n1-per-row", "full-L10"])
def test_string_order_and_multi_spin_expectations(pkg, name):
    L, nup, boundary, ls, path = SMALL[name]
    m = build(pkg, L, nup, boundary, ls)
    psi = fill_randn(pkg, m, m.N, True, 71 + L)
    host = psi.cpu().numpy()
    Z = pkg.correlation_matrix(psi, m, "zz")
    n2 = float(np.vdot(host, host).real)
    for i in (1, 5, L - 1):
        got = pkg.string_order(psi, m, i, i + 1)                             # no site in between: -<S^z_i S^z_i+1>
        assert abs(got + Z[i - 1, i]) <= 2e-13 * 0.25 * n2 and got.imag == 0.0
    for (i, j) in ((1, 4), (2, L), (3, 8)):
        (val, scale), = OR.expectations(OR.string_order(i, j), host, host, L, nup)
        assert abs(pkg.string_order(psi, m, i, j) - val) <= 1e-13 * scale
        assert pkg.string_order(host, m, i, j) == pkg.string_order(psi, m, i, j)
    strings = [(1.0, ("z", 1), ("z", 2), ("+", 3), ("-", 4)), (0.5 - 1j, ("z", L)), (2.0, ("+", 2), ("-", 7), ("+", 5), ("-", 1), ("z", 3), ("z", 9))]
    got = pkg.multi_spin_expectation(psi, m, strings)
    ref = []
    for k, sdef in enumerate(strings):
        ref += OR.expand(sdef[0], list(sdef[1:]), op=k)
    for k, (val, scale) in enumerate(OR.expectations(ref, host, host, L, nup)):
        assert abs(got[k] - val) <= 1e-13 * scale


# ---- 6. every refusal; the context stays usable ----
def test_refusals(pkg):
    import torch
    lib, EARG, EDIM, F64, C128 = pkg.lib(), pkg._lib.SD_EARG, pkg._lib.SD_EDIM, pkg._lib.SD_F64, pkg._lib.SD_C128
    T = pkg.Term
    m = build(pkg, 12, 6, "periodic", None)
    full = build(pkg, 10, None, "periodic", None)
    psi, out = fill_randn(pkg, m, m.N, True, 81), nan_complex(m.N, torch.device("cuda", m.ctx.device))
    psi_r = fill_randn(pkg, m, m.N, False, 82)
    good = pkg.pack_terms(to_pkg(pkg, hand_list(12, None)))
    m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    res = np.zeros(2 * 256)

    def apply_rc(model, dtype, p, n, tl, y, b, dtype_out, o):
        tl = pkg.pack_terms(tl)
        return lib.sd_opstring_apply_dev(model.ctx.h, model.h, dtype, p, n, tl.ctypes.data, len(tl), y, b.real, b.imag, dtype_out, o)

    def expect_rc(model, dtype, bra, ket, n, tl, n_terms=None):
        tl = pkg.pack_terms(tl)
        return lib.sd_opstring_expect_dev(model.ctx.h, model.h, dtype, bra, ket, n, tl.ctypes.data, len(tl) if n_terms is None else n_terms,
                                          res.ctypes.data_as(_dp))

    def usable():
        o = pkg.operator_apply(psi, m, good)
        want = OR.apply_rows(hand_list(12, None), psi.cpu().numpy(), 12, 6)
        assert bits_equal(o.cpu().numpy(), want)

    P, O = psi.data_ptr(), out.data_ptr()
    bad_lists = {
        "overlapping masks": [T(3, 2, 0, 1 + 0j, 0)],
        "plus and z overlap": [T(1, 2, 1, 1 + 0j, 0)],
        "a bit at L": [T(1, 1 << 12, 0, 1 + 0j, 0)],
        "|P| != |M| in a sector": [T(1, 0, 0, 1 + 0j, 0)],
        "non-finite coefficient": [T(1, 2, 0, complex(np.nan, 0), 0)],
        "negative op": [T(1, 2, 0, 1 + 0j, -1)],
        "op too large": [T(1, 2, 0, 1 + 0j, 256)],
    }
    for why, tl in bad_lists.items():
        assert apply_rc(m, C128, P, m.N, tl, None, 0j, C128, O) == EARG, why
        assert expect_rc(m, C128, None, P, m.N, tl) == EARG, why
        assert pkg.lib().sd_last_error(m.ctx.h)
        with pytest.raises(pkg.ArgumentError):
            pkg.operator_apply(psi, m, tl)
        with pytest.raises(pkg.ArgumentError):
            pkg.operator_expectations(psi, m, tl)
        usable()
    # the number of terms
    assert expect_rc(m, C128, None, P, m.N, good, n_terms=-1) == EARG
    assert expect_rc(m, C128, None, P, m.N, [T(0, 0, 1, 1 + 0j, 0)] * 4097) == EARG
    assert apply_rc(m, C128, P, m.N, [T(0, 0, 1, 1 + 0j, 0)] * 4097, None, 0j, C128, O) == EARG
    # op != 0 in the write form (fine for the expectations)
    assert apply_rc(m, C128, P, m.N, [T(1, 2, 0, 1 + 0j, 1)], None, 0j, C128, O) == EARG
    assert expect_rc(m, C128, None, P, m.N, [T(1, 2, 0, 1 + 0j, 1)]) == 0
    # a Float64 output with an imaginary coefficient, an imaginary b, a ComplexF64 psi
    R = psi_r.data_ptr()
    assert apply_rc(m, F64, R, m.N, [T(1, 2, 0, 1j, 0)], None, 0j, F64, O) == EARG
    assert apply_rc(m, F64, R, m.N, [T(1, 2, 0, 1 + 0j, 0)], O, 1j, F64, O) == EARG
    assert apply_rc(m, C128, P, m.N, [T(1, 2, 0, 1 + 0j, 0)], None, 0j, F64, O) == EARG
    assert apply_rc(m, F64, R, m.N, [T(1, 2, 0, 1 + 0j, 0)], None, 0j, F64, O) == 0
    with pytest.raises(pkg.ArgumentError):
        pkg.operator_apply(psi_r, m, [T(1, 2, 0, 1j, 0)], out=torch.empty_like(psi_r))
    # a non-finite b
    assert apply_rc(m, C128, P, m.N, good, O, complex(np.inf, 0), C128, O) == EARG
    # bad dtypes
    assert apply_rc(m, 3, P, m.N, good, None, 0j, C128, O) == EARG
    assert apply_rc(m, C128, P, m.N, good, None, 0j, 0, O) == EARG
    assert expect_rc(m, 7, None, P, m.N, good) == EARG
    # NULL vectors
    assert apply_rc(m, C128, None, m.N, good, None, 0j, C128, O) == EARG
    assert apply_rc(m, C128, P, m.N, good, None, 0j, C128, None) == EARG
    assert expect_rc(m, C128, None, None, m.N, good) == EARG
    # aliasing: identity, partial overlap with psi, partial overlap with y
    assert apply_rc(m, C128, P, m.N, good, None, 0j, C128, P) == EARG
    both = torch.zeros(2 * m.N, dtype=torch.complex128, device=psi.device)
    B = both.data_ptr()
    assert apply_rc(m, C128, B, m.N, good, None, 0j, C128, B + 16 * (m.N - 1)) == EARG
    assert apply_rc(m, C128, B + 16 * 5, m.N, good, None, 0j, C128, B) == EARG
    assert apply_rc(m, C128, P, m.N, good, B + 16, 1 + 0j, C128, B) == EARG
    assert apply_rc(m, C128, P, m.N, good, B, 1 + 0j, C128, B) == 0
    with pytest.raises(pkg.ArgumentError):
        pkg.operator_apply(psi, m, good, out=psi)
    # the dimension
    assert apply_rc(m, C128, P, m.N - 1, good, None, 0j, C128, O) == EDIM
    assert expect_rc(m, C128, None, P, m.N + 1, good) == EDIM
    with pytest.raises(pkg.DimensionMismatch):
        pkg.operator_expectations(psi[:-1].contiguous(), m, good)
    usable()
    # a sharded model, and a model without device tables
    sharded = build(pkg, 14, 7, "periodic", 8)
    sharded.set_shard(0, 2)
    v = torch.zeros(int(sharded.shard_info().n_local), dtype=torch.complex128, device=psi.device)
    assert apply_rc(sharded, C128, v.data_ptr(), len(v), good, None, 0j, C128, O) == EARG
    assert expect_rc(sharded, C128, None, v.data_ptr(), len(v), good) == EARG
    hostonly = pkg.XXZChain(12, nup=6, ctx=None)
    tl = pkg.pack_terms(good)
    assert lib.sd_opstring_apply_dev(m.ctx.h, hostonly.h, C128, P, m.N, tl.ctypes.data, len(tl), None, 0.0, 0.0, C128, O) == EARG
    assert lib.sd_opstring_expect_dev(m.ctx.h, hostonly.h, C128, None, P, m.N, tl.ctypes.data, len(tl), res.ctypes.data_as(_dp)) == EARG
    usable()
    # a sector-changing term is fine on the full basis
    pf = fill_randn(pkg, full, full.N, True, 83)
    assert pkg.operator_apply(pf, full, [T(1, 0, 0, 1 + 0j, 0)]).shape == (full.N,)
    # empty lists: a zero vector, K = 0
    assert not pkg.operator_apply(psi, m, []).cpu().numpy().any()
    assert len(pkg.operator_expectations(psi, m, [])) == 0
    # a non-Hermitian list is no Hamiltonian
    with pytest.raises(pkg.ArgumentError):
        pkg.operator_hamiltonian(m, pkg.op_string(1.0, ("+", 1), ("-", 2)))
    with pytest.raises(pkg.ArgumentError):
        pkg.operator_hamiltonian(m, pkg.op_string(1.0, ("z", 1), op=1))
    assert callable(pkg.operator_hamiltonian(m, pkg.op_string(1.0, ("+", 1), ("-", 2)) + pkg.op_string(1.0, ("-", 1), ("+", 2))))
    usable()


def test_one_row_sector(pkg):
    """nup = 0: a sector of one row, where only the diagonal groups contribute"""
    m = pkg.XXZChain(6, nup=0, boundary="open")
    assert m.N == 1
    psi = np.array([2.0 - 1.0j])
    got = pkg.operator_apply(psi, m, hand_list_pkg(pkg, 6))
    assert bits_equal(got, OR.apply_rows(hand_list(6, None), psi, 6, 0))
    vals = pkg.operator_expectations(psi, m, hand_list_pkg(pkg, 6))
    (val, scale), = OR.expectations(hand_list(6, None), psi, psi, 6, 0)
    assert abs(vals[0] - val) <= 1e-13 * scale


def hand_list_pkg(pkg, L):
    return to_pkg(pkg, hand_list(L, None))
