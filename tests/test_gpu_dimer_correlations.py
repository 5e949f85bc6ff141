"""Bond operators and dimer correlations: sd_bond_apply[_dev], sd_dimer_correlations[_dev] and the Python mirror
(bond_operator, dimer_correlation_matrix, bond_energies, dimer_structure_factor) against tests/dimer_ref.py (proven on the CPU by
tests/test_dimer_ref_host.py), against exact states, against the solver on the Majumdar-Ghosh chain, and against the library's own
independent kernels.

Tolerance of every comparison with dimer_ref: elementwise |D_dev - D_ref| <= 1e-12 <psi|psi> with |xy|, |zz| <= 1.  Each entry is a
sum of at most N products bounded by |psi|^2 (|(D_b psi)(s)| <= max(|psi(s)|, |psi(s')|) for such weights) and the blocked sums
are accurate to a few tens of eps at these N: the argument of tests/test_gpu_pair_correlations.py.

bond_operator is one multiply, and one multiply and one add, per component and row, in the order dimer_ref.bond_rows states
them; the library is built without contraction, so the comparison is bit for bit.

The kernels take the rows' configurations from the tile plan (sd_model_path 1), from unrank (path 0, fixed-nup sector) or from the
row index (full basis) and find partner rows by the plan's tables, by the local rank walk in either orientation, or by an
exclusive or: every shape asserts its path.  The grid-wrap shapes are those of tests/test_gpu_operator_grids.py.

The conjugation check: Im D_ab = <[D_a, D_b]> / 2i vanishes unless the two bonds share a site, and for a random vector it is of the
order of <psi|psi> / sqrt(N), not of <psi|psi>: measured with dimer_ref on the vectors used here, on the pair (2, 3), (3, 4) alone it
is 4e-3 <psi|psi> at N = 924 but 2e-4 at N = 12870 (L16n8), and with xy-only weights below 1e-3 even as the largest entry there.
So the bar 1e-3 <psi|psi> is asserted on the largest imaginary part of the matrix of the hand list, which holds the overlapping
bonds, for the weights (1, 1) and (0.8, 0.7) (2e-3 at L16n8); the entry of the overlapping pair itself must be far from rounding
and is compared with dimer_ref like every other entry.

The model's own bond list of the J1-J2 lists at L = 14 has 28 bonds (14 first and 14 second neighbours, 7 chunks of 4); the
raggedness test runs it whole and cut to its first 24 (6 full chunks)."""
import ctypes as C
import gc

import numpy as np
import pytest

import dimer_ref as DR
from test_gpu_operator_grids import XXZ, Shape, assert_crosses_the_caps, fill_randn
from test_gpu_pair_correlations import SMALL, build, norm2

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
DIMER_MAX_BLOCKS = 2048       # SD_DIMER_MAX_BLOCKS of kernels_dimer.hip: row blocks of the launch (tiles, or blocks of 256 rows)
DIMER_MAX_BONDS = 128         # SD_DIMER_MAX_BONDS of include/spindyn.h
WEIGHTS = [(1.0, 1.0), (0.8, 0.7), (1.0, 0.0), (0.0, 1.0)]


def hand_list(L):
    """B = 5, a ragged tile: the closing bond (L, 1), a reversed bond, the same bond again, a bond overlapping it, a bond longer than
    4 sites (L >= 6; the longest there is below that) -> (bonds, (a, b) of the overlapping pair).  L = 2 has one bond."""
    if L == 2:
        return [(1, 2)], None
    far = (1, 6) if L >= 6 else (1, L - 1)
    return [(L, 1), (3, 2), (2, 3), (3, 4), far], (2, 3)


def raw_dimer(pkg, m, psi, bonds, xy=1.0, zz=1.0, n=None, dtype=None, B=None):
    """status, the (B, B) complex matrix and e of sd_dimer_correlations[_dev] called directly"""
    import torch
    flat = np.ascontiguousarray(np.array(bonds, dtype=np.intc).reshape(-1))
    nb = len(bonds)
    D = np.full((max(nb, 1), max(nb, 1)), np.nan + 1j * np.nan, dtype=np.complex128)
    e = np.full(max(nb, 1), np.nan)
    n = len(psi) if n is None else n
    B = nb if B is None else B
    args = (flat.ctypes.data_as(_ip), B, xy, zz, D.ctypes.data_as(_dp), e.ctypes.data_as(_dp))
    if isinstance(psi, torch.Tensor):
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        code = (pkg._lib.SD_C128 if psi.is_complex() else pkg._lib.SD_F64) if dtype is None else dtype
        rc = pkg.lib().sd_dimer_correlations_dev(m.ctx.h, m.h, code, psi.data_ptr(), n, *args)
    else:
        code = (pkg._lib.SD_C128 if np.iscomplexobj(psi) else pkg._lib.SD_F64) if dtype is None else dtype
        rc = pkg.lib().sd_dimer_correlations(m.ctx.h, m.h, code, psi.ctypes.data, n, *args)
    return rc, D, e


def raw_bond(pkg, m, psi, i, j, out, xy=1.0, zz=1.0, n=None, dtype=None):
    """status of sd_bond_apply[_dev] called directly; the caller owns `out`"""
    import torch
    n = len(psi) if n is None else n
    if isinstance(psi, torch.Tensor):
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        code = (pkg._lib.SD_C128 if psi.is_complex() else pkg._lib.SD_F64) if dtype is None else dtype
        return pkg.lib().sd_bond_apply_dev(m.ctx.h, m.h, code, psi.data_ptr(), n, i, j, xy, zz, out.data_ptr())
    code = (pkg._lib.SD_C128 if np.iscomplexobj(psi) else pkg._lib.SD_F64) if dtype is None else dtype
    return pkg.lib().sd_bond_apply(m.ctx.h, m.h, code, psi.ctypes.data, n, i, j, xy, zz, out.ctypes.data)


def check_matrix(D, e, B, cplx):
    assert D.shape == (B, B) and D.dtype == (np.complex128 if cplx else np.float64)
    assert e.shape == (B,) and e.dtype == np.float64
    assert np.array_equal(D, D.conj().T)                      # Hermitian to the bit: one triangle is summed
    assert np.all(np.diagonal(D).imag == 0.0)
    if not cplx:
        assert np.all(D.imag == 0.0)


def equal_bits(x, y):
    import torch
    if x.is_complex():
        return torch.equal(torch.view_as_real(x), torch.view_as_real(y))
    return torch.equal(x, y)


# ---- 1. small shapes: every pair, every row ----
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("name", list(SMALL))
def test_all_pairs_small(pkg, name, cplx):
    import torch
    L, nup, boundary, ls, path = SMALL[name]
    m = build(pkg, L, nup, boundary, ls)
    assert pkg.lib().sd_model_path(m.h) == path
    psi = fill_randn(pkg, m, m.N, cplx, 5151 + 7 * L + (nup or 0))
    n2 = norm2(psi)
    host = psi.cpu().numpy()
    s = DR.configurations(m.N, L, nup, psi.device)
    own = pkg.model_bonds(m)
    hand, over = hand_list(L)
    for bonds in (own, hand):
        B = len(bonds)
        for xy, zz in WEIGHTS:
            refD, refe = DR.gram(psi, L, nup, bonds, xy, zz, s=s)
            for x in (psi, host):
                D = pkg.dimer_correlation_matrix(x, m, None if bonds is own else bonds, xy=xy, zz=zz)
                e = pkg.bond_energies(x, m, None if bonds is own else bonds, xy=xy, zz=zz)
                check_matrix(D, e, B, cplx)
                err, erre = np.abs(D - refD).max(), np.abs(e - refe).max()
                print(f"{name} B={B} xy={xy} zz={zz} {'dev' if x is psi else 'host'}: D {err:.2e} e {erre:.2e} (bar {1e-12 * n2:.2e})")
                assert err <= 1e-12 * n2 and erre <= 1e-12 * n2
            if cplx and bonds is hand and over is not None and (xy, zz) in WEIGHTS[:2]:
                im = abs(refD[over].imag)
                print(f"{name} xy={xy} zz={zz}: |Im D| on the overlapping pair {im / n2:.3e}, largest {np.abs(D.imag).max() / n2:.3e} <psi|psi>")
                assert np.abs(D.imag).max() > 1e-3 * n2 and abs(D[over].imag) > 1e-13 * n2      # the conjugation is exercised
    # the bond operator on all rows, both orientations, device and host: equal bits
    for (i, j) in hand:
        for xy, zz in WEIGHTS[:2]:
            want = DR.bond_rows(psi, s, L, nup, i, j, xy, zz)
            for a, b in ((i, j), (j, i)):
                got = pkg.bond_operator(psi, m, a, b, xy=xy, zz=zz)
                assert got.dtype == psi.dtype and got.shape == psi.shape and equal_bits(got, want), (name, a, b, xy, zz)
                goth = pkg.bond_operator(host, m, a, b, xy=xy, zz=zz)
                assert goth.dtype == host.dtype and np.array_equal(goth, want.cpu().numpy()), (name, a, b, xy, zz)
    out = torch.full_like(psi, float("nan"))
    assert pkg.bond_operator(psi, m, hand[0][0], hand[0][1], out=out) is out
    assert equal_bits(out, DR.bond_rows(psi, s, L, nup, hand[0][0], hand[0][1], 1.0, 1.0))
    # connected=True subtracts e_a e_b
    Dc = pkg.dimer_correlation_matrix(psi, m, hand, connected=True, xy=0.8, zz=0.7)
    D, e = pkg.dimer_correlation_matrix(psi, m, hand, xy=0.8, zz=0.7), pkg.bond_energies(psi, m, hand, xy=0.8, zz=0.7)
    assert np.array_equal(Dc, D - np.outer(e, e))


# ---- 2. tile raggedness ----
@pytest.mark.parametrize("B", [1, 4, 5, 8, 9])
def test_ragged_bond_counts(pkg, B):
    L, nup = 12, 6
    m = build(pkg, L, nup, "periodic", None)
    bonds = pkg.model_bonds(m)[:B]
    assert len(bonds) == B
    for cplx in (False, True):
        psi = fill_randn(pkg, m, m.N, cplx, 77 + B)
        n2 = norm2(psi)
        refD, refe = DR.gram(psi, L, nup, bonds, 0.8, 0.7)
        D, e = pkg.dimer_correlation_matrix(psi, m, bonds, xy=0.8, zz=0.7), pkg.bond_energies(psi, m, bonds, xy=0.8, zz=0.7)
        check_matrix(D, e, B, cplx)
        assert np.abs(D - refD).max() <= 1e-12 * n2 and np.abs(e - refe).max() <= 1e-12 * n2


@pytest.mark.parametrize("B", [24, 28])
def test_the_j1j2_bond_list(pkg, B):
    L, nup, boundary, ls, path = SMALL["J1J2-L14n7"]
    m = build(pkg, L, nup, boundary, ls)
    own = pkg.model_bonds(m)
    assert len(own) == 28 and len(m.hopping_list) == 28
    bonds = None if B == 28 else own[:B]
    psi = fill_randn(pkg, m, m.N, True, 1400 + B)
    n2 = norm2(psi)
    refD, refe = DR.gram(psi, L, nup, own[:B], 0.8, 0.7)
    D, e = pkg.dimer_correlation_matrix(psi, m, bonds, xy=0.8, zz=0.7), pkg.bond_energies(psi, m, bonds, xy=0.8, zz=0.7)
    check_matrix(D, e, B, True)
    assert np.abs(D - refD).max() <= 1e-12 * n2 and np.abs(e - refe).max() <= 1e-12 * n2
    assert np.abs(D.imag).max() > 1e-3 * n2


def test_the_largest_bond_list(pkg):
    """B = 128 seeded random bonds at L = 16, nup = 8: a seeded sample of 64 entries plus the whole diagonal, and all of e"""
    L, nup, B = 16, 8, DIMER_MAX_BONDS
    m = build(pkg, L, nup, "periodic", None)
    rng = np.random.default_rng(128)
    bonds = []
    while len(bonds) < B:
        i, j = (int(x) for x in rng.integers(1, L + 1, 2))
        if i != j:
            bonds.append((i, j))
    psi = fill_randn(pkg, m, m.N, True, 128)
    n2 = norm2(psi)
    pairs = [(int(a), int(b)) for a, b in rng.integers(0, B, (64, 2))] + [(a, a) for a in range(B)]
    ref, refe = DR.gram(psi, L, nup, bonds, 0.8, 0.7, pairs=pairs)
    D, e = pkg.dimer_correlation_matrix(psi, m, bonds, xy=0.8, zz=0.7), pkg.bond_energies(psi, m, bonds, xy=0.8, zz=0.7)
    check_matrix(D, e, B, True)
    err = max(abs(D[p] - v) for p, v in ref.items())
    print(f"B = 128: {err:.2e}, e {np.abs(e - refe).max():.2e} (bar {1e-12 * n2:.2e})")
    assert err <= 1e-12 * n2 and np.abs(e - refe).max() <= 1e-12 * n2
    assert raw_dimer(pkg, m, psi, bonds + [(1, 2)])[0] == pkg._lib.SD_EARG       # one bond more than the library takes


# ---- 3. exact states ----
def test_dimer_singlet_product_state(pkg):
    from test_gpu_transverse import dimer_singlet
    L = 16
    m = pkg.XXZChain(L, nup=L // 2, boundary="periodic")
    psi = dimer_singlet(L)
    bonds = pkg.model_bonds(m)
    assert bonds == [(i, i % L + 1) for i in range(1, L + 1)]
    D, e = pkg.dimer_correlation_matrix(psi, m), pkg.bond_energies(psi, m)
    want_e = np.array([-0.75 if b % 2 == 0 else 0.0 for b in range(L)])
    want_D = np.zeros((L, L))
    for a in range(L):
        for b in range(L):
            if a % 2 == 0 and b % 2 == 0:
                want_D[a, b] = 9 / 16                             # two singlet bonds
            elif a == b:
                want_D[a, b] = 3 / 16                             # a bond between singlets
    assert D.dtype == np.float64
    print("singlet product:", np.abs(D - want_D).max(), np.abs(e - want_e).max())
    assert np.abs(D - want_D).max() <= 1e-14 and np.abs(e - want_e).max() <= 1e-14
    sd_pi = pkg.dimer_structure_factor(psi, m, np.pi)
    assert sd_pi.shape == (1,) and sd_pi.dtype == np.float64
    assert abs(sd_pi[0] - ((L / 2) ** 2 * 9 / 16 + (L / 2) * 3 / 16) / L) <= 1e-13
    two = pkg.dimer_structure_factor(psi, m, [0.0, np.pi], connected=True)
    Dc = D - np.outer(e, e)
    assert abs(two[0] - Dc.sum() / L) <= 1e-13


def test_neel_state_is_exact(pkg):
    L = 12
    m = pkg.XXZChain(L, nup=L // 2, boundary="periodic", **XXZ)
    psi = pkg.neel_state(m)
    bonds = pkg.model_bonds(m) + [(1, 3), (2, 7)]
    up = np.array([1.0 if i % 2 == 0 else 0.0 for i in range(L)])            # neel: sites 1, 3, ... up
    sgn = np.array([(2 * up[i - 1] - 1) * (2 * up[j - 1] - 1) for i, j in bonds])
    for zz in (1.0, 0.7):
        c = zz * 0.25
        D, e = pkg.dimer_correlation_matrix(psi, m, bonds, xy=0.0, zz=zz), pkg.bond_energies(psi, m, bonds, xy=0.0, zz=zz)
        assert np.array_equal(D, np.outer(c * sgn, c * sgn)) and np.array_equal(e, c * sgn)


@pytest.mark.parametrize("nup", [0, 6])
def test_polarised_sectors(pkg, nup):
    L = 6
    m = pkg.XXZChain(L, nup=nup, **XXZ)
    assert m.N == 1
    bonds = [(1, 2), (6, 1), (2, 5), (3, 4), (4, 3)]
    for psi in (np.array([1.5]), np.array([0.5 - 1.25j])):
        for xy, zz in ((1.0, 1.0), (0.8, 0.7)):
            c = zz * 0.25
            re, im = c * psi[0].real, c * psi[0].imag
            n2 = re * re + im * im                            # (zz/4)^2 |psi|^2 in the kernel's order: (c re)(c re) + (c im)(c im)
            D, e = pkg.dimer_correlation_matrix(psi, m, bonds, xy=xy, zz=zz), pkg.bond_energies(psi, m, bonds, xy=xy, zz=zz)
            assert np.array_equal(D, np.full((5, 5), n2)) and D.dtype == psi.dtype
            assert np.array_equal(e, np.full(5, psi[0].real * re + psi[0].imag * im))
            want = np.array([complex(re, im)]) if np.iscomplexobj(psi) else np.array([re])
            assert np.array_equal(pkg.bond_operator(psi, m, 2, 5, xy=xy, zz=zz), want)


# ---- 4. physics from the solver ----
def test_majumdar_ghosh_chain_from_the_solver(pkg):
    """Open J1-J2 chain, L = 12, nup = 6, J1 = 1, J2 = 0.5, no field: the ground state is the product of singlets on (1,2), (3,4), ...,
    E0 = -3L/8 = -4.5, and the nearest-neighbour bond energies alternate (-3/4, 0).  Bar 1e-8, that of the free-fermion test of
    tests/test_gpu_pair_correlations.py (the gap here, 0.4, is larger than in that gapless case)."""
    L, nup, J1, J2 = 12, 6, 1.0, 0.5
    hop = [(i, i + 1, J1 / 2) for i in range(1, L)] + [(i, i + 2, J2 / 2) for i in range(1, L - 1)]
    zz = [(i, i + 1, J1) for i in range(1, L)] + [(i, i + 2, J2) for i in range(1, L - 1)]
    m = pkg.build_model(L, nup=nup, hopping=hop, zz=zz, onsite_field=np.zeros(L))
    E0, psi = pkg.groundstate(m, lanc_m=100)
    psi = np.asarray(psi)
    nn = [(i, i + 1) for i in range(1, L)]
    e = pkg.bond_energies(psi, m, nn)
    want = np.array([-0.75 if b % 2 == 0 else 0.0 for b in range(L - 1)])
    print("E0", E0, "bond energies", e)
    assert abs(E0 + 4.5) <= 1e-8 and np.abs(e - want).max() <= 1e-8
    every = pkg.bond_energies(psi, m)                          # the model's own list: first, then second neighbours
    assert len(every) == 2 * L - 3 and abs(J1 * every[:L - 1].sum() + J2 * every[L - 1:].sum() - E0) <= 1e-8
    sd_pi = pkg.dimer_structure_factor(psi, m, np.pi, bonds=nn)[0]      # B entries per row of D, each within 1e-8
    assert abs(sd_pi - ((L / 2) ** 2 * 9 / 16 + (L / 2 - 1) * 3 / 16) / (L - 1)) <= 1e-8 * (L - 1)


# ---- 5 and 6. the grid-wrap shapes ----
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


def assert_wraps(sh):
    assert_crosses_the_caps(sh)
    if sh.path == 1:
        assert len(sh.tiles[0]) > DIMER_MAX_BLOCKS           # a workgroup takes a second and later tile
    else:
        assert sh.N > DIMER_MAX_BLOCKS * 256                 # the grid-stride loop runs again


def wrap_bonds(L):
    """seven bonds, a ragged 4 + 3; (L-12, L-11) straddles the prefix / suffix cut of the tiled plan"""
    mid = L // 2
    return [(mid, mid + 1), (mid + 1, mid + 2), (L, 1), (1, 2), (L - 12, L - 11), (L - 10, L - 5), (2, L - 1)]


@pytest.mark.parametrize("name", ["T-periodic", "R-periodic", "Rg", "F"])
def test_grid_wrap_against_the_row_sums(pkg, shapes, name):
    sh = shapes.get(name)
    assert_wraps(sh)
    L, m = sh.L, sh.m
    bonds = wrap_bonds(L)
    for psi in (sh.psi_r, sh.psi_c):
        cplx = psi.is_complex()
        n2 = norm2(psi)
        refD, refe = DR.gram(psi, L, sh.nup, bonds, 0.8, 0.7, s=sh.s)
        rc, D, e = raw_dimer(pkg, m, psi, bonds, 0.8, 0.7)
        assert rc == 0
        check_matrix(D, e, 7, True)
        if not cplx:
            assert np.all(D.imag == 0.0)
        err, erre = np.abs(D - refD).max(), np.abs(e - refe).max()
        print(f"{name} {'c128' if cplx else 'f64'}: D {err:.2e} e {erre:.2e} (bar {1e-12 * n2:.2e}), max |ref| {np.abs(refD).max():.3e}")
        assert err <= 1e-12 * n2 and erre <= 1e-12 * n2
        assert np.abs(refD).max() > 1e-6 * n2                 # a real comparison, not zeros against zeros
        rc2, D2, e2 = raw_dimer(pkg, m, psi, bonds, 0.8, 0.7)  # same call twice: equal bits
        assert rc2 == 0 and np.array_equal(D.view(np.float64), D2.view(np.float64)) and np.array_equal(e, e2)
        for (i, j) in ((L - 12, L - 11), (L, 1)):
            want = DR.bond_rows(psi, sh.s, L, sh.nup, i, j, 0.8, 0.7)
            got = pkg.bond_operator(psi, m, i, j, xy=0.8, zz=0.7)
            assert equal_bits(got, want), (name, i, j, int((got != want).sum()))
            del got, want


def test_ties_to_independent_kernels_at_T(pkg, shapes):
    """the bond energies against the pair kernel, and sum_ab D_ab against |H psi|^2 of the apply; psi normalised"""
    import torch
    sh = shapes.get("T-periodic")
    assert_wraps(sh)
    m, L, nup = sh.m, sh.L, sh.nup
    psi = sh.psi_c / torch.linalg.vector_norm(sh.psi_c)
    hop = m.hopping_list
    bonds = [(i, j) for i, j, _t in hop]
    assert bonds == pkg.model_bonds(m) and len({t for _i, _j, t in hop}) == 1 and len({J for _i, _j, J in m.zz_list}) == 1
    assert [(i, j) for i, j, _J in m.zz_list] == bonds
    xy, zz = 2 * hop[0][2], m.zz_list[0][2]
    assert (xy, zz) == (XXZ["Jxy"], XXZ["Jz"])
    D, e = pkg.dimer_correlation_matrix(psi, m, xy=xy, zz=zz), pkg.bond_energies(psi, m, xy=xy, zz=zz)
    G, Z = pkg.correlation_matrix(psi, m, "+-"), pkg.correlation_matrix(psi, m, "zz")
    want = np.array([xy * G[i - 1, j - 1].real + zz * Z[i - 1, j - 1] for i, j in bonds])
    print("bond energies vs the pair kernel:", np.abs(e - want).max())
    assert np.abs(e - want).max() <= 1e-11
    hz = XXZ["hz"]
    assert np.all(m.onsite_field == hz)
    c = hz * (nup - L / 2)
    hpsi = torch.empty_like(psi)
    pkg.apply_H(hpsi, psi, m)
    h2 = norm2(hpsi)
    got = D.sum() + 2 * c * e.sum() + c * c
    scale = sum(abs(t) for _, _, t in hop) + sum(abs(J) for _, _, J in m.zz_list) / 4 + np.abs(m.onsite_field).sum() / 2
    print(f"|H psi|^2 from the dimer matrix {got.real:.12f}, from apply_H {h2:.12f} (scale^2 {scale ** 2:.2f})")
    assert abs(got.real - h2) <= 1e-11 * scale ** 2 and abs(got.imag) <= 1e-11 * scale ** 2


# ---- 7. refusals ----
def test_refusals(pkg):
    import torch
    E = pkg._lib
    L = 12
    m = pkg.XXZChain(L, nup=6, boundary="periodic", **XXZ)
    psi = fill_randn(pkg, m, m.N, True, 99)
    host = psi.cpu().numpy()
    ok = [(1, 2), (3, 4)]
    for x in (psi, host):
        out = torch.empty_like(psi) if x is psi else np.empty_like(host)
        assert raw_dimer(pkg, m, x, ok)[0] == 0 and raw_bond(pkg, m, x, 1, 2, out) == 0
        for bad in ((3, 3), (0, 1), (1, L + 1), (-1, 2)):                                  # i == j, a site outside 1..L
            assert raw_dimer(pkg, m, x, [(1, 2), bad])[0] == E.SD_EARG
            assert raw_bond(pkg, m, x, bad[0], bad[1], out) == E.SD_EARG
        assert raw_dimer(pkg, m, x, ok, B=0)[0] == E.SD_EARG and raw_dimer(pkg, m, x, ok, B=-1)[0] == E.SD_EARG
        assert raw_dimer(pkg, m, x, [(1, 2)] * (DIMER_MAX_BONDS + 1))[0] == E.SD_EARG
        assert raw_dimer(pkg, m, x, [(1, 2)] * DIMER_MAX_BONDS)[0] == 0
        assert raw_dimer(pkg, m, x, ok, dtype=3)[0] == E.SD_EARG and raw_bond(pkg, m, x, 1, 2, out, dtype=3) == E.SD_EARG
        assert raw_dimer(pkg, m, x, ok, n=m.N - 1)[0] == E.SD_EDIM and raw_bond(pkg, m, x, 1, 2, out, n=m.N - 1) == E.SD_EDIM
        assert raw_dimer(pkg, m, x, ok, xy=float("nan"))[0] == E.SD_EARG and raw_bond(pkg, m, x, 1, 2, out, zz=float("inf")) == E.SD_EARG
    assert raw_bond(pkg, m, psi, 1, 2, psi) == E.SD_EARG                                   # out aliasing psi on the device
    # the Python exceptions
    with pytest.raises(pkg.ArgumentError):
        pkg.dimer_correlation_matrix(host, m, [(1, 1)])
    with pytest.raises(pkg.ArgumentError):
        pkg.bond_energies(psi, m, [])
    with pytest.raises(pkg.ArgumentError):
        pkg.bond_operator(psi, m, 1, L + 1)
    with pytest.raises(pkg.ArgumentError):
        pkg.bond_operator(psi, m, 1, 2, out=psi)
    with pytest.raises(pkg.ArgumentError):
        pkg.bond_operator(psi, m, 1, 2, out=host)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.bond_operator(host, m, 1, 2, out=np.empty(m.N - 1, dtype=host.dtype))
    with pytest.raises(pkg.DimensionMismatch):
        pkg.dimer_correlation_matrix(host[:-1], m)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.dimer_structure_factor(psi[:-1].contiguous(), m, np.pi)
    # a sharded model
    sharded = pkg.XXZChain(L, nup=6, boundary="periodic", **XXZ)
    sharded.set_shard(0, 2)
    out = torch.empty_like(psi)
    assert raw_dimer(pkg, sharded, psi, ok)[0] == E.SD_EARG and raw_dimer(pkg, sharded, host, ok)[0] == E.SD_EARG
    assert raw_bond(pkg, sharded, psi, 1, 2, out) == E.SD_EARG and raw_bond(pkg, sharded, host, 1, 2, np.empty_like(host)) == E.SD_EARG
    with pytest.raises(pkg.ArgumentError):
        pkg.dimer_correlation_matrix(host, sharded)
    # a model without device tables
    bare = pkg.XXZChain(L, nup=6, boundary="periodic", ctx=None, **XXZ)
    rc = pkg.lib().sd_dimer_correlations(m.ctx.h, bare.h, E.SD_C128, host.ctypes.data, m.N, np.array([1, 2], dtype=np.intc).ctypes.data_as(_ip),
                                         1, 1.0, 1.0, np.empty(2).ctypes.data_as(_dp), np.empty(1).ctypes.data_as(_dp))
    assert rc == E.SD_EARG
    assert pkg.lib().sd_bond_apply(m.ctx.h, bare.h, E.SD_C128, host.ctypes.data, m.N, 1, 2, 1.0, 1.0, np.empty_like(host).ctypes.data) == E.SD_EARG
