"""Equal-time pair correlations: sd_pair_correlations[_dev] and the Python mirror (correlation_matrix,
static_structure_factor, momentum_distribution) against tests/pair_ref.py (proven on the CPU by tests/test_pair_ref_host.py),
against exact states, against the library's own independent kernels, and against free fermions.

Tolerance of every comparison with pair_ref: elementwise |M_dev - M_ref| <= 1e-12 <psi|psi>.  Each entry is a sum of at most N
products bounded by |psi|^2 and the blocked sums are accurate to a few tens of eps at these N, so 1e-12 leaves more than two orders
of margin and still catches one dropped or misplaced row block.

The kernel takes the rows' configurations from the tile plan (sd_model_path 1), from unrank (path 0, fixed-nup sector) or from the
row index (full basis, path 0 or 2) and finds partner rows by the plan's tables, by the local rank walk or by an exclusive or: every
shape asserts its path so that all three are known to run.  The grid-wrap shapes are those of tests/test_gpu_operator_grids.py."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

import pair_ref as PR
from test_gpu_operator_grids import XXZ, Shape, assert_crosses_the_caps, fill_randn, j1j2

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
PAIR_MAX_BLOCKS = 2048        # SD_PAIR_MAX_BLOCKS of kernels_pairs.hip: row blocks of the launch (tiles, or blocks of 256 rows)

# name -> (L, nup, boundary (None: the J1-J2 lists), SD_SUFFIX_BITS, sd_model_path)
SMALL = {
    "L2n1-open": (2, 1, "open", None, 1), "L2n1-periodic": (2, 1, "periodic", None, 1),
    "L4n2-open": (4, 2, "open", None, 1), "L4n2-periodic": (4, 2, "periodic", None, 1),
    "L12n6-open": (12, 6, "open", None, 1), "L12n6-periodic": (12, 6, "periodic", None, 1),
    "L16n8-open": (16, 8, "open", None, 1), "L16n8-periodic": (16, 8, "periodic", None, 1),
    "L16n3-open": (16, 3, "open", None, 1), "L16n3-periodic": (16, 3, "periodic", None, 1),
    "J1J2-L14n7": (14, 7, None, None, 1),
    "L14n7-suffix8": (14, 7, "periodic", 8, 1),
    "L13n1-per-row": (13, 1, "periodic", None, 0),       # the smallest sector the planner leaves without tiles: the rank walk
    "full-L10": (10, None, "periodic", None, 0),         # full basis below the tiled size: rows are configurations
}


def build(pkg, L, nup, boundary, ls):
    with pytest.MonkeyPatch.context() as mp:              # the plan reads SD_SUFFIX_BITS when the model is built
        if ls is None:
            mp.delenv("SD_SUFFIX_BITS", raising=False)
        else:
            mp.setenv("SD_SUFFIX_BITS", str(ls))
        if boundary is None:
            hop, zz, field = j1j2(L)
            return pkg.build_model(L, nup=nup, hopping=hop, zz=zz, onsite_field=field)
        return pkg.XXZChain(L, nup=nup, boundary=boundary, **XXZ)


def raw(pkg, m, psi, component, n=None, dtype=None):
    """status and the (L, L) complex matrix of sd_pair_correlations[_dev] called directly"""
    import torch
    out = np.full((m.L, m.L), np.nan + 1j * np.nan, dtype=np.complex128)
    n = len(psi) if n is None else n
    if isinstance(psi, torch.Tensor):
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        code = (pkg._lib.SD_C128 if psi.is_complex() else pkg._lib.SD_F64) if dtype is None else dtype
        rc = pkg.lib().sd_pair_correlations_dev(m.ctx.h, m.h, code, psi.data_ptr(), n, component, out.ctypes.data_as(_dp))
    else:
        code = (pkg._lib.SD_C128 if np.iscomplexobj(psi) else pkg._lib.SD_F64) if dtype is None else dtype
        rc = pkg.lib().sd_pair_correlations(m.ctx.h, m.h, code, psi.ctypes.data, n, component, out.ctypes.data_as(_dp))
    return rc, out


def norm2(psi):
    import torch
    return float(torch.linalg.vector_norm(psi).item()) ** 2


# ---- 1. all pairs, all rows, small ----
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("name", list(SMALL))
def test_all_pairs_small(pkg, name, cplx):
    L, nup, boundary, ls, path = SMALL[name]
    m = build(pkg, L, nup, boundary, ls)
    assert pkg.lib().sd_model_path(m.h) == path
    if ls is not None:                                    # many short tiles: prefix-prefix, prefix-suffix and suffix-suffix pairs
        assert len(m.local_tiles()[0]) == 2 ** (L - ls) and L - ls >= 2 and ls >= 2
    psi = fill_randn(pkg, m, m.N, cplx, 4242 + 7 * L + (nup or 0))
    n2 = norm2(psi)
    host = psi.cpu().numpy()
    for comp in ("zz", "+-"):
        ref = PR.correlations(psi, L, nup, comp)
        if comp == "+-" and cplx:
            assert np.abs(ref.imag).max() > 1e-3          # the conjugation is really exercised
        for x in (psi, host):
            got = pkg.correlation_matrix(x, m, comp)
            assert got.shape == (L, L) and got.dtype == (np.float64 if comp == "zz" else np.complex128)
            err = np.abs(got - ref).max()
            print(f"{name} {comp} {'dev' if x is psi else 'host'}: {err:.2e} (bar {1e-12 * n2:.2e})")
            assert err <= 1e-12 * n2
            if comp == "+-":
                assert np.array_equal(got, got.conj().T)  # Hermitian to the bit: one triangle is summed
                if not cplx:
                    assert np.all(got.imag == 0.0)
        rc, z = raw(pkg, m, psi, 0)
        assert rc == 0 and np.all(z.imag == 0.0)
    # derived components
    G, sz = pkg.correlation_matrix(psi, m, "+-"), pkg.magnetization_per_site(psi, m)
    Gmp = pkg.correlation_matrix(psi, m, "-+")
    off = ~np.eye(L, dtype=bool)
    assert np.array_equal(Gmp[off], G.conj()[off])
    assert np.abs(np.diagonal(Gmp).real - (0.5 * n2 - sz)).max() <= 1e-12 * n2 and np.all(np.diagonal(Gmp).imag == 0.0)
    assert np.abs(np.diagonal(G).real - (0.5 * n2 + sz)).max() <= 1e-12 * n2
    if nup is None:
        with pytest.raises(pkg.ArgumentError):
            pkg.correlation_matrix(psi, m, "xx")
    else:
        X = pkg.correlation_matrix(psi, m, "xx")
        assert X.dtype == np.float64 and np.abs(X - 0.25 * (G + Gmp).real).max() <= 1e-15 * n2
    with pytest.raises(pkg.ArgumentError):
        pkg.correlation_matrix(psi, m, "yy")


# ---- 2. edges ----
@pytest.mark.parametrize("nup", [0, 6])
def test_polarised_sectors(pkg, nup):
    L = 6
    m = pkg.XXZChain(L, nup=nup, **XXZ)
    assert m.N == 1
    for psi in (np.array([1.5]), np.array([0.5 - 1.25j])):
        n2 = float(psi[0].real ** 2 + psi[0].imag ** 2)       # the kernel's |psi|^2: re * re + im * im
        G, Z = pkg.correlation_matrix(psi, m, "+-"), pkg.correlation_matrix(psi, m, "zz")
        assert np.array_equal(G, np.eye(L) * (n2 if nup == L else 0.0))       # G_ii = <psi|psi>/2 + <S^z_i>, off-diagonals 0
        assert np.array_equal(Z, np.full((L, L), 0.25 * n2))
        Gmp = pkg.correlation_matrix(psi, m, "-+")
        assert np.array_equal(Gmp, np.eye(L) * (0.0 if nup == L else n2))


def test_neel_state_is_exact(pkg):
    L = 12
    m = pkg.XXZChain(L, nup=L // 2, boundary="periodic", **XXZ)
    psi = pkg.neel_state(m)
    up = np.array([1.0 if i % 2 == 0 else 0.0 for i in range(L)])            # neel: sites 1, 3, ... up
    sgn = 2 * up - 1
    assert np.array_equal(pkg.correlation_matrix(psi, m, "zz"), 0.25 * np.outer(sgn, sgn))
    assert np.array_equal(pkg.correlation_matrix(psi, m, "+-"), np.diag(up).astype(np.complex128))


def test_dimer_singlet_product_state(pkg):
    from test_gpu_transverse import dimer_singlet
    L = 16
    m = pkg.XXZChain(L, nup=L // 2, boundary="periodic")
    psi = dimer_singlet(L)
    G, Z = pkg.correlation_matrix(psi, m, "+-"), pkg.correlation_matrix(psi, m, "zz")
    wantG, wantZ = 0.5 * np.eye(L), 0.25 * np.eye(L)
    for k in range(0, L, 2):                               # sites (2k-1, 2k) of the issue: 0-based (k, k+1), k even
        wantG[k, k + 1] = wantG[k + 1, k] = -0.5
        wantZ[k, k + 1] = wantZ[k + 1, k] = -0.25
    assert np.abs(G - wantG).max() <= 1e-14 and np.abs(Z - wantZ).max() <= 1e-14
    X = pkg.correlation_matrix(psi, m, "xx")               # a singlet: <S^x S^x> = <S^z S^z>
    assert np.abs(X - Z).max() <= 1e-14


# ---- 3 and 4. the grid-wrap shapes ----
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
        assert len(sh.tiles[0]) > PAIR_MAX_BLOCKS            # a workgroup takes a second and later tile
    else:
        assert sh.N > PAIR_MAX_BLOCKS * 256                  # the grid-stride loop runs again


def subset_pairs(L, split):
    """13 ordered pairs: nearest in both orders, (1, L), (1, 2), (L-1, L), one straddling site `split` | `split`+1 (the prefix / suffix cut of the tiled
    plan), one inside the suffix, six seeded random ones"""
    mid = L // 2
    pairs = [(mid, mid + 1), (mid + 1, mid), (1, L), (1, 2), (L - 1, L), (split, split + 1), (split + 2, split + 7)]
    rng = np.random.default_rng(1000 + L)
    while len(pairs) < 13:
        i, j = (int(x) for x in rng.integers(1, L + 1, 2))
        if i != j and (i, j) not in pairs:
            pairs.append((i, j))
    return pairs


@pytest.mark.parametrize("name", ["T-periodic", "R-periodic", "Rg", "F"])
def test_grid_wrap_against_the_row_sums(pkg, shapes, name):
    sh = shapes.get(name)
    assert_wraps(sh)
    L = sh.L
    pairs = subset_pairs(L, L - 12)
    for psi in (sh.psi_r, sh.psi_c):
        n2 = norm2(psi)
        G, Z = pkg.correlation_matrix(psi, sh.m, "+-"), pkg.correlation_matrix(psi, sh.m, "zz")
        rg = PR.correlations(psi, L, sh.nup, "+-", pairs=pairs, s=sh.s)
        rz = PR.correlations(psi, L, sh.nup, "zz", pairs=pairs + [(1, 1), (L, L)], s=sh.s)
        eg = max(abs(G[i - 1, j - 1] - v) for (i, j), v in rg.items())
        ez = max(abs(Z[i - 1, j - 1] - v) for (i, j), v in rz.items())
        print(f"{name} {'c128' if psi.is_complex() else 'f64'}: +- {eg:.2e} zz {ez:.2e} (bar {1e-12 * n2:.2e})")
        assert eg <= 1e-12 * n2 and ez <= 1e-12 * n2
        assert max(abs(v) for v in rg.values()) > 1e-6 * n2      # a real comparison, not zeros against zeros
        diag = np.array([PR.g_pm(psi, sh.s, L, sh.nup, i, i) for i in (1, L // 2, L)]).real
        assert np.abs(np.diagonal(G).real[[0, L // 2 - 1, L - 1]] - diag).max() <= 1e-12 * n2
        # same call twice: equal bits
        assert np.array_equal(G.view(np.float64), pkg.correlation_matrix(psi, sh.m, "+-").view(np.float64))


def test_identities_on_all_pairs_at_T(pkg, shapes):
    """every pair of the T shape tied to an independent kernel of the library; psi normalised, tolerances relative 1e-11"""
    import torch
    sh = shapes.get("T-periodic")
    assert_wraps(sh)
    m, L, nup = sh.m, sh.L, sh.nup
    psi = sh.psi_c / torch.linalg.vector_norm(sh.psi_c)
    G, Z = pkg.correlation_matrix(psi, m, "+-"), pkg.correlation_matrix(psi, m, "zz")
    qs = np.array([0.0, np.pi, 2 * np.pi * 3 / L])
    spm, szz = pkg.static_structure_factor(psi, m, qs, "+-"), pkg.static_structure_factor(psi, m, qs, "zz")
    for k, q in enumerate(qs):
        want = norm2(pkg.Sminus_q_vector(m, psi, q))
        wantz = norm2(pkg.Sz_q_vector(m, psi, q))
        print(f"q={q:.3f}: S+- {spm[k]:.12f} vs {want:.12f}; Szz {szz[k]:.12f} vs {wantz:.12f}")
        assert abs(spm[k] - want) <= 1e-11 * max(want, 1.0) and abs(szz[k] - wantz) <= 1e-11 * max(wantz, 1.0)
    assert np.array_equal(pkg.momentum_distribution(psi, m, qs), spm)
    assert len(pkg.momentum_distribution(psi, m)) == L
    assert abs(np.trace(G).real - nup) <= 1e-11 * nup and abs(np.trace(G).imag) == 0.0
    assert abs(Z.sum() - (nup - L / 2) ** 2) <= 1e-11
    Zc = pkg.correlation_matrix(psi, m, "zz", connected=True)
    lag = np.array([np.mean([Zc[i, (i + r) % L] for i in range(L)]) for r in range(L)])
    assert np.abs(lag - pkg.connected_correlations(psi, m)).max() <= 1e-11
    # <H> from the model's own lists (hops stored as t_b = Jxy / 2)
    sz = pkg.magnetization_per_site(psi, m)
    e = sum(2 * t * G[i - 1, j - 1].real for i, j, t in m.hopping_list) + sum(J * Z[i - 1, j - 1] for i, j, J in m.zz_list) \
        + float(np.dot(m.onsite_field, sz))
    hpsi = torch.empty_like(psi)
    pkg.apply_H(hpsi, psi, m)
    want = float(torch.vdot(psi, hpsi).real.item())
    scale = sum(abs(t) for _, _, t in m.hopping_list) + sum(abs(J) for _, _, J in m.zz_list) / 4 + np.abs(m.onsite_field).sum() / 2
    print(f"<H> from the matrices {e:.12f}, from apply_H {want:.12f} (scale {scale:.2f})")
    assert abs(e - want) <= 1e-11 * scale


# ---- 5. known physics: free fermions ----
def test_xx_chain_bond_correlations_are_free_fermions(pkg):
    """Open XX chain, Jz = 0, L = 12, nup = 6, Jxy = -1: the Jordan-Wigner fermions hop with amplitude Jxy / 2 < 0, the ground state
    fills the orbitals k = 1..6 of phi_k(i) = sqrt(2/(L+1)) sin(k pi i/(L+1)), and the string is trivial between neighbours:
    G_{i,i+1} = sum_{k<=6} phi_k(i) phi_k(i+1).  (With Jxy = +1 the filled orbitals are k = 7..12 and the sum changes sign.)"""
    L, nup = 12, 6
    m = pkg.XXZChain(L, Jxy=-1.0, Jz=0.0, hz=0.0, nup=nup, boundary="open")
    _E0, psi = pkg.groundstate(m, lanc_m=100)
    G = pkg.correlation_matrix(np.asarray(psi), m, "+-")
    i = np.arange(1, L + 1)
    phi = np.array([math.sqrt(2 / (L + 1)) * np.sin(k * np.pi * i / (L + 1)) for k in range(1, nup + 1)])
    want = (phi[:, :-1] * phi[:, 1:]).sum(axis=0)
    got = np.array([G[k, k + 1].real for k in range(L - 1)])
    print("bond correlations", got, "free fermions", want)
    assert np.abs(got - want).max() <= 1e-8
    assert np.abs(np.diagonal(G).real - (phi ** 2).sum(axis=0)).max() <= 1e-8      # the density


# ---- 6. refusals and determinism ----
def test_refusals_and_equal_bits(pkg):
    E = pkg._lib
    m = pkg.XXZChain(12, nup=6, boundary="periodic", **XXZ)
    psi = fill_randn(pkg, m, m.N, True, 99)
    host = psi.cpu().numpy()
    for x in (psi, host):
        assert raw(pkg, m, x, 2)[0] == E.SD_EARG and raw(pkg, m, x, -1)[0] == E.SD_EARG        # component
        assert raw(pkg, m, x, 1, dtype=3)[0] == E.SD_EARG                                       # dtype
        assert raw(pkg, m, x, 1, n=m.N - 1)[0] == E.SD_EDIM                                     # length
        a, b = raw(pkg, m, x, 1), raw(pkg, m, x, 1)
        assert a[0] == b[0] == 0 and np.array_equal(a[1].view(np.float64), b[1].view(np.float64))
    with pytest.raises(pkg.DimensionMismatch):
        pkg.correlation_matrix(host[:-1], m, "zz")
    sharded = pkg.XXZChain(12, nup=6, boundary="periodic", **XXZ)
    sharded.set_shard(0, 2)
    assert raw(pkg, sharded, psi, 1)[0] == E.SD_EARG and raw(pkg, sharded, host, 0)[0] == E.SD_EARG
    with pytest.raises(pkg.ArgumentError):
        pkg.correlation_matrix(host, sharded, "+-")
