"""The operator and reduction kernels at the sizes where their capped launch grids wrap: the spin current (write and bracket
form), the site projections, the observables, S^z_q and the single-site spin operators, at the smallest shapes that send a
workgroup through its grid-stride loop more than once -- a second and later tile per workgroup, the tail blocks, the 64-bit row
arithmetic -- against the row restatements of tests/rows_ref.py (proven on the CPU by tests/test_rows_ref_host.py), formed with torch
on the device over ALL rows.

Shapes (default plan: 12 suffix sites):
  T   XXZ L=25 nup=12, tiled, 8191 tiles of up to 924 rows, 5 200 300 rows   (> 4096 and 2048 tiles, > 16384 * 256 rows)
  Ts  XXZ L=21 nup=10, SD_SUFFIX_BITS=8: 8086 tiles of at most 70 rows        (tiles shorter than a workgroup: waves 2, 3 idle)
  R   XXZ L=39 nup=6, per-row path, 3 262 623 rows                            (> 8192 * 256 and 2048 * 256 rows)
  Rg  J1-J2 hop list on L=39 nup=6, per-row path                              (every non-chain hop through the rank walk)
  F   XXZ L=23 full basis, 8192 tiles of 1024 rows, 8 388 608 rows            (4 passes of 8192 blocks, 2 of 16384; k_szq_full k=11)
  B   XXZ L=34 nup=17, 2 333 606 220 rows                                     (rows past 2^31; sampled rows)
Every test first asserts that its shape still crosses the cap it is there for: the numbers are the launchers' constants.

Vectors come from the library's counter-based normal stream and stay on the device; outputs the caller owns are filled with
NaN first.  Exact comparisons are exact: real and imaginary parts as separate IEEE doubles under ==.

site_project: the public entry point returns the L site sums only -- the (sum |ket|^2, 0) entry of the kernel's result row stays
inside the library (it guards the moment recursion) -- so the probe kets pin the L site entries."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

import rows_ref as RR

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
NAN = float("nan")


def j1j2(L, J1=1.0, J2=0.4):
    hop = [(i, i % L + 1, J1 / 2) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2 / 2) for i in range(1, L + 1)]
    zz = [(i, i % L + 1, J1) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2) for i in range(1, L + 1)]
    return hop, zz, np.full(L, 0.1)


def weight_sets(nh, seed):
    return [None, np.eye(nh)[nh // 2], np.random.default_rng(seed).standard_normal(nh)]


XXZ = dict(Jxy=0.8, Jz=0.7, hz=0.3)
# name -> L, nup, boundary (None: the J1-J2 lists), SD_SUFFIX_BITS or None, sd_model_path (0 per row, 1 tiled, 2 full basis)
SPECS = {
    "T-periodic": (25, 12, "periodic", None, 1),
    "T-open": (25, 12, "open", None, 1),
    "Ts": (21, 10, "periodic", 8, 1),
    "R-periodic": (39, 6, "periodic", None, 0),
    "R-open": (39, 6, "open", None, 0),
    "Rg": (39, 6, None, None, 0),
    "F": (23, None, "periodic", None, 2),
}


def fill_randn(pkg, m, N, cplx, seed):
    import torch
    x = torch.empty(N, dtype=torch.complex128 if cplx else torch.float64, device=torch.device("cuda", m.ctx.device))
    m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, x.data_ptr(), (2 if cplx else 1) * N, seed, 0), m.ctx.h)
    return x


class Shape:
    """a model at one of the shapes, its configurations and random vectors on the device, and the row-loop current of the vectors"""

    def __init__(self, pkg, name):
        import torch
        self.name = name
        self.L, self.nup, boundary, ls, self.path = SPECS[name]
        L = self.L
        with pytest.MonkeyPatch.context() as mp:              # the plan reads SD_SUFFIX_BITS when the model is built
            if ls is None:
                mp.delenv("SD_SUFFIX_BITS", raising=False)
            else:
                mp.setenv("SD_SUFFIX_BITS", str(ls))
            if boundary is None:
                hop, zz, field = j1j2(L)
                self.m = pkg.build_model(L, nup=self.nup, hopping=hop, zz=zz, onsite_field=field)
            else:
                self.m = pkg.XXZChain(L, nup=self.nup, boundary=boundary, **XXZ)
            assert pkg.lib().sd_model_path(self.m.h) == self.path
            self.tiles = None
            if self.path == 1:                                # (first row, length) of every tile, in the kernels' tile order
                lb, gb, ln = self.m.local_tiles()
                assert np.array_equal(lb, gb)                 # one device holds the whole sector: local rows are global rows
                self.tiles = (gb, ln)
        m = self.m
        self.hop, self.N = m.hopping_list, m.N
        self.dev = torch.device("cuda", m.ctx.device)
        self.rows = torch.arange(m.N, dtype=torch.int64, device=self.dev)
        self.s = RR.configurations_t(self.rows, L, self.nup)
        self.psi_r = fill_randn(pkg, m, m.N, False, 101 + L)
        self.psi_c = fill_randn(pkg, m, m.N, True, 202 + L)
        self.wsets = weight_sets(len(self.hop), L)
        self._jref = self._bra = None

    def jref(self):
        """{(k, m): (re, im)} of J_w psi for psi = (psi_r, psi_c)[k] and weights wsets[m], all rows, by the row loop"""
        if self._jref is None:
            self._jref = RR.current_rows([self.psi_r, self.psi_c], self.wsets, self.s, self.rows, self.L, self.nup, self.hop)
        return self._jref

    def bra_c(self, pkg):
        if self._bra is None:
            self._bra = fill_randn(pkg, self.m, self.N, True, 303 + self.L)
        return self._bra

    def config(self, row):
        return int(self.s[row].item())

    def tile_of(self, rows):
        if self.tiles is None:
            return None
        order = np.argsort(self.tiles[0])                     # the tile order is not the row order
        return order[np.searchsorted(self.tiles[0][order], np.asarray(rows), side="right") - 1].tolist()

    def probe_rows(self):
        """rows a one-pass grid does not reach: the first and last row, and in tiles past 2048 and past 4096 (tiled plans) the
        first row, a row of wave 1, a row of the second trip of the inner loop and the last row; rows past 2048 * 256 and past
        8192 * 256 otherwise"""
        N = self.N
        rows = [0, N - 1]
        if self.tiles is not None:
            gb, ln = self.tiles
            two_waves = np.nonzero(ln > 66)[0]                 # tiles that fill more than one wave
            picks = [two_waves[two_waves >= 2048 + 5][0], two_waves[two_waves >= 4096 + 3][0], two_waves[-1]]
            assert picks[2] > picks[1] >= 4096
            for t in picks:
                rows += [int(gb[t]), int(gb[t]) + 66, int(gb[t]) + min(int(ln[t]) - 1, 300), int(gb[t]) + int(ln[t]) - 1]
        else:
            rows += [524_288 + 77, 2_097_152, 2_097_152 + 1029, (N + 2_097_152) // 2]
        return sorted(set(rows))


class Shapes:
    def __init__(self, pkg):
        self.pkg, self.store = pkg, {}

    def get(self, name):
        if name not in self.store:
            self.store[name] = Shape(self.pkg, name)
        return self.store[name]

    def drop(self, name):
        self.store.pop(name, None)


@pytest.fixture(scope="module")
def shapes(pkg):
    import torch
    st = Shapes(pkg)
    yield st
    st.store.clear()
    gc.collect()
    torch.cuda.empty_cache()


def code(pkg, x):
    return pkg._lib.SD_C128 if x.is_complex() else pkg._lib.SD_F64


def current_into(pkg, m, psi, w, out):
    """out = J_w psi through the C ABI, so that the caller owns (and pre-fills) the output"""
    import torch
    wa = None if w is None else np.ascontiguousarray(w, dtype=np.float64)
    m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    pkg.check(pkg.lib().sd_current_apply_dev(m.ctx.h, m.h, code(pkg, psi), psi.data_ptr(), len(psi),
                                             None if wa is None else wa.ctypes.data_as(_dp), out.data_ptr()), m.ctx.h)
    torch.cuda.synchronize()


def szq_into(pkg, m, psi, q, out):
    import torch
    m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    pkg.check(pkg.lib().sd_szq_dev(m.ctx.h, m.h, code(pkg, psi), psi.data_ptr(), len(psi), float(q), out.data_ptr()), m.ctx.h)
    torch.cuda.synchronize()


def nan_complex(N, dev):
    import torch
    out = torch.empty(N, dtype=torch.complex128, device=dev)
    torch.view_as_real(out).fill_(NAN)
    return out


def differing(sh, got, re, im):
    """which rows differ, for the failure message: count, the first rows and their tiles"""
    bad = (got.real != re) | (got.imag != im)
    first = bad.nonzero().flatten()[:8].tolist()
    return f"{sh.name}: {int(bad.sum())} of {sh.N} rows differ; first rows {first}, tiles {sh.tile_of(first)}"


def assert_crosses_the_caps(sh):
    """the conditions under which the capped grids of the launchers wrap at this shape (constants of the launchers)"""
    if sh.path == 1:
        n_tiles = len(sh.tiles[0])
        assert n_tiles > 4096 and n_tiles > 2048              # k_current tiled: 4096 blocks; k_site_project / k_obs2: 2048
        assert sh.m.device_path == "tiled"
        if sh.name == "Ts":
            assert sh.tiles[1].max() <= 128 and (sh.tiles[1] > 64).any()     # waves 2 and 3 never hold a row, wave 1 does
        else:
            assert sh.tiles[1].max() > 256 and sh.N > 16384 * 256            # the inner loop runs again; k_spin_op: 16384 blocks
    elif sh.path == 0:
        assert sh.m.device_path == "generic"
        assert sh.N > 8192 * 256 and sh.N > 2048 * 256        # k_current / k_szq_generic: 8192 blocks; k_site_chunk / k_obs: 2048
    else:
        assert sh.m.device_path == "full-tiled"
        assert sh.N >= 4 * 8192 * 256 and (sh.N >> 10) > 2048 and sh.N >= 2 * 16384 * 256 and sh.L // 2 > 8


# ---- 1. the spin current, write form: all rows, bit for bit ----
@pytest.mark.parametrize("name", ["T-periodic", "T-open", "Ts", "R-periodic", "R-open", "Rg", "F"])
def test_spin_current_equals_the_row_loop_on_all_rows(pkg, shapes, name):
    import torch
    sh = shapes.get(name)
    assert_crosses_the_caps(sh)
    ref = sh.jref()
    out = nan_complex(sh.N, sh.dev)
    for k, psi in enumerate((sh.psi_r, sh.psi_c)):
        for mi, w in enumerate(sh.wsets):
            torch.view_as_real(out).fill_(NAN)
            current_into(pkg, sh.m, psi, w, out)
            re, im = ref[(k, mi)]
            assert torch.equal(out.real, re) and torch.equal(out.imag, im), (k, mi, differing(sh, out, re, im))
    assert float(ref[(1, 0)][1].abs().max()) > 0.1             # a real comparison, not zeros against zeros
    assert torch.equal(pkg.spin_current(sh.psi_c, sh.m, sh.wsets[2]), out)      # the Python mirror is that very call
    if name in ("T-open", "R-open", "Rg"):                     # no later test uses these
        shapes.drop(name)


def test_spin_current_sampled_rows_past_2_31(pkg):
    """B: L = 34, nup = 17, Float64 psi, 2.33e9 rows (19 GB in, 37 GB out).  The rows of `sample_rows` of
    tests/rows_ref.py -- the first and last 2048, both sides of 300 tile boundaries, 12 000 random ones -- with the
    partners gathered from the device vector.  Its run time on an MI355X has not been measured; the allocations, the fills and
    the plan of the sector make it the one slow case of this module."""
    import torch
    L, nup = 34, 17
    m = pkg.XXZChain(L, nup=nup, boundary="open", **XXZ)
    N = m.N
    assert N > 2 ** 31 and m.device_path == "tiled" and len(m.local_tiles()[0]) > 4096
    gc.collect()
    torch.cuda.empty_cache()                 # what earlier tests left in torch's caching allocator is not "in use" ...
    pkg.default_context().release_scratch()  # ... nor are the work vectors the library's context keeps between calls
    free, _ = torch.cuda.mem_get_info()
    if free < (8 + 16) * N + (3 << 30):
        pytest.skip("not enough device memory")
    dev = torch.device("cuda", m.ctx.device)
    psi = fill_randn(pkg, m, N, False, 20260821)
    rows_np = RR.sample_rows(m, 12000, seed=L * 1000 + nup)
    assert rows_np.max() > 2 ** 31
    rows = torch.from_numpy(rows_np).to(dev)
    s = RR.unrank_t(rows, L, nup)
    assert torch.equal(RR.rank_t(s, L, nup), rows)
    wsets = weight_sets(len(m.hopping_list), L)
    ref = RR.current_rows([psi], wsets, s, rows, L, nup, m.hopping_list)
    out = nan_complex(N, dev)
    for mi, w in enumerate(wsets):
        if mi:
            torch.view_as_real(out).fill_(NAN)
        current_into(pkg, m, psi, w, out)
        got = out[rows]
        re, im = ref[(0, mi)]
        bad = (got.real != re) | (got.imag != im)
        assert not bool(bad.any()), (mi, rows[bad][:8].tolist())
    assert float(ref[(0, 0)][1].abs().max()) > 0.1
    del out, psi
    torch.cuda.empty_cache()


# ---- 2. the spin current, bracket form ----
@pytest.mark.parametrize("name", ["T-periodic", "Ts", "R-periodic", "F"])
def test_current_bracket_probes_and_summation_bound(pkg, shapes, name):
    import torch
    sh = shapes.get(name)
    assert_crosses_the_caps(sh)
    m, ket, ref = sh.m, sh.psi_c, sh.jref()
    # probe brackets: bra = e_r picks (J_w ket)[r]; every other term of the sum is an exact zero
    rows = sh.probe_rows()
    if sh.tiles is not None:
        assert max(sh.tile_of(rows)) >= 4096
    else:
        assert max(rows) >= 8192 * 256
    bra = torch.zeros(sh.N, dtype=torch.float64, device=sh.dev)
    for r in rows:
        bra[r] = 1.0
        for mi, w in enumerate(sh.wsets):
            got = pkg.current_expectation(bra, ket, m, w)
            want = (float(ref[(1, mi)][0][r]), float(ref[(1, mi)][1][r]))
            assert got.real == want[0] and got.imag == want[1], (name, r, sh.tile_of([r]), mi, got, want)
        bra[r] = 0.0
    # random bra and ket against the exactly rounded sum of the per-row products
    t = np.array([x for _, _, x in sh.hop])
    for bra, cases in ((sh.psi_r, (0, 2)), (sh.bra_c(pkg), (1, 2))):
        for mi in cases:
            w = sh.wsets[mi]
            re, im = ref[(1, mi)]
            prod = torch.conj(bra) * torch.complex(re, im) if bra.is_complex() else torch.complex(bra * re, bra * im)
            prod = prod.cpu().numpy()
            want = complex(math.fsum(prod.real.tolist()), math.fsum(prod.imag.tolist()))
            wt = float(np.abs(t * (1.0 if w is None else w)).sum())
            bar = 2 * sh.N * 2.0 ** -53 * float(torch.linalg.vector_norm(bra)) * float(torch.linalg.vector_norm(ket)) * wt
            got = pkg.current_expectation(bra, ket, m, w)
            print(f"{name} bra={'c128' if bra.is_complex() else 'f64'} weights {mi}: {abs(got - want):.2e} (bar {bar:.2e}, |want| {abs(want):.2e})")
            assert abs(got - want) <= bar
            again = pkg.current_expectation(bra, ket, m, w)
            assert got.real.hex() == again.real.hex() and got.imag.hex() == again.imag.hex()     # same call twice: equal bits


# ---- 3. the site projections ----
@pytest.mark.parametrize("name", ["Ts", "T-periodic", "R-periodic", "F"])
def test_site_project_probes_and_random_vectors(pkg, shapes, name):
    import torch
    sh = shapes.get(name)
    assert_crosses_the_caps(sh)
    m, L = sh.m, sh.L
    rows = sh.probe_rows()
    if sh.tiles is not None:
        tl = np.array(sh.tile_of(rows))
        off = np.array(rows) - sh.tiles[0][tl]
        assert (tl >= 2048).any() and ((off >= 64) & (tl >= 2048)).any() and ((off < 64) & (tl >= 2048)).any()    # waves 0 and 1
    else:
        assert max(rows) >= 2048 * (1024 if sh.path == 2 else 256)
    bras = (sh.psi_r, sh.bra_c(pkg))
    ket = torch.zeros(sh.N, dtype=torch.complex128, device=sh.dev)
    for r in rows:
        ket[r] = 1.0
        cfg = sh.config(r)
        sz = np.array([0.5 if (cfg >> i) & 1 else -0.5 for i in range(L)])
        for bra in bras:
            b = complex(bra[r].item())
            got = pkg.site_project(m, bra, ket)
            # conj(bra_r) s_i: one non-zero term per part, and the halving is exact
            assert np.array_equal(got.real, sz * b.real) and np.array_equal(got.imag, sz * -b.imag), (name, r, sh.tile_of([r]), got)
        ket[r] = 0.0
    ket = sh.psi_c
    for bra in bras:
        got = pkg.site_project(m, bra, ket)
        w = torch.conj(bra) * ket if bra.is_complex() else bra * ket
        want = np.array([complex((w * RR.site_sz(sh.s, i)).sum().item()) for i in range(1, L + 1)])
        bar = 1e-13 * float((bra.abs() * ket.abs()).sum().item())
        err = np.abs(got - want).max()
        print(f"{name} bra={'c128' if bra.is_complex() else 'f64'}: {err:.2e} (bar {bar:.2e}, max |want| {np.abs(want).max():.2e})")
        assert got.shape == (L,) and err <= bar
        again = pkg.site_project(m, bra, ket)
        assert np.array_equal(got.view(np.float64), again.view(np.float64))         # same call twice: equal bits


# ---- 4. the observables ----
@pytest.mark.parametrize("name", ["Ts", "T-periodic", "R-periodic", "F"])
def test_observables_probes_and_random_states(pkg, shapes, name, monkeypatch):
    import torch
    monkeypatch.delenv("SD_OBS_CHUNKED", raising=False)
    sh = shapes.get(name)
    assert_crosses_the_caps(sh)
    m, L = sh.m, sh.L
    rows = sh.probe_rows()
    if sh.tiles is not None:
        assert max(sh.tile_of(rows)) >= 2048
    else:
        assert max(rows) >= 2048 * (1024 if sh.path == 2 else 256)
    sz_of = lambda cfg: np.array([0.5 if (cfg >> i) & 1 else -0.5 for i in range(L)])      # noqa: E731
    # one basis state: <S^z_i> = +-1/2 exactly, and its connected correlations vanish exactly
    for cplx in (False, True):
        psi = torch.zeros(sh.N, dtype=torch.complex128 if cplx else torch.float64, device=sh.dev)
        for r in rows:
            psi[r] = 1.0
            assert np.array_equal(pkg.magnetization_per_site(psi, m), sz_of(sh.config(r))), (name, r, sh.tile_of([r]))
            assert np.array_equal(pkg.connected_correlations(psi, m), np.zeros(L)), (name, r)
            psi[r] = 0.0
        # two basis states of unit amplitude each.  The library does not normalise psi, and these probes rely on that: with
        # <psi|psi> = 2 taken as it is, S_i and the lag sums R_r = sum_i s_i s_{i+r} of the two rows add up, all in
        # exact arithmetic (quarters of small integers), and C_r = (R_r - sum_i S_i S_{i+r}) / L rounds once
        for a, b in zip(rows[:-1], rows[1:]):
            psi[a] = psi[b] = 1.0
            S = sz_of(sh.config(a)) + sz_of(sh.config(b))
            R = RR.lag_sums(sh.config(a), L) + RR.lag_sums(sh.config(b), L)
            want = np.array([(R[r] - sum(S[i] * S[(i + r) % L] for i in range(L))) / L for r in range(L)])
            assert np.array_equal(pkg.magnetization_per_site(psi, m), S), (name, a, b)
            assert np.array_equal(pkg.connected_correlations(psi, m), want), (name, a, b, sh.tile_of([a, b]))
            psi[a] = psi[b] = 0.0
    # random states of norm 1
    for x in (sh.psi_r, sh.psi_c):
        psi = x / torch.linalg.vector_norm(x)
        prob = psi.abs() ** 2 if psi.is_complex() else psi * psi
        mag = pkg.magnetization_per_site(psi, m)
        want = np.array([float((prob * RR.site_sz(sh.s, i)).sum().item()) for i in range(1, L + 1)])
        print(f"{name} {'c128' if psi.is_complex() else 'f64'}: magnetization {np.abs(mag - want).max():.2e}")
        assert np.abs(mag - want).max() <= 1e-13
        cr = pkg.connected_correlations(psi, m)
        monkeypatch.setenv("SD_OBS_CHUNKED", "1")
        mag2, cr2 = pkg.magnetization_per_site(psi, m), pkg.connected_correlations(psi, m)
        monkeypatch.delenv("SD_OBS_CHUNKED")
        assert np.abs(mag - mag2).max() <= 1e-13 and np.abs(cr - cr2).max() <= 1e-13
        # ... and against the definition (the per-row plan has the chunked kernels only): C_r = (sum prob R_r(row) - sum_i S_i
        # S_{i+r}) / L.  Both sides sum N positive terms of total <= L/4 in trees of depth ~ log2 N: ~ 1e-15, far inside 1e-13.
        lag = np.array([float((prob * RR.lag_sums_t(sh.s, L, r)).sum().item()) for r in range(L)])
        cdef = np.array([(lag[r] - sum(want[i] * want[(i + r) % L] for i in range(L))) / L for r in range(L)])
        print(f"   connected correlations vs the definition {np.abs(cr - cdef).max():.2e}")
        assert np.abs(cr - cdef).max() <= 1e-13


# ---- 5. S^z_q ----
@pytest.mark.parametrize("name", ["R-periodic", "F", "T-periodic"])
def test_szq_equals_the_row_loop_on_all_rows(pkg, shapes, name, monkeypatch):
    import torch
    monkeypatch.delenv("SD_SZQ_FULL_GENERIC", raising=False)
    sh = shapes.get(name)
    assert_crosses_the_caps(sh)
    out = nan_complex(sh.N, sh.dev)
    for psi in (sh.psi_r, sh.psi_c):
        for q in (0.3, 2 * np.pi * 5 / sh.L):
            want = RR.szq_rows(psi, sh.s, sh.L, q)
            torch.view_as_real(out).fill_(NAN)
            szq_into(pkg, sh.m, psi, q, out)
            err, top = float((out - want).abs().max()), float(want.abs().max())
            print(f"{name} {'c128' if psi.is_complex() else 'f64'} q={q:.3f}: {err:.2e} (max |want| {top:.2e})")
            assert err <= 1e-15 * max(1.0, top)                 # (a NaN left in `out` fails this too)
            assert top > 0.1                                     # a real comparison, not zeros against zeros
            if sh.path == 2:                                    # k_szq_full (k = 11) and the row loop kernel: equal bits
                monkeypatch.setenv("SD_SZQ_FULL_GENERIC", "1")
                gen = nan_complex(sh.N, sh.dev)
                szq_into(pkg, sh.m, psi, q, gen)
                monkeypatch.delenv("SD_SZQ_FULL_GENERIC")
                assert torch.equal(torch.view_as_real(out), torch.view_as_real(gen))
                del gen


# ---- 6. create_spin_operator ----
@pytest.mark.parametrize("site", [1, 12, 25])
def test_spin_operator_z_in_a_sector_past_16384_blocks(pkg, shapes, site):
    sh = shapes.get("T-periodic")
    assert_crosses_the_caps(sh)
    assert site <= sh.L and sh.N > 16384 * 256
    op = pkg.create_spin_operator(site, "z")
    for psi in (sh.psi_r, sh.psi_c):
        want = (RR.site_sz(sh.s, site) * psi).cpu().numpy()      # +-0.5 psi[row]: exact
        got = op(psi.cpu().numpy(), sh.m)
        assert got.dtype == want.dtype and np.array_equal(got, want)


@pytest.mark.parametrize("op", ["plus", "minus", "x", "y"])
def test_spin_operators_on_the_full_basis_past_16384_blocks(pkg, shapes, op):
    sh = shapes.get("F")
    assert_crosses_the_caps(sh)
    for site in (1, 12, sh.L):
        f = pkg.create_spin_operator(site, op)
        for psi in ((sh.psi_c,) if op == "y" else (sh.psi_r, sh.psi_c)):
            want = RR.spin_operator_rows(psi, site, op).cpu().numpy()
            got = f(psi.cpu().numpy(), sh.m)
            assert got.dtype == want.dtype
            bad = np.nonzero(got != want)[0]
            assert len(bad) == 0, (op, site, len(bad), bad[:8].tolist())
