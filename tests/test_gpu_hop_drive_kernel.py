"""k_hop_drive_epilogue (csrc/kernels_hop_drive.hip) through sd_driven_hop_apply_dev, its host twin and sd_hop_apply_dev, Float64 and
ComplexF64, on random vectors: bit for bit against tests/hopdrive_ref.py (with tests/driven_ref.py for the diagonal part) applied to
H0 psi.  H0 psi is the apply's own pinned bits: the CPU oracle's at the small shapes (tests/test_gpu_apply.py pins the apply to it
bit for bit), the library's apply on the device at the large ones, where every row is restated with torch on the device.

Shapes.  Every row at  L = 12 nup = 6,  L = 10 nup = 1 (both tiled plans),  L = 7 full basis,  L = 14 nup = 1 (per-row plan);  and the shapes
at which the capped grids wrap -- T: L = 25 nup = 12 (8191 tiles > SD_HOP_TILE_BLOCKS), R: L = 39 nup = 6 and F: L = 23 full basis (more
than SD_HOP_ROW_BLOCKS blocks of 256 rows); each test first asserts that its shape crosses the launcher's own constants, read from
the source.

Lists (small shapes): the chain; (1, L) and (L, 1); a repeated bond; second neighbours; every (k, k + 1), (k, k + 2) and (1, L), which
for any prefix length p holds a bond inside the prefix, one inside the suffix and the ones straddling p; K + KH = 3 with a zero
coefficient; hopping and diagonal drives together.  Real lists run on Float64 and ComplexF64 vectors, complex lists on ComplexF64.

SD_EPI_DOT is reached through a one-stage stage_evolve with kry_m = 1, as tests/test_gpu_drive_kernel.py reaches it.

Cross-checks against kernels already pinned, each within (n_terms + 2) 2^-53 sum |weights| max |psi| per element, the forward bound of
a sequential sum: hopping_apply(current_drive) against spin_current, hopping_apply against operator_apply of the same terms.
Measured on an MI355X: difference 0.0 in both at all four small shapes (bounds 9e-15 ... 1e-13); SD_EPI_DOT largest error / bar
1.2e-3 at N = 924, 5.7e-3 at N = 128, 4e-7 past the caps."""
import math
import os
import re

import numpy as np
import pytest

import driven_ref as DR
import hopdrive_ref as HR
import rows_ref as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
XXZ = dict(Jxy=0.8, Jz=0.7, hz=0.3)
SMALL = {"S12": (12, 6, 1), "S10": (10, 1, 1), "S7": (7, None, 0), "S14": (14, 1, 0)}
LARGE = {"T": (25, 12, 1), "R": (39, 6, 0), "F": (23, None, 2)}
U = 2.0 ** -53


def caps():
    src = open(os.path.join(ROOT, "spindynamics.jl_amd", "csrc", "kernels_hop_drive.hip")).read()
    return tuple(int(re.search(r"#define %s (\d+)" % n, src).group(1)) for n in ("SD_HOP_TILE_BLOCKS", "SD_HOP_ROW_BLOCKS"))


def small_sets(L, seed):
    """name -> (hopping drives as hopdrive_ref tuples, diagonal drives as driven_ref tuples, coefficients: diagonal ones first)"""
    rng = np.random.default_rng(seed)
    rz = lambda n: rng.standard_normal(n)                                                    # noqa: E731
    cz = lambda n: rng.standard_normal(n) + 1j * rng.standard_normal(n)                      # noqa: E731
    chain = [(i, i + 1) for i in range(1, L)]
    second = [(i, i + 2) for i in range(1, L - 1)]
    mixed = [(1, L), (L, 1), (2, 1), (1, 2), (1, 2), (3, 1), (L, L - 2), (L // 2, L // 2 + 1)]
    w1 = rng.standard_normal(L)
    return {
        "chain real": ([(chain, rz(L - 1))], [], [0.7]),
        "chain complex": ([(chain, cz(L - 1))], [], [-1.3]),
        "ends and repeats real": ([(mixed, rz(len(mixed)))], [], [0.9]),
        "ends and repeats complex": ([(mixed, cz(len(mixed)))], [], [0.45]),
        "all near pairs complex": ([(chain + second + [(1, L)], cz(2 * L - 2))], [], [0.6]),
        "second real": ([(second, rz(L - 2))], [], [1.2]),
        "K3 zero complex": ([(chain, cz(L - 1)), (second, rz(L - 2)), ([(L, 1), (2, 1)], [0.5, 0.25j])], [], [0.9, 0.0, -0.35]),
        "with diagonal real": ([(chain + [(L, 1)], rz(L))], [(w1, [(1, 2), (L, 2)], [0.3, -0.8])], [0.45, 0.8]),
        "with diagonal complex": ([(second, cz(L - 2)), (chain, rz(L - 1))], [(None, chain, list(rz(L - 1)))], [-0.6, 0.0, 1.1]),
    }


def to_pkg(pkg, hops, diags):
    """(the package's drive list with the hopping drives FIRST, the permutation that puts a diagonal-first coefficient list in that order)"""
    lst = [pkg.HoppingDrive(b, w) for (b, w) in hops] + [pkg.DiagonalDrive(site_weights=w, bonds=b, bond_weights=v) for (w, b, v) in diags]
    K, KH = len(diags), len(hops)
    return lst, list(range(K, K + KH)) + list(range(K))


def randn(rng, N, cplx):
    x = rng.standard_normal(N)
    return x + 1j * rng.standard_normal(N) if cplx else x


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.float64), np.ascontiguousarray(b).view(np.float64))


def restate(h, psi, s, parts, hops, diags, coefs, L):
    """h + d(s) psi + B psi by the two restatements; coefs: the diagonal drives' first"""
    K = len(diags)
    cf, el = HR.effective_list(hops, coefs[K:])
    acc = h
    if K:
        acc = DR.drive_rows(h, psi, DR.diag_values(s, L, DR.effective_weights(L, diags, coefs[:K])))
    return HR.hop_rows(acc, psi, s, parts(el), el, cf)


# ---- every row at the small shapes ----
@pytest.mark.parametrize("name", list(SMALL))
def test_every_row_small_shapes(pkg, O, name):
    import torch
    L, nup, path = SMALL[name]
    m, r = pkg.XXZChain(L, nup=nup, **XXZ), O.XXZChain(L, nup=nup, **XXZ)
    assert pkg.lib().sd_model_path(m.h) == path
    dev = torch.device("cuda", m.ctx.device)
    s = np.asarray(m.states).astype(np.int64)
    idx = np.arange(m.N, dtype=np.int64)
    parts = lambda el: HR.partner_rows(s, idx, el, None if nup is None else (lambda c: m.rank(c.astype(np.uint64))))   # noqa: E731
    rng = np.random.default_rng(200 + L)
    sets = small_sets(L, L)
    assert len(sets) == 9
    for cplx in (False, True):
        psi, y = randn(rng, m.N, cplx), randn(rng, m.N, cplx)
        h0 = O.apply_H(r, psi)
        tp, ty = torch.as_tensor(psi, device=dev), torch.as_tensor(y, device=dev)
        hdev = torch.empty_like(tp)
        pkg.apply_H(hdev, tp, m)
        assert np.array_equal(hdev.cpu().numpy(), h0)                       # the apply's bits are the oracle's
        for key, (hops, diags, coefs) in sets.items():
            lst, perm = to_pkg(pkg, hops, diags)
            pc = [coefs[k] for k in perm]                                   # the caller's order: hopping drives first
            if not cplx and "complex" in key:
                with pytest.raises(pkg.ArgumentError):                      # a complex-form list on a Float64 vector
                    pkg.driven_apply(torch.empty_like(tp), tp, m, lst, pc)
                with pytest.raises(pkg.ArgumentError):
                    pkg.hopping_apply(tp, m, lst[:len(hops)], coefs[len(diags):])
                continue
            want = restate(h0, psi, s, parts, hops, diags, coefs, L)
            out = torch.full_like(tp, float("nan"))
            pkg.driven_apply(out, tp, m, lst, pc)
            got = out.cpu().numpy()
            assert same_bits(got, want), (name, cplx, key, np.abs(got - want).max())
            assert np.abs(want - h0).max() > 0.01                           # the drives did something
            # the host-pointer entry gives the same bits
            assert same_bits(pkg.driven_apply(np.empty_like(psi), psi, m, lst, pc), want), (name, cplx, key)
            # B psi alone, B psi + y, and y = out in place
            hp, hc = lst[:len(hops)], coefs[len(diags):]
            got = pkg.hopping_apply(tp, m, hp, hc).cpu().numpy()
            assert same_bits(got, restate(None, psi, s, parts, hops, [], hc, L)), (name, cplx, key)
            wy = restate(y, psi, s, parts, hops, [], hc, L)
            assert same_bits(pkg.hopping_apply(tp, m, hp, hc, y=ty).cpu().numpy(), wy), (name, cplx, key)
            buf = ty.clone()
            pkg.hopping_apply(tp, m, hp, hc, y=buf, out=buf)
            assert same_bits(buf.cpu().numpy(), wy), (name, cplx, key)
            assert same_bits(pkg.hopping_apply(psi, m, hp, hc, y=y), wy)
    # hopping coefficients all zero: the diagonal entry's bits; no drive in effect at all: H0 psi
    e, g = pkg.exchange_drive(m), pkg.gradient_drive(m)
    a, b = torch.empty_like(tp), torch.empty_like(tp)
    pkg.driven_apply(a, tp, m, [e, g], [0.0, 0.7])
    pkg.driven_apply(b, tp, m, [g], [0.7])
    assert torch.equal(torch.view_as_real(a), torch.view_as_real(b))
    with pytest.raises(pkg.ArgumentError):
        pkg.driven_apply(tp, tp, m, [e], [1.0])                             # out must not alias psi
    with pytest.raises(pkg.ArgumentError):
        pkg.hopping_apply(tp, m, [e], [1.0], y=tp)                          # nor may y
    with pytest.raises(pkg.ArgumentError):
        pkg.hopping_apply(tp, m, [pkg.HoppingDrive([(1, 1)])], [1.0])
    with pytest.raises(pkg.DimensionMismatch):
        pkg.check(pkg.lib().sd_hop_apply_dev(m.ctx.h, m.h, 2, tp.data_ptr(), m.N - 1, None, 0, None, None, a.data_ptr()), m.ctx.h)


# ---- the wrap rows: all rows at the shapes whose grids are capped ----
def prefix_sites(m, L, nup):
    """p of a tiled sector plan, from its tiles: the prefixes P < 2^p with nup - (L - p) <= popcount(P) <= nup, one tile each"""
    n_tiles = len(m.local_tiles()[0])
    fits = [p for p in range(1, L) if sum(math.comb(p, j) for j in range(max(0, nup - (L - p)), min(p, nup) + 1)) == n_tiles]
    assert len(fits) == 1, fits
    return fits[0]


class Big:
    def __init__(self, pkg, name):
        import torch
        self.L, self.nup, self.path = LARGE[name]
        L = self.L
        self.m = pkg.XXZChain(L, nup=self.nup, boundary="open", **XXZ)
        assert pkg.lib().sd_model_path(self.m.h) == self.path
        self.dev = torch.device("cuda", self.m.ctx.device)
        self.N = self.m.N
        self.rows = torch.arange(self.N, dtype=torch.int64, device=self.dev)
        self.s = RR.configurations_t(self.rows, L, self.nup)
        self.psi = {}
        for cplx in (False, True):
            x = torch.empty(self.N, dtype=torch.complex128 if cplx else torch.float64, device=self.dev)
            self.m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            pkg.check(pkg.lib().sd_fill_randn_dev(self.m.ctx.h, x.data_ptr(), (2 if cplx else 1) * self.N, 919 + L, 0), self.m.ctx.h)
            self.psi[cplx] = x
        p = prefix_sites(self.m, L, self.nup) if self.path == 1 else L // 2
        assert 2 <= p <= L - 2
        self.bonds = [(1, 2), (L - 1, L), (p, p + 1), (L, 1)]               # inside the prefix, inside the suffix, straddling p, the ends
        rng = np.random.default_rng(L)
        self.real = (self.bonds, rng.standard_normal(4))
        self.cplx = (self.bonds, rng.standard_normal(4) + 1j * rng.standard_normal(4))
        self.diag = (rng.standard_normal(L), [(1, 2), (L, 2)], [0.3, -0.8])

    def parts(self, el):
        rank = None if self.nup is None else (lambda c: RR.rank_t(c, self.L, self.nup))
        return HR.partner_rows(self.s, self.rows, el, rank)

    def crosses(self):
        tile_cap, row_cap = caps()
        if self.path == 1:
            n_tiles = len(self.m.local_tiles()[0])
            assert n_tiles > tile_cap and self.m.device_path == "tiled", (n_tiles, tile_cap)
        else:
            assert (self.N + 255) // 256 > row_cap, (self.N, row_cap)


@pytest.fixture(scope="module")
def bigs(pkg):
    import gc
    import torch
    store = {}

    def get(name):
        if name not in store:
            store.clear()
            gc.collect()
            torch.cuda.empty_cache()
            store[name] = Big(pkg, name)
        return store[name]
    yield get
    store.clear()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.mark.parametrize("name", list(LARGE))
def test_all_rows_where_the_grid_wraps(pkg, bigs, name):
    import torch
    b = bigs(name)
    b.crosses()
    m, L = b.m, b.L
    for cplx, hop, diags, coefs in ((True, b.cplx, [b.diag], [0.45, 0.8]), (True, b.real, [], [1.1]), (False, b.real, [b.diag], [-0.7, 0.6])):
        psi = b.psi[cplx]
        h0 = torch.empty_like(psi)
        pkg.apply_H(h0, psi, m)                                             # pinned where its own grids wrap by the apply's tests
        lst, perm = to_pkg(pkg, [hop], diags)
        out = torch.full_like(psi, float("nan"))
        pkg.driven_apply(out, psi, m, lst, [coefs[k] for k in perm])
        want = restate(h0, psi, b.s, b.parts, [hop], diags, coefs, L)
        bad = (torch.view_as_real(out) != torch.view_as_real(want)).any(-1) if cplx else (out != want)
        assert not bool(bad.any()), (name, cplx, int(bad.sum()), bad.nonzero().flatten()[:8].tolist())
        assert float((want - h0).abs().max()) > 0.01
        del out, want, bad
        got = pkg.hopping_apply(psi, m, lst[:1], coefs[len(diags):])
        want = restate(None, psi, b.s, b.parts, [hop], [], coefs[len(diags):], L)
        assert torch.equal(torch.view_as_real(got), torch.view_as_real(want)) if cplx else torch.equal(got, want), (name, cplx)
        del got, want, h0


# ---- SD_EPI_DOT ----
def alpha_check(pkg, m, s, parts, psi, h0, hop, diags, coefs, L, label):
    """alpha = <v|(H0 + D + B)v> from the phase of a one-stage, kry_m = 1 evolution against the exactly rounded sum of the row products"""
    import torch
    is_t = DR._is_torch(psi)
    nrm = float(torch.linalg.vector_norm(psi)) if is_t else float(np.linalg.norm(psi))
    v = psi / nrm
    hv = restate(h0 / nrm, v, s, parts, [hop], diags, coefs, L)             # (H0 + D + B) v up to an ulp per row (the scaling)
    prod = (torch.conj(v) * hv if is_t else np.conj(v) * hv)
    terms = (prod.real.cpu().numpy() if is_t else np.asarray(prod.real)).tolist()
    want, mag, n = math.fsum(terms), math.fsum(abs(t) for t in terms), len(terms)
    bound = sum(abs(J) for _i, _j, J in m.hopping_list) + sum(abs(J) for _i, _j, J in m.zz_list) / 4 + np.abs(m.onsite_field).sum() / 2
    for c, (w, _b, vv) in zip(coefs, diags):
        bound += abs(c) * ((0 if w is None else np.abs(w).sum() / 2) + np.abs(vv).sum() / 4)
    bound += abs(coefs[-1]) * float(np.abs(np.asarray(hop[1])).sum())
    tau = 1.0 / bound                                                       # |alpha| tau <= 1 < pi
    lst, perm = to_pkg(pkg, [hop], diags)
    out, info = pkg.stage_evolve(m, psi, lst, [tau], [[coefs[k] for k in perm]], kry_m=1, return_info=True)
    assert info["stages"] == 1 and info["applies"] == 1
    z = complex(torch.vdot(v.to(out.dtype), out)) if is_t else complex(np.vdot(v, out))
    assert abs(abs(z) - 1) <= 1e-13
    got = -math.atan2(z.imag, z.real) / tau
    bar = n * 2.0 ** -53 * mag
    print(f"{label}: alpha {got:.15g} want {want:.15g} diff {abs(got - want):.2e} bar {bar:.2e}")
    assert abs(got - want) <= bar, (label, got, want, bar)


@pytest.mark.parametrize("name", ["S12", "S7"])
def test_dot_epilogue_small(pkg, O, name):
    L, nup, _ = SMALL[name]
    m, r = pkg.XXZChain(L, nup=nup, **XXZ), O.XXZChain(L, nup=nup, **XXZ)
    assert m.N >= 128
    s = np.asarray(m.states).astype(np.int64)
    idx = np.arange(m.N, dtype=np.int64)
    parts = lambda el: HR.partner_rows(s, idx, el, None if nup is None else (lambda c: m.rank(c.astype(np.uint64))))   # noqa: E731
    rng = np.random.default_rng(17 + L)
    sets = small_sets(L, L)
    for cplx, key in ((False, "with diagonal real"), (True, "chain complex"), (True, "ends and repeats real")):
        hops, diags, coefs = sets[key]
        psi = randn(rng, m.N, cplx)
        alpha_check(pkg, m, s, parts, psi, O.apply_H(r, psi), hops[0], diags, coefs, L, f"{name} {'c128' if cplx else 'f64'} {key}")


@pytest.mark.parametrize("name", list(LARGE))
def test_dot_epilogue_where_the_grid_wraps(pkg, bigs, name):
    import torch
    b = bigs(name)
    b.crosses()
    for cplx, hop, diags, coefs in ((True, b.cplx, [b.diag], [0.45, 0.8]), (False, b.real, [], [1.1])):
        psi = b.psi[cplx]
        h0 = torch.empty_like(psi)
        pkg.apply_H(h0, psi, b.m)
        alpha_check(pkg, b.m, b.s, b.parts, psi, h0, hop, diags, coefs, b.L, f"{name} {'c128' if cplx else 'f64'}")


# ---- cross-checks against kernels already pinned ----
@pytest.mark.parametrize("name", ["S12", "S10", "S7", "S14"])
def test_against_spin_current_and_operator_strings(pkg, name):
    import torch
    L, nup, _ = SMALL[name]
    rng = np.random.default_rng(31 + L)
    hop = [(i, i + 1, 0.4 + 0.05 * i) for i in range(1, L)] + [(L, 1, -0.3), (1, 3, 0.2), (4, 2, 0.6)]
    m = pkg.Model(L, nup=nup, hopping=hop, zz=[(i, i + 1, 0.7) for i in range(1, L)])
    dev = torch.device("cuda", m.ctx.device)
    psi = torch.as_tensor(randn(rng, m.N, True), device=dev)
    w = rng.standard_normal(len(hop))
    cd = pkg.current_drive(m, weights=w)
    got = pkg.hopping_apply(psi, m, [cd], [1.0])
    want = pkg.spin_current(psi, m, weights=w)
    bound = (len(hop) + 2) * U * float(np.abs(cd.weights).sum()) * float(psi.abs().max())
    err = float((got - want).abs().max())
    print(f"{name}: current {err:.2e} bound {bound:.2e}")
    assert float(want.abs().max()) > 0.1 and err <= bound
    # the same terms as operator strings
    z = rng.standard_normal(len(hop)) + 1j * rng.standard_normal(len(hop))
    hd = pkg.HoppingDrive([(i, j) for (i, j, _t) in hop], z)
    terms = []
    for (i, j, _t), zb in zip(hop, z):
        terms += pkg.op_string(0.8 * zb, ("+", i), ("-", j)) + pkg.op_string(np.conj(0.8 * zb), ("-", i), ("+", j))
    got = pkg.hopping_apply(psi, m, [hd], [0.8])
    want = pkg.operator_apply(psi, m, terms)
    bound = (len(hop) + 2) * U * float(np.abs(0.8 * z).sum()) * float(psi.abs().max())
    err = float((got - want).abs().max())
    print(f"{name}: operator strings {err:.2e} bound {bound:.2e}")
    assert float(want.abs().max()) > 0.1 and err <= bound
