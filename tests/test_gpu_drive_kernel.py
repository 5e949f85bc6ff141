"""k_drive_epilogue (csrc/kernels_drive.hip) through sd_driven_apply_dev and sd_diag_apply_dev, Float64 and ComplexF64, on random
vectors: bit for bit against tests/driven_ref.py -- h + d(s) psi with d(s) in the contract's order -- applied to H0 psi.  H0 psi is
the apply's own pinned bits: the CPU oracle's at the small shapes (tests/test_gpu_apply.py pins the apply to it bit for bit), the
library's apply on the device at the large ones, where every row is restated with torch on the device.

Shapes.  Every row at  L = 12 nup = 6,  L = 10 nup = 1 (both tiled plans),  L = 7 full basis,  L = 14 nup = 1 (per-row plan);  and the shapes of
tests/test_gpu_operator_grids.py at which the capped grids wrap -- T: L = 25 nup = 12 (8191 tiles > SD_DRIVE_TILE_BLOCKS), R: L = 39
nup = 6 and F: L = 23 full basis (more than SD_DRIVE_ROW_BLOCKS blocks of 256 rows); each test first asserts that its shape crosses
the launcher's own constants, read from the source.

Weights: site weights only; bonds only (the list starts inside the prefix, so a tiled plan takes the per-tile head); both; K = 3
with a repeated bond and a zero coefficient; two drives without any site list.

SD_EPI_DOT is reached through a one-stage stage_evolve with kry_m = 1, whose result is psi0 e^{-i alpha tau} with
alpha = <v|(H0 + D)v>, v = psi0/|psi0|: alpha is read off the phase (tau |H0 + D| < 1, so nothing wraps) and compared with math.fsum of
the per-row products under n 2^-53 sum |term|.  The phase carries a few ulp of its own (the cosine and sine, the normalisation, the
dot product that reads it back: ~1e-15 / tau), which is why this check runs where n >= 128."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import driven_ref as DR
import rows_ref as RR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_dp = C.POINTER(C.c_double)
XXZ = dict(Jxy=0.8, Jz=0.7, hz=0.3)
# L, nup, sd_model_path: 1 tiled (at L = 10, nup = 1 tiles of at most 10 rows), 0 per row -- the full basis below 12 sites, and the
# dilute sector L = 14, nup = 1, whose tiles would be too short (the plan then ranks and unranks per row)
SMALL = {"S12": (12, 6, 1), "S10": (10, 1, 1), "S7": (7, None, 0), "S14": (14, 1, 0)}
LARGE = {"T": (25, 12, 1), "R": (39, 6, 0), "F": (23, None, 2)}


def caps():
    src = open(os.path.join(ROOT, "spindynamics.jl_amd", "csrc", "kernels_drive.hip")).read()
    return tuple(int(re.search(r"#define %s (\d+)" % n, src).group(1)) for n in ("SD_DRIVE_TILE_BLOCKS", "SD_DRIVE_ROW_BLOCKS"))


def weight_sets(L, seed):
    """name -> (drives as driven_ref tuples, coefficients)"""
    rng = np.random.default_rng(seed)
    w1, w2 = rng.standard_normal(L), rng.standard_normal(L)
    chain = [(i, i + 1) for i in range(1, L)]
    mixed = [(1, 2), (2, 3), (1, 3), (1, L), (L, 2), (L - 1, L), (L - 2, L), (3, L - 1)]
    return {
        "sites": ([(w1, [], [])], [0.7]),
        "bonds": ([(None, chain + mixed, list(rng.standard_normal(len(chain) + len(mixed))))], [-1.3]),
        "both": ([(w1, mixed, list(rng.standard_normal(len(mixed))))], [0.45]),
        "K3": ([(w1, [(1, 2), (4, 5)], [0.3, -0.8]), (w2, [(2, 1), (1, 2), (L, 1)], [1.1, 0.6, -0.2]), (None, chain, [1.0] * (L - 1))],
               [0.9, 0.0, -0.35]),
        "nosites": ([(None, [(2, 3), (1, L)], [0.5, 1.5]), (None, chain, list(rng.standard_normal(L - 1)))], [1.25, 0.0]),
    }


def to_pkg(pkg, drives):
    return [pkg.DiagonalDrive(site_weights=w, bonds=b, bond_weights=v) for (w, b, v) in drives]


def randn(rng, N, cplx):
    x = rng.standard_normal(N)
    return x + 1j * rng.standard_normal(N) if cplx else x


# ---- every row at the small shapes ----
@pytest.mark.parametrize("name", list(SMALL))
def test_every_row_small_shapes(pkg, O, name):
    import torch
    L, nup, path = SMALL[name]
    m, r = pkg.XXZChain(L, nup=nup, **XXZ), O.XXZChain(L, nup=nup, **XXZ)
    assert pkg.lib().sd_model_path(m.h) == path
    dev = torch.device("cuda", m.ctx.device)
    s = np.asarray(m.states).astype(np.int64)
    rng = np.random.default_rng(100 + L)
    sets = weight_sets(L, L)
    assert set(sets) == {"sites", "bonds", "both", "K3", "nosites"}
    for cplx in (False, True):
        psi = randn(rng, m.N, cplx)
        y = randn(rng, m.N, cplx)
        h0 = O.apply_H(r, psi)
        tp, ty = torch.as_tensor(psi, device=dev), torch.as_tensor(y, device=dev)
        hdev = torch.empty_like(tp)
        pkg.apply_H(hdev, tp, m)
        assert np.array_equal(hdev.cpu().numpy(), h0)                       # the apply's bits are the oracle's
        for key, (drives, coefs) in sets.items():
            d = DR.diag_values(s, L, DR.effective_weights(L, drives, coefs))
            pd = to_pkg(pkg, drives)
            out = torch.full_like(tp, float("nan"))
            pkg.driven_apply(out, tp, m, pd, coefs)
            want = DR.drive_rows(h0, psi, d)
            got = out.cpu().numpy()
            assert np.array_equal(got.view(np.float64), want.view(np.float64)), (name, cplx, key, np.abs(got - want).max())
            assert np.abs(want - h0).max() > 0.01                           # the drive did something
            # the host-pointer entry gives the same bits
            assert np.array_equal(pkg.driven_apply(np.empty_like(psi), psi, m, pd, coefs).view(np.float64), want.view(np.float64))
            # D psi alone, D psi + y, and y = out in place
            got = pkg.diagonal_apply(tp, m, pd, coefs).cpu().numpy()
            assert np.array_equal(got.view(np.float64), DR.drive_rows(None, psi, d).view(np.float64)), (name, cplx, key)
            wy = DR.drive_rows(y, psi, d)
            got = pkg.diagonal_apply(tp, m, pd, coefs, y=ty).cpu().numpy()
            assert np.array_equal(got.view(np.float64), wy.view(np.float64)), (name, cplx, key)
            buf = ty.clone()
            pkg.diagonal_apply(tp, m, pd, coefs, y=buf, out=buf)
            assert np.array_equal(buf.cpu().numpy().view(np.float64), wy.view(np.float64)), (name, cplx, key)
            assert np.array_equal(pkg.diagonal_apply(psi, m, pd, coefs, y=y).view(np.float64), wy.view(np.float64))
    # no drives at all: H0 psi, and zeros
    out = torch.empty_like(tp)
    pkg.driven_apply(out, tp, m, [], [])
    assert np.array_equal(out.cpu().numpy(), h0)
    with pytest.raises(pkg.ArgumentError):
        pkg.driven_apply(tp, tp, m, [], [])                                 # out must not alias psi
    with pytest.raises(pkg.ArgumentError):
        pkg.diagonal_apply(tp, m, [pkg.DiagonalDrive(bonds=[(1, 1)])], [1.0])


# ---- the wrap rows: all rows at the shapes whose grids are capped ----
class Big:
    def __init__(self, pkg, name):
        import torch
        self.L, self.nup, self.path = LARGE[name]
        self.m = pkg.XXZChain(self.L, nup=self.nup, boundary="open", **XXZ)
        assert pkg.lib().sd_model_path(self.m.h) == self.path
        self.dev = torch.device("cuda", self.m.ctx.device)
        self.N = self.m.N
        rows = torch.arange(self.N, dtype=torch.int64, device=self.dev)
        self.s = RR.configurations_t(rows, self.L, self.nup)
        self.psi = {}
        for cplx in (False, True):
            x = torch.empty(self.N, dtype=torch.complex128 if cplx else torch.float64, device=self.dev)
            self.m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            pkg.check(pkg.lib().sd_fill_randn_dev(self.m.ctx.h, x.data_ptr(), (2 if cplx else 1) * self.N, 909 + self.L, 0), self.m.ctx.h)
            self.psi[cplx] = x
        self.sets = weight_sets(self.L, self.L)

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
    for cplx, keys in ((True, ("both", "bonds")), (False, ("K3", "sites"))):
        psi = b.psi[cplx]
        h0 = torch.empty_like(psi)
        pkg.apply_H(h0, psi, m)                                             # pinned where its own grids wrap by the apply's tests
        for key in keys:
            drives, coefs = b.sets[key]
            d = DR.diag_values(b.s, L, DR.effective_weights(L, drives, coefs))
            pd = to_pkg(pkg, drives)
            out = torch.full_like(psi, float("nan"))
            pkg.driven_apply(out, psi, m, pd, coefs)
            want = DR.drive_rows(h0, psi, d)
            bad = (torch.view_as_real(out) != torch.view_as_real(want)).any(-1) if cplx else (out != want)
            assert not bool(bad.any()), (name, cplx, key, int(bad.sum()), bad.nonzero().flatten()[:8].tolist())
            assert float((want - h0).abs().max()) > 0.01
        drives, coefs = b.sets["nosites"]
        d = DR.diag_values(b.s, L, DR.effective_weights(L, drives, coefs))
        got = pkg.diagonal_apply(psi, m, to_pkg(pkg, drives), coefs)
        want = DR.drive_rows(None, psi, d)
        assert torch.equal(torch.view_as_real(got), torch.view_as_real(want)) if cplx else torch.equal(got, want), (name, cplx)


# ---- SD_EPI_DOT ----
def alpha_check(pkg, m, s, psi, h0, drives, coefs, L, label):
    """alpha = <v|(H0 + D)v> from the phase of a one-stage, kry_m = 1 evolution against the exactly rounded sum of the row products"""
    import torch
    is_t = DR._is_torch(psi)
    d = DR.diag_values(s, L, DR.effective_weights(L, drives, coefs))
    nrm = float(torch.linalg.vector_norm(psi)) if is_t else float(np.linalg.norm(psi))
    v = psi / nrm
    hv = DR.drive_rows(h0 / nrm, v, d)                                      # (H0 + D) v up to an ulp per row (the scaling)
    prod = (torch.conj(v) * hv if is_t else np.conj(v) * hv)
    terms = (prod.real.cpu().numpy() if is_t else np.asarray(prod.real)).tolist()
    want, mag, n = math.fsum(terms), math.fsum(abs(t) for t in terms), len(terms)
    bound = sum(abs(J) for _i, _j, J in m.hopping_list) + sum(abs(J) for _i, _j, J in m.zz_list) / 4 + np.abs(m.onsite_field).sum() / 2
    for c, (w, _b, vv) in zip(coefs, drives):
        bound += abs(c) * ((0 if w is None else np.abs(w).sum() / 2) + np.abs(vv).sum() / 4)
    tau = 1.0 / bound                                                       # |alpha| tau <= 1 < pi
    out, info = pkg.stage_evolve(m, psi, to_pkg(pkg, drives), [tau], [coefs], kry_m=1, return_info=True)
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
    rng = np.random.default_rng(7 + L)
    sets = weight_sets(L, L)
    for cplx, key in ((False, "both"), (True, "K3"), (True, "bonds")):
        psi = randn(rng, m.N, cplx)
        alpha_check(pkg, m, s, psi, O.apply_H(r, psi), *sets[key], L, f"{name} {'c128' if cplx else 'f64'} {key}")


@pytest.mark.parametrize("name", list(LARGE))
def test_dot_epilogue_where_the_grid_wraps(pkg, bigs, name):
    import torch
    b = bigs(name)
    b.crosses()
    for cplx, key in ((True, "both"), (False, "nosites")):
        psi = b.psi[cplx]
        h0 = torch.empty_like(psi)
        pkg.apply_H(h0, psi, b.m)
        alpha_check(pkg, b.m, b.s, psi, h0, *b.sets[key], b.L, f"{name} {'c128' if cplx else 'f64'} {key}")
