"""Lattice symmetry operators: sd_symmetry_apply / _overlaps / _project, their Python mirror and what is built on
them, against tests/symmetry_ref.py (proven on the CPU by tests/test_symmetry_ref_host.py), formed with torch on the device over ALL
rows.

The write form is a permutation and is compared exactly.  Bars of the sums:
  overlaps   |got - ref| <= 1e-12 |bra| |ket| elementwise: sums of at most N bounded products, blocked -- the pair tests' bar and argument;
  projector  max norm <= 1e-13 |psi|: at most 4 L <= 64 terms of modulus <= |c_g| |psi|_max per row, sum |c_g| = 1.
Small shapes are those of tests/test_gpu_pair_correlations.py (every shape asserts its row mode), the grid-wrap shapes those of
tests/test_gpu_operator_grids.py plus
  Zs  XXZ L = 22, nup = 11, SD_SUFFIX_BITS = 8: 16 172 tiles of at most 70 rows, 705 432 rows -- the smallest half-filled even-L tiled
      shape with more tiles than the write form's 4096 workgroups (L = 20 has 4070 tiles with 8 suffix sites, and 1 with 12): Z in a
      sector where the grid wraps."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

import rows_ref as RR
import symmetry_ref as SR
from test_gpu_operator_grids import NAN, XXZ, Shapes, assert_crosses_the_caps, fill_randn
from test_gpu_pair_correlations import SMALL, build, norm2

pytestmark = pytest.mark.gpu

_dp, _ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
SD_EARG = 1
# the launchers' constants (kernels_symmetry.hip)
SYM_TILE_BLOCKS, SYM_ROW_BLOCKS, SYM_RED_BLOCKS, SYM_CHUNK = 4096, 8192, 2048, 8


def code_of(g):
    return int(g[0]) | (256 if g[1] else 0) | (512 if g[2] else 0)


def elements(L, nup):
    """r in {0, 1, 2, L//2, L-1} x refl x flip (where defined)"""
    fl = (0, 1) if SR.flip_defined(L, nup) else (0,)
    return [(r, refl, f) for r in sorted({0, 1 % L, 2 % L, L // 2, L - 1}) for refl in (0, 1) for f in fl]


def group(L, nup):
    """the whole group: every T^r R^refl Z^flip"""
    fl = (0, 1) if SR.flip_defined(L, nup) else (0,)
    return [(r, refl, f) for r in range(L) for refl in (0, 1) for f in fl]


def nan_like(x):
    import torch
    out = torch.empty_like(x)
    (torch.view_as_real(out) if out.is_complex() else out).fill_(NAN)
    return out


def raw_apply(pkg, m, x, g, out, y=None, c=0j, code=None):
    """status of sd_symmetry_apply[_dev] called directly; the caller owns `out`"""
    import torch
    code = code_of(g) if code is None else code
    c = complex(c)
    if isinstance(x, torch.Tensor):
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        dt = pkg._lib.SD_C128 if x.is_complex() else pkg._lib.SD_F64
        rc = pkg.lib().sd_symmetry_apply_dev(m.ctx.h, m.h, dt, x.data_ptr(), len(x), code, None if y is None else y.data_ptr(),
                                             c.real, c.imag, out.data_ptr())
        torch.cuda.synchronize()
        return rc
    dt = pkg._lib.SD_C128 if np.iscomplexobj(x) else pkg._lib.SD_F64
    return pkg.lib().sd_symmetry_apply(m.ctx.h, m.h, dt, x.ctypes.data, len(x), code, None if y is None else y.ctypes.data, c.real,
                                       c.imag, out.ctypes.data)


class Small:
    """a SMALL shape: the model, the configurations of all rows and the source rows of elements, on the device"""

    def __init__(self, pkg, name):
        import torch
        self.name = name
        self.L, self.nup, boundary, ls, self.path = SMALL[name]
        self.m = build(pkg, self.L, self.nup, boundary, ls)
        assert pkg.lib().sd_model_path(self.m.h) == self.path
        self.N = self.m.N
        self.dev = torch.device("cuda", self.m.ctx.device)
        self.rows = torch.arange(self.N, dtype=torch.int64, device=self.dev)
        self.s = RR.configurations_t(self.rows, self.L, self.nup)
        self._src = {}

    def src(self, g):
        if g not in self._src:
            self._src[g] = SR.source_rows_t(self.s, self.L, self.nup, g)
        return self._src[g]

    def vec(self, pkg, cplx, seed):
        return fill_randn(pkg, self.m, self.N, cplx, seed + 7 * self.L + (self.nup or 0))


@pytest.fixture(scope="module")
def smalls(pkg):
    import torch
    store = {}

    def get(name):
        if name not in store:
            store[name] = Small(pkg, name)
        return store[name]
    yield get
    store.clear()
    gc.collect()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module")
def shapes(pkg):
    import torch
    st = Shapes(pkg)
    yield st
    st.store.clear()
    gc.collect()
    torch.cuda.empty_cache()


# ---- 1. the write form: all rows, bit for bit ----
@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("name", list(SMALL))
def test_write_form_small(pkg, smalls, name, cplx):
    import torch
    sh = smalls(name)
    m, L, nup = sh.m, sh.L, sh.nup
    x, y = sh.vec(pkg, cplx, 11), sh.vec(pkg, cplx, 12)
    hx, hy = x.cpu().numpy(), y.cpu().numpy()
    c = (0.75 - 1.25j) if cplx else -1.5
    worst = 0.0
    for g in elements(L, nup):
        want = x[sh.src(g)]
        out = nan_like(x)
        assert raw_apply(pkg, m, x, g, out) == 0 and torch.equal(out, want), (name, g)
        hout = np.full_like(hx, NAN)
        assert raw_apply(pkg, m, hx, g, hout) == 0 and np.array_equal(hout, want.cpu().numpy()), (name, g)
        # the fused form: one multiply-add per entry
        ref = want + c * y
        bar = 1e-15 * float(ref.abs().max())
        out = nan_like(x)
        assert raw_apply(pkg, m, x, g, out, y, c) == 0
        err = float((out - ref).abs().max())
        worst = max(worst, err / bar)
        assert err <= bar, (name, g, err, bar)
        hout = np.full_like(hx, NAN)
        assert raw_apply(pkg, m, hx, g, hout, hy, c) == 0 and np.array_equal(hout, out.cpu().numpy())
    print(f"{name} {'c128' if cplx else 'f64'}: fused form, worst error / bar {worst:.2f}")
    # the mirror is that very call: device tensors and host arrays, out= and the sugar
    g = elements(L, nup)[-1]
    kw = dict(shift=g[0], reflect=bool(g[1]), flip=bool(g[2]))
    assert torch.equal(pkg.symmetry_apply(x, m, **kw), x[sh.src(g)])
    got = pkg.symmetry_apply(hx, m, **kw)
    assert got.dtype == hx.dtype and np.array_equal(got, x[sh.src(g)].cpu().numpy())
    out = nan_like(x)
    assert pkg.translate(x, m, -1, out=out) is out and torch.equal(out, x[sh.src((L - 1, 0, 0))])
    assert torch.equal(pkg.reflect(x, m), x[sh.src((0, 1, 0))])
    assert torch.equal(pkg.symmetry_apply(x, m, shift=1, y=y, c=c, out=y.clone()), pkg.symmetry_apply(x, m, shift=1, y=y, c=c))
    if SR.flip_defined(L, nup):
        assert torch.equal(pkg.spin_flip(x, m), x[sh.src((0, 0, 1))])
        if nup is not None:
            assert torch.equal(pkg.spin_flip(x, m), torch.flip(x, [0]))          # the reversed stream


def test_write_form_argument_errors_leave_the_context_usable(pkg, smalls):
    import torch
    sh = smalls("L16n3-periodic")
    m, E = sh.m, pkg._lib
    x = sh.vec(pkg, True, 5)
    out = nan_like(x)
    assert raw_apply(pkg, m, x, (1, 0, 0), x) == SD_EARG                         # out aliases psi
    assert raw_apply(pkg, m, x, (0, 0, 1), out) == SD_EARG                       # Z at nup = 3 of L = 16
    for bad in (sh.L, 255, 1 << 10, -1):
        assert raw_apply(pkg, m, x, None, out, code=bad) == SD_EARG
    assert raw_apply(pkg, m, x.real.contiguous(), (1, 0, 0), nan_like(x.real.contiguous()), x.real.contiguous(), 1j) == SD_EARG
    assert raw_apply(pkg, m, x, (1, 0, 0), out, x, complex(NAN, 0.0)) == SD_EARG
    assert bool(torch.isnan(torch.view_as_real(out)).all())                      # nothing was written
    assert pkg.lib().sd_symmetry_apply_dev(m.ctx.h, m.h, E.SD_C128, x.data_ptr(), len(x) - 1, 1, None, 0.0, 0.0, out.data_ptr()) == E.SD_EDIM
    assert pkg.lib().sd_symmetry_apply_dev(m.ctx.h, m.h, 7, x.data_ptr(), len(x), 1, None, 0.0, 0.0, out.data_ptr()) == SD_EARG
    assert pkg.lib().sd_symmetry_apply_dev(m.ctx.h, m.h, E.SD_C128, None, len(x), 1, None, 0.0, 0.0, out.data_ptr()) == SD_EARG
    with pytest.raises(pkg.ArgumentError):
        pkg.spin_flip(x, m)
    with pytest.raises(pkg.ArgumentError):
        pkg.translate(x, m, 1, out=x)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.translate(x[:-1].contiguous(), m, 1)
    # overlaps and projector: list length, codes, null pointers, dtype_out
    one = np.array([1], dtype=np.intc)
    res = np.empty(2)
    big = np.zeros(253, dtype=np.intc)
    ov = pkg.lib().sd_symmetry_overlaps_dev
    assert ov(m.ctx.h, m.h, E.SD_C128, None, x.data_ptr(), len(x), big.ctypes.data_as(_ip), 253, res.ctypes.data_as(_dp)) == SD_EARG
    assert ov(m.ctx.h, m.h, E.SD_C128, None, x.data_ptr(), len(x), one.ctypes.data_as(_ip), 0, res.ctypes.data_as(_dp)) == SD_EARG
    assert ov(m.ctx.h, m.h, E.SD_C128, None, x.data_ptr(), len(x), None, 1, res.ctypes.data_as(_dp)) == SD_EARG
    assert ov(m.ctx.h, m.h, E.SD_C128, None, None, len(x), one.ctypes.data_as(_ip), 1, res.ctypes.data_as(_dp)) == SD_EARG
    short = x[:-1].contiguous()
    with pytest.raises(pkg.DimensionMismatch):                                   # a shorter device bra would be read past its end
        pkg.symmetry_overlaps(x, m, [(1,)], bra=short)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.symmetry_overlaps(x.cpu().numpy(), m, [(1,)], bra=short.cpu().numpy())
    with pytest.raises(pkg.DimensionMismatch):
        pkg.symmetry_apply(x, m, shift=1, y=short)
    with pytest.raises(pkg.ArgumentError):
        pkg.symmetry_overlaps(x, m, [(1,)], bra=x.cpu().numpy())
    # out and psi as two views into one buffer that overlap partly, and out overlapping y partly: refused like out == psi
    buf = torch.zeros(2 * len(x), dtype=x.dtype, device=x.device)
    half = len(x) // 2
    assert raw_apply(pkg, m, buf[:len(x)], (1, 0, 0), buf[half:half + len(x)]) == SD_EARG
    assert raw_apply(pkg, m, x, (1, 0, 0), buf[half:half + len(x)], buf[:len(x)], 1.0) == SD_EARG
    assert raw_apply(pkg, m, buf[:len(x)], (1, 0, 0), buf[len(x):]) == 0         # adjacent, no shared byte: accepted
    with pytest.raises(pkg.ArgumentError):
        pkg.symmetry_combine(buf[:len(x)], m, [(1,)], [1.0], out=buf[1:len(x) + 1])
    with pytest.raises(pkg.ArgumentError):
        pkg.symmetry_overlaps(x, m, [(0, 0, 1)])
    with pytest.raises(pkg.ArgumentError):
        pkg.symmetry_overlaps(x, m, [16])
    xr = x.real.contiguous()
    with pytest.raises(pkg.ArgumentError):                                       # float64 asked for with an imaginary coefficient
        pkg.symmetry_combine(xr, m, [(1,)], [1j], out=torch.empty_like(xr))
    with pytest.raises(pkg.ArgumentError):                                       # ... or for a complex psi
        pkg.symmetry_combine(x, m, [(1,)], [1.0], out=torch.empty_like(xr))
    with pytest.raises(pkg.ArgumentError):
        pkg.symmetry_combine(x, m, [(1,)], [1.0], out=x)
    with pytest.raises(pkg.ArgumentError):
        pkg.symmetry_project(x, m, momentum=3, parity=1)
    with pytest.raises(pkg.ArgumentError):
        pkg.symmetry_project(x, m, momentum=16)
    with pytest.raises(pkg.ArgumentError):
        pkg.symmetry_project(x, m, spin_flip=1)
    sharded = pkg.XXZChain(16, nup=8, boundary="periodic", **XXZ)
    sharded.set_shard(0, 2)
    xs = fill_randn(pkg, sharded, sharded.N, True, 1)
    with pytest.raises(pkg.ArgumentError):
        pkg.translate(xs, sharded, 1)
    with pytest.raises(pkg.ArgumentError):
        pkg.momentum_weights(xs, sharded)
    bare = pkg.XXZChain(16, nup=3, boundary="periodic", ctx=None, **XXZ)
    assert pkg.lib().sd_symmetry_apply_dev(m.ctx.h, bare.h, E.SD_C128, x.data_ptr(), len(x), 1, None, 0.0, 0.0, out.data_ptr()) == SD_EARG
    # ... and the context still works
    assert raw_apply(pkg, m, x, (1, 1, 0), out) == 0 and torch.equal(out, x[sh.src((1, 1, 0))])


@pytest.mark.parametrize("nup", [0, 6])
def test_polarised_sectors(pkg, nup):
    """one row: every U_g is the identity, the state has momentum 0 and even parity, Z is undefined"""
    L = 6
    m = pkg.XXZChain(L, nup=nup, boundary="periodic", **XXZ)
    assert m.N == 1
    for psi in (np.array([1.5]), np.array([0.5 - 1.25j])):
        for g in [(r, refl, 0) for r in range(L) for refl in (0, 1)]:
            assert np.array_equal(pkg.symmetry_apply(psi, m, *g), psi)
        n2 = abs(psi[0]) ** 2
        ov = pkg.symmetry_overlaps(psi, m, [(r,) for r in range(L)])
        assert np.abs(ov - n2).max() <= 1e-15 * n2
        assert np.array_equal(pkg.symmetry_project(psi, m, parity=1), psi) and np.all(pkg.symmetry_project(psi, m, parity=-1) == 0.0)
        assert np.abs(pkg.symmetry_project(psi, m, momentum=2)).max() <= 1e-13 * abs(psi[0])      # the projector's bar
        qn = pkg.quantum_numbers(psi, m)
        assert (qn["momentum"], qn["parity"], qn["spin_flip"]) == (0, 1, None)
        with pytest.raises(pkg.ArgumentError):
            pkg.spin_flip(psi, m)


# ---- 2. group laws on the device, exact ----
@pytest.mark.parametrize("name", ["L2n1-periodic", "L12n6-periodic", "L16n8-open", "L16n3-periodic", "L14n7-suffix8", "L13n1-per-row", "full-L10"])
def test_group_laws_on_the_device(pkg, smalls, name):
    import torch
    sh = smalls(name)
    m, L = sh.m, sh.L
    for cplx in (False, True):
        psi = sh.vec(pkg, cplx, 31)
        x = psi
        for _ in range(L):
            x = pkg.translate(x, m, 1)
        assert torch.equal(x, psi)                                                          # T^L = 1
        assert torch.equal(pkg.reflect(pkg.reflect(psi, m), m), psi)                        # R^2 = 1
        assert torch.equal(pkg.reflect(pkg.translate(pkg.reflect(psi, m), m, 1), m), pkg.translate(psi, m, -1))     # R T R = T^-1
        for a, b in ((1, 1), (2, L - 1), (L // 2, L // 2), (L - 1, 3 % L)):
            assert torch.equal(pkg.translate(pkg.translate(psi, m, b), m, a), pkg.translate(psi, m, a + b))
        assert torch.equal(pkg.symmetry_apply(psi, m, 2 % L, True), pkg.translate(pkg.reflect(psi, m), m, 2))       # U_g = T^r R
        if SR.flip_defined(L, sh.nup):
            assert torch.equal(pkg.spin_flip(pkg.spin_flip(psi, m), m), psi)                # Z^2 = 1
            assert torch.equal(pkg.spin_flip(pkg.translate(psi, m, 1), m), pkg.translate(pkg.spin_flip(psi, m), m, 1))
            assert torch.equal(pkg.symmetry_apply(psi, m, 1, True, True), pkg.translate(pkg.reflect(pkg.spin_flip(psi, m), m), m, 1))


# ---- 3. where the capped grids wrap ----
class ZSector:
    """Zs (see the module docstring), with the attributes of test_gpu_operator_grids.Shape that the checks below read"""

    def __init__(self, pkg):
        import torch
        self.name, self.L, self.nup, self.path = "Zs", 22, 11, 1
        self.m = build(pkg, self.L, self.nup, "periodic", 8)
        assert pkg.lib().sd_model_path(self.m.h) == 1
        lb, gb, ln = self.m.local_tiles()
        self.tiles = (gb, ln)
        self.N = self.m.N
        self.dev = torch.device("cuda", self.m.ctx.device)
        self.rows = torch.arange(self.N, dtype=torch.int64, device=self.dev)
        self.s = RR.configurations_t(self.rows, self.L, self.nup)
        self.psi_r = fill_randn(pkg, self.m, self.N, False, 101 + self.L)
        self.psi_c = fill_randn(pkg, self.m, self.N, True, 202 + self.L)


def crosses_the_symmetry_caps(sh):
    """every launcher of kernels_symmetry.hip sends a workgroup through its loop more than once at this shape"""
    if sh.path == 1:
        n_tiles = len(sh.tiles[0])
        assert n_tiles > SYM_TILE_BLOCKS and n_tiles > SYM_RED_BLOCKS          # write form / projector; overlaps
    else:
        assert sh.N > SYM_ROW_BLOCKS * 256 and sh.N > SYM_RED_BLOCKS * 256


def wrap_elements(L, nup):
    z = 1 if SR.flip_defined(L, nup) else 0
    return [(1, 0, 0), (L // 2, 1, 0), (L - 1, 1, z), (3, 0, z)]


@pytest.mark.parametrize("name", ["T-periodic", "Ts", "R-periodic", "F", "Zs"])
def test_grid_wrap(pkg, shapes, name):
    import torch
    if name == "Zs":
        sh = ZSector(pkg)
        assert sh.tiles[1].max() <= 128 and 2 * sh.nup == sh.L
    else:
        sh = shapes.get(name)
        assert_crosses_the_caps(sh)
    crosses_the_symmetry_caps(sh)
    m, L, nup = sh.m, sh.L, sh.nup
    if name == "R-periodic":
        assert L > 32                                        # the rotation crosses bit 38 of a 64-bit word
    el = wrap_elements(L, nup)
    src = {g: SR.source_rows_t(sh.s, L, nup, g) for g in el}
    # the write form, all rows, exactly
    for psi in (sh.psi_r, sh.psi_c):
        out = nan_like(psi)
        for g in el:
            (torch.view_as_real(out) if out.is_complex() else out).fill_(NAN)
            assert raw_apply(pkg, m, psi, g, out) == 0
            want = psi[src[g]]
            if not torch.equal(out, want):
                bad = (out != want) | torch.isnan(out.real if out.is_complex() else out)
                raise AssertionError(f"{name} {g}: {int(bad.sum())} of {sh.N} rows differ; first rows {bad.nonzero().flatten()[:8].tolist()}")
        del out
    if SR.flip_defined(L, nup) and nup is not None:
        assert torch.equal(pkg.spin_flip(sh.psi_c, m), torch.flip(sh.psi_c, [0]))
    # overlaps: ten elements, a full chunk and a partial one
    bra, ket = sh.psi_c, fill_randn(pkg, m, sh.N, True, 404 + L)
    many = (el + [(0, 0, 0), (2, 0, 0), (0, 1, 0), (L - 2, 0, 0), (1, 1, 0), (L // 2, 0, 0)])[:10]
    assert len(many) > SYM_CHUNK
    for g in many:
        if g not in src:
            src[g] = SR.source_rows_t(sh.s, L, nup, g)
    want = np.array([complex((torch.conj(bra) * ket[src[g]]).sum().item()) for g in many])
    got = pkg.symmetry_overlaps(ket, m, many, bra=bra)
    bar = 1e-12 * math.sqrt(norm2(bra) * norm2(ket))
    print(f"{name}: overlaps {np.abs(got - want).max():.2e} (bar {bar:.2e}, max |want| {np.abs(want).max():.2e})")
    assert np.abs(got - want).max() <= bar
    again = pkg.symmetry_overlaps(ket, m, many, bra=bra)
    assert np.array_equal(got.view(np.float64), again.view(np.float64))
    gr = pkg.symmetry_overlaps(sh.psi_r, m, many[:3])
    wr = np.array([float((sh.psi_r * sh.psi_r[src[g]]).sum().item()) for g in many[:3]])
    assert np.all(gr.imag == 0.0) and np.abs(gr.real - wr).max() <= 1e-12 * norm2(sh.psi_r)
    del bra
    # the projector: three elements with complex coefficients, and a real combination of a real vector
    co = [0.5 - 0.25j, -0.75j, 0.3 + 0.1j, 0.2]
    for psi in (sh.psi_r, ket):
        ref = SR.combine_t(psi, sh.s, L, nup, el, co)
        out = nan_like(ket)
        assert pkg.symmetry_combine(psi, m, el, co, out=out) is out
        bar = 1e-13 * math.sqrt(norm2(psi))
        err = float((out - ref).abs().max())
        print(f"{name}: projector {'c128' if psi.is_complex() else 'f64'} {err:.2e} (bar {bar:.2e})")
        assert err <= bar
        del ref, out
    ref = SR.combine_t(sh.psi_r, sh.s, L, nup, el, [0.5, -1.0, 0.25, 2.0]).real
    got = pkg.symmetry_combine(sh.psi_r, m, el, [0.5, -1.0, 0.25, 2.0])
    assert got.dtype == torch.float64 and float((got - ref).abs().max()) <= 1e-13 * math.sqrt(norm2(sh.psi_r))
    shapes.drop(name)                                        # no later test of this module uses the shape
    del sh, src, ket, ref, got
    gc.collect()
    torch.cuda.empty_cache()


# ---- 4. overlaps and momentum weights ----
@pytest.mark.parametrize("name", list(SMALL))
def test_overlaps_and_weights_small(pkg, smalls, name):
    import torch
    sh = smalls(name)
    m, L, nup = sh.m, sh.L, sh.nup
    bra, ket = sh.vec(pkg, True, 41), sh.vec(pkg, True, 42)
    el = group(L, nup)                                       # up to 64 elements: several chunks, the last one partial or full
    ref = np.array([complex((torch.conj(bra) * ket[sh.src(g)]).sum().item()) for g in el])
    assert np.abs(ref.imag).max() > 1e-3                     # the conjugation is really exercised
    bar = 1e-12 * math.sqrt(norm2(bra) * norm2(ket))
    for b, k in ((bra, ket), (bra.cpu().numpy(), ket.cpu().numpy())):
        got = pkg.symmetry_overlaps(k, m, el, bra=b)
        assert got.shape == (len(el),) and got.dtype == np.complex128
        err = np.abs(got - ref).max()
        print(f"{name} {'dev' if b is bra else 'host'}: {len(el)} elements, {err:.2e} (bar {bar:.2e})")
        assert err <= bar
    assert el[0] == (0, 0, 0) and abs(got[0] - complex(torch.vdot(bra, ket).item())) <= bar       # the r = 0 entry is <bra|ket>
    again = pkg.symmetry_overlaps(ket, m, el, bra=bra)
    first = pkg.symmetry_overlaps(ket, m, el, bra=bra)
    assert np.array_equal(first.view(np.float64), again.view(np.float64))                         # two calls: identical bits
    # a real bra with a complex ket is promoted; real with real stays real
    br = sh.vec(pkg, False, 43)
    mixed = pkg.symmetry_overlaps(ket, m, el[:5], bra=br)
    assert np.abs(mixed - np.array([complex((br * ket[sh.src(g)]).sum().item()) for g in el[:5]])).max() <= 1e-12 * math.sqrt(norm2(br) * norm2(ket))
    rr = pkg.symmetry_overlaps(br, m, el[:5])
    assert np.all(rr.imag == 0.0) and abs(rr[0].real - norm2(br)) <= 1e-12 * norm2(br)
    # momentum weights
    for psi in (ket, br):
        n2 = norm2(psi)
        w = pkg.momentum_weights(psi, m)
        ov = np.array([complex((torch.conj(psi) * psi[sh.src((r, 0, 0))]).sum().item()) for r in range(L)])
        want = np.array([sum(SR.phase(n, r, L) * ov[r] for r in range(L)).real / L for n in range(L)])
        assert w.shape == (L,) and w.dtype == np.float64
        assert np.abs(w - want).max() <= 1e-12 * n2
        assert np.all(w >= -1e-12 * n2) and abs(w.sum() - n2) <= 1e-12 * n2
        assert np.array_equal(w, pkg.momentum_weights(psi.cpu().numpy(), m))


# ---- 5. the projector ----
@pytest.mark.parametrize("name", list(SMALL))
def test_projector_small(pkg, smalls, name):
    import torch
    sh = smalls(name)
    m, L, nup = sh.m, sh.L, sh.nup
    k = 2 * np.pi * np.arange(L) / L
    for cplx in (True, False):
        psi = sh.vec(pkg, cplx, 51)
        nrm = math.sqrt(norm2(psi))
        bar = 1e-13 * nrm
        P = []
        for n in range(L):
            el, co = SR.projector_list(L, momentum=n)
            ref = SR.combine_t(psi, sh.s, L, nup, el, co)
            got = pkg.symmetry_project(psi, m, momentum=n)
            real_out = (not cplx) and (n == 0 or 2 * n == L)
            assert got.dtype == (torch.float64 if real_out else torch.complex128), (name, n)       # float64 in, real projector: float64 out
            err = float((got - (ref.real if real_out else ref)).abs().max())
            assert err <= bar, (name, n, err, bar)
            host = pkg.symmetry_project(psi.cpu().numpy(), m, momentum=n)
            assert host.dtype == (np.float64 if real_out else np.complex128) and np.array_equal(host, got.cpu().numpy())
            P.append(got.to(torch.complex128))
            assert float((pkg.symmetry_project(got, m, momentum=n) - got).abs().max()) <= bar      # P_n P_n psi = P_n psi
            assert float((pkg.translate(P[n], m, 1) - complex(np.exp(-1j * k[n])) * P[n]).abs().max()) <= bar   # T P_n = e^{-i k_n} P_n
        G = np.array([[complex(torch.vdot(P[a], P[b]).item()) for b in range(L)] for a in range(L)])
        off = ~np.eye(L, dtype=bool)
        if L > 1:
            assert np.abs(G[off]).max() <= 1e-12 * nrm * nrm, name                                   # <P_n psi|P_m psi> = 0
        assert float((sum(P) - psi).abs().max()) <= bar                                              # sum_n P_n = 1
        # parity and spin flip, alone and with the momenta that allow them
        sectors = [dict(parity=1), dict(parity=-1), dict(momentum=0, parity=-1)]
        if L % 2 == 0:
            sectors.append(dict(momentum=L // 2, parity=1))
        if SR.flip_defined(L, nup):
            sectors += [dict(spin_flip=-1), dict(momentum=0, parity=1, spin_flip=1)]
        for kw in sectors:
            el, co = SR.projector_list(L, **kw)
            assert len(el) <= 4 * L
            ref = SR.combine_t(psi, sh.s, L, nup, el, co)
            got = pkg.symmetry_project(psi, m, **kw)
            assert got.dtype == psi.dtype                    # these coefficients are real
            assert float((got - (ref if cplx else ref.real)).abs().max()) <= bar, (name, kw)
            assert float((pkg.symmetry_project(got, m, **kw) - got).abs().max()) <= bar
            if "parity" in kw:
                assert float((pkg.reflect(got, m) - kw["parity"] * got).abs().max()) <= bar
            if "spin_flip" in kw:
                assert float((pkg.spin_flip(got, m) - kw["spin_flip"] * got).abs().max()) <= bar


# ---- 6. physics ----
def commutator(pkg, m, psi, U):
    """|H U psi - U H psi| / |H psi|"""
    import torch
    a, b = torch.empty_like(psi), torch.empty_like(psi)
    pkg.apply_H(a, U(psi), m)
    pkg.apply_H(b, psi, m)
    return float(torch.linalg.vector_norm(a - U(b)) / torch.linalg.vector_norm(b))


def test_symmetries_commute_with_the_hamiltonian(pkg):
    """XXZ ring L = 12, nup = 6, hz = 0: apply_H(U_g psi) against U_g apply_H(psi) for T, R and Z, relative to |H psi|.  The write form
    is a permutation, so the only error is apply_H's own: the same sum in another order at the permuted row.  The bar is 10 x the
    same commutator formed with the torch restatement of U_g on the same vector (the library's U_g equals it bit for bit, see the
    write-form tests, so the two numbers agree), with a floor of 1e-15 -- a few roundings of a reordered 13-term sum, so that a
    restatement value of exactly 0 (Z: the apply happens to sum alike at the reversed row) does not pin the apply's summation order --
    and never above 1e-14: a row of H psi has at most 13 terms of modulus <= 0.4 |psi|_max.
    Measured on an MI355X: T 1.0e-16, R 1.5e-16, Z 0 exactly, T^5 R Z 1.5e-16 (ComplexF64; Float64 alike), the restatement's the same
    to the digit (compare the energy current's 9e-15, a product of two operators at L = 25).  On the open chain the T commutator is of
    order one and symmetric_operator refuses the momentum sector."""
    import torch
    L, nup = 12, 6
    m = pkg.XXZChain(L, nup=nup, boundary="periodic", Jxy=0.8, Jz=0.7, hz=0.0)
    rows = torch.arange(m.N, dtype=torch.int64, device=torch.device("cuda", m.ctx.device))
    s = RR.configurations_t(rows, L, nup)
    for cplx in (False, True):
        psi = fill_randn(pkg, m, m.N, cplx, 61)
        for label, kw, g in (("T", dict(shift=1), (1, 0, 0)), ("R", dict(reflect=True), (0, 1, 0)), ("Z", dict(flip=True), (0, 0, 1)),
                             ("T^5 R Z", dict(shift=5, reflect=True, flip=True), (5, 1, 1))):
            assert pkg.is_symmetric(m, **kw)
            src = SR.source_rows_t(s, L, nup, g)
            got = commutator(pkg, m, psi, lambda v: pkg.symmetry_apply(v, m, **kw))
            ref = commutator(pkg, m, psi, lambda v: v[src])
            print(f"[H, {label}] {'c128' if cplx else 'f64'}: {got:.2e} (restatement {ref:.2e})")
            assert got <= max(10 * ref, 1e-15) and got <= 1e-14
    mo = pkg.XXZChain(L, nup=nup, boundary="open", Jxy=0.8, Jz=0.7, hz=0.0)
    psi = fill_randn(pkg, mo, mo.N, True, 62)
    assert not pkg.is_symmetric(mo, shift=1) and pkg.is_symmetric(mo, reflect=True)
    assert commutator(pkg, mo, psi, lambda v: pkg.translate(v, mo, 1)) > 1e-3
    assert commutator(pkg, mo, psi, lambda v: pkg.reflect(v, mo)) <= 1e-14
    with pytest.raises(pkg.ArgumentError):
        pkg.symmetric_operator(mo, momentum=0)
    with pytest.raises(pkg.ArgumentError):
        pkg.lowest_level(mo, momentum=1)
    assert callable(pkg.symmetric_operator(mo, parity=1))
    field = pkg.XXZChain(L, nup=nup, boundary="periodic", hz=0.3)
    with pytest.raises(pkg.ArgumentError):
        pkg.symmetric_operator(field, spin_flip=1)


_ed = {}


def dense_ring(D, L):
    """(levels, eigenvectors, H) of the Heisenberg ring at nup = L/2 from oracle/dense.py's operators.  dense_H forms 4^L-entry
    products per bond, minutes at L = 12; the same site operators as sparse matrices give the same H in a second."""
    if L not in _ed:
        import scipy.sparse as sp
        hop, zz, _field = D.xxz_lists(L, boundary="periodic")
        st = D.sector_states(L, L // 2).astype(np.int64)
        plus = {i: sp.csr_matrix(D.site_op(D.SP, i, L)) for i in range(1, L + 1)}
        sz = {i: np.diag(D.site_op(D.SZ, i, L)).copy() for i in range(1, L + 1)}
        H = sp.csr_matrix((1 << L, 1 << L))
        for i, j, J in zz:
            H = H + sp.diags(J * sz[i] * sz[j])
        for i, j, J in hop:
            t = plus[i] @ plus[j].T
            H = H + J * (t + t.T)
        Hs = H.tocsr()[st][:, st].toarray()
        w, v = np.linalg.eigh(Hs)
        _ed[L] = (w, v, Hs)
    return _ed[L]


@pytest.mark.parametrize("L", [10, 12])
def test_quantum_numbers_of_the_ground_state(pkg, D, L):
    """the labels of groundstate() equal those of the dense ground state, labelled by the restatement (nothing hard-coded)"""
    nup = L // 2
    w, v, _H = dense_ring(D, L)
    assert w[1] - w[0] > 0.1
    want = SR.labels(v[:, 0], L, nup)
    assert None not in want
    m = pkg.XXZChain(L, nup=nup, boundary="periodic")
    E0, psi = pkg.groundstate(m)
    assert abs(E0 - w[0]) <= 1e-10 * abs(w[0])
    qn = pkg.quantum_numbers(psi, m)
    print(f"L={L}: E0 {E0:.10f}, labels {qn['momentum'], qn['parity'], qn['spin_flip']} (dense {want})")
    assert (qn["momentum"], qn["parity"], qn["spin_flip"]) == want
    ex = qn["expectation"]
    assert abs(ex["norm2"] - 1.0) <= 1e-10 and abs(ex["weights"].sum() - ex["norm2"]) <= 1e-12
    assert abs(ex["T"][1] - np.exp(-2j * np.pi * want[0] / L)) <= 1e-8 and abs(ex["R"] - want[1]) <= 1e-8 and abs(ex["Z"] - want[2]) <= 1e-8
    import torch
    dev_psi = torch.as_tensor(psi, device=torch.device("cuda", m.ctx.device))
    assert pkg.quantum_numbers(dev_psi, m)["momentum"] == want[0]
    # a random vector has no label; in a sector where Z is undefined its label is None and nothing fails
    rnd = fill_randn(pkg, m, m.N, True, 71)
    qr = pkg.quantum_numbers(rnd, m)
    assert (qr["momentum"], qr["parity"], qr["spin_flip"]) == (None, None, None)
    m3 = pkg.XXZChain(L, nup=3, boundary="periodic")
    q3 = pkg.quantum_numbers(pkg.symmetry_project(fill_randn(pkg, m3, m3.N, True, 72), m3, momentum=2), m3)
    assert (q3["momentum"], q3["parity"], q3["spin_flip"]) == (2, None, None) and q3["expectation"]["Z"] is None


def test_lowest_level_of_every_sector(pkg, D):
    """Heisenberg ring L = 12, nup = 6: lowest_level at every momentum, and with parity +-1 at n = 0, against the dense levels
    labelled by the restatement's projectors (the lowest eigenvalue of P (H - sigma) P + sigma, sigma above the spectrum).  Bar:
    max(1e-10 max|E|, 10 x the error of the plain lanczos_extremal call against dense ED at this shape).  Measured on an MI355X: plain
    call 1.8e-15, bar 5.4e-10, worst of the 14 sectors 2.2e-14 (the sectors hold 75 to 80 levels, 50 and 30 with parity: 100 steps exhaust them)."""
    L, nup = 12, 6
    w, _v, H = dense_ring(D, L)
    m = pkg.XXZChain(L, nup=nup, boundary="periodic")
    plain = abs(pkg.lanczos_extremal(pkg.apply_H, m, lanc_m=100)[0] - w[0])
    bar = max(1e-10 * np.abs(w).max(), 10 * plain)
    sigma = np.abs(w).max() + 1.0
    eye = np.eye(m.N)
    sectors = [dict(momentum=n) for n in range(L)] + [dict(momentum=0, parity=1), dict(momentum=0, parity=-1)]
    worst, levels = 0.0, []
    for kw in sectors:
        P = SR.project(eye, L, nup, **kw)
        want = np.linalg.eigvalsh(P.conj().T @ (H - sigma * eye) @ P)[0] + sigma
        got = pkg.lowest_level(m, lanc_m=100, **kw)
        levels.append(got)
        worst = max(worst, abs(got - want))
        print(f"{kw}: {got:.10f} (dense {want:.10f}, error {abs(got - want):.2e})")
        assert abs(got - want) <= bar, (kw, got, want, bar)
    print(f"plain lanczos_extremal error {plain:.2e}, bar {bar:.2e}, worst sector error {worst:.2e}")
    assert abs(min(levels[:L]) - w[0]) <= bar and abs(min(levels[L:]) - levels[0]) <= bar
    assert pkg.default_context()._apply_cb is None           # the sector operator was removed again
