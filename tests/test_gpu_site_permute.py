"""Site permutations: sd_site_permute[_dev] and permute_sites, bit for bit, at the smallest shapes at which the capped
launch grids of k_site_permute wrap -- the shapes tests/test_gpu_operator_grids.py documents, each asserted first against the
launcher's constants (4096 workgroups over the tiles of a tiled plan, 8192 blocks of 256 rows otherwise):
  Ts  XXZ L=21 nup=10, SD_SUFFIX_BITS=8: 8086 tiles of at most 70 rows (> 4096 tiles; tiles that leave waves of the workgroup idle)
  R   XXZ L=39 nup=6, per-row path, 3 262 623 rows                    (> 8192 * 256 rows; five table bytes; binomials in LDS)
  F   XXZ L=22 full basis, 4 194 304 rows                             (> 8192 * 256 rows; three table bytes)
  T   XXZ L=25 nup=12, the default plan: 8191 tiles of up to 924 rows (> 4096 tiles; the inner loop of a tile runs four times)
The expected vector is formed on the device with torch over ALL rows: the configurations of tests/rows_ref.py, a per-bit permutation
loop, rank_t, one gather.  Real and imaginary parts are compared as separate doubles under ==; outputs are filled with NaN first."""
import ctypes as C

import numpy as np
import pytest

import rows_ref as RR
import subsystem_ref as SR

pytestmark = pytest.mark.gpu

_ip = C.POINTER(C.c_int)
TILE_BLOCKS, ROW_BLOCKS = 4096, 8192          # SD_PERM_TILE_BLOCKS, SD_PERM_ROW_BLOCKS
# name -> L, nup, SD_SUFFIX_BITS or None, sd_model_path (0 per row, 1 tiled, 2 full basis)
SPECS = {"Ts": (21, 10, 8, 1), "R": (39, 6, None, 0), "F": (22, None, None, 2), "T": (25, 12, None, 1)}
PERMS = ["identity", "T", "R", "random", "last two sites to the front", "middle block to the front"]
_shapes = {}


def perm_of(name, L):
    if name == "identity":
        return list(range(1, L + 1))
    if name == "T":
        return SR.translation(L)
    if name == "R":
        return SR.reflection(L)
    if name == "random":
        return [int(x) for x in np.random.default_rng(20261020 + L).permutation(L) + 1]
    if name == "last two sites to the front":                  # every suffix bit moves
        return SR.stable_partition(L, [L - 1, L])
    return SR.stable_partition(L, [5, 6, 7, 8])                # the suffix sites stay where they are


class Shape:
    def __init__(self, pkg, name):
        import torch
        self.L, self.nup, ls, self.path = SPECS[name]
        with pytest.MonkeyPatch.context() as mp:               # the plan reads SD_SUFFIX_BITS when the model is built
            if ls is None:
                mp.delenv("SD_SUFFIX_BITS", raising=False)
            else:
                mp.setenv("SD_SUFFIX_BITS", str(ls))
            self.m = pkg.XXZChain(self.L, nup=self.nup, boundary="open")
            assert pkg.lib().sd_model_path(self.m.h) == self.path
            self.tile_len = self.m.local_tiles()[2] if self.path == 1 else None
        m = self.m
        self.N = m.N
        self.dev = torch.device("cuda", m.ctx.device)
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        self.psi = {}
        for cplx in (False, True):
            x = torch.empty(m.N, dtype=torch.complex128 if cplx else torch.float64, device=self.dev)
            pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, x.data_ptr(), (2 if cplx else 1) * m.N, 77 + self.L + cplx, 0), m.ctx.h)
            self.psi[cplx] = x
        rows = torch.arange(m.N, dtype=torch.int64, device=self.dev)
        self.s = RR.configurations_t(rows, self.L, self.nup)

    def source_rows(self, perm):
        """the row of psi that every row of U psi copies: bit i of the source = bit perm[i] - 1 of the row's configuration"""
        import torch
        src = torch.zeros_like(self.s)
        for i in range(self.L):
            src = src | (((self.s >> (perm[i] - 1)) & 1) << i)
        return src if self.nup is None else RR.rank_t(src, self.L, self.nup)


def shape_of(pkg, name):
    if name not in _shapes:
        _shapes.clear()                                        # one shape's vectors on the device at a time
        _shapes[name] = Shape(pkg, name)
    return _shapes[name]


def same_bits(a, b):
    import torch
    if a.is_complex():
        a, b = torch.view_as_real(a), torch.view_as_real(b)
    return a.shape == b.shape and bool((a == b).all())


def nan_like(x):
    import torch
    return torch.full_like(x, float("nan")) if not x.is_complex() else torch.full_like(x, complex(float("nan"), float("nan")))


def raw(pkg, m, x, perm, out, n=None, dtype=None, ctx="model"):
    """status of sd_site_permute[_dev] called directly; the caller owns `out`"""
    import torch
    dev = isinstance(x, torch.Tensor) or isinstance(out, torch.Tensor)
    cplx = (x if x is not None else out).is_complex() if dev else np.iscomplexobj(x if x is not None else out)
    code = (pkg._lib.SD_C128 if cplx else pkg._lib.SD_F64) if dtype is None else dtype
    p = None if perm is None else np.ascontiguousarray(perm, dtype=np.intc)
    pp = None if p is None else p.ctypes.data_as(_ip)
    ptr = lambda v: None if v is None else (v.data_ptr() if dev else v.ctypes.data)      # noqa: E731
    if dev and m.ctx is not None:
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    h = m.ctx.h if ctx == "model" else ctx
    fn = pkg.lib().sd_site_permute_dev if dev else pkg.lib().sd_site_permute
    length = (len(x) if x is not None else len(out)) if n is None else n
    return fn(h, m.h, code, ptr(x), length, pp, ptr(out))


@pytest.mark.parametrize("pname", PERMS)
@pytest.mark.parametrize("name", list(SPECS))
def test_every_row_bit_for_bit_where_the_grids_wrap(pkg, name, pname):
    import torch
    sh = shape_of(pkg, name)
    m, L = sh.m, sh.L
    if sh.path == 1:                                           # the cap this shape is there to cross
        assert len(sh.tile_len) > TILE_BLOCKS
        if name == "Ts":
            assert len(sh.tile_len) == 8086 and sh.tile_len.max() == 70
        else:
            assert len(sh.tile_len) == 8191 and sh.tile_len.max() == 924 > 3 * 256
    else:
        assert sh.N > ROW_BLOCKS * 256
    perm = perm_of(pname, L)
    if pname != "identity":
        assert perm != list(range(1, L + 1))
    if pname == "middle block to the front":
        assert perm[8:] == list(range(9, L + 1))               # sites 9..L stay: the plan's suffix sites among them
    idx = sh.source_rows(perm)
    for cplx in (False, True):
        x = sh.psi[cplx]
        want = x[idx]
        out = nan_like(x)
        assert raw(pkg, m, x, perm, out) == 0, pkg.lib().sd_last_error(m.ctx.h)
        torch.cuda.synchronize()
        assert same_bits(out, want), (name, pname, cplx)
        if pname == "identity":
            assert same_bits(out, x)
        if pname == "T":
            assert same_bits(out, pkg.translate(x, m, 1))
        if pname == "R":
            assert same_bits(out, pkg.reflect(x, m))
        if pname == "random":                                  # U_{pi^-1} U_pi = 1, through the Python mirror
            back = pkg.permute_sites(out, m, pkg.permutation_inverse(perm), out=nan_like(x))
            assert same_bits(back, x)
        del want, out
    del idx


@pytest.mark.parametrize("L,nup,ls", [(12, 6, None), (12, 6, 4), (13, 5, 8), (13, 5, 5), (10, None, None), (17, 8, 9), (6, 0, None), (6, 6, None), (2, 1, None)])
def test_small_shapes_host_and_device_forms(pkg, L, nup, ls):
    """host form == device form == the restatement of tests/subsystem_ref.py (numpy, per-bit loops and a dict), both dtypes"""
    import torch
    with pytest.MonkeyPatch.context() as mp:
        if ls is None:
            mp.delenv("SD_SUFFIX_BITS", raising=False)
        else:
            mp.setenv("SD_SUFFIX_BITS", str(ls))
        m = pkg.XXZChain(L, nup=nup)
    rng = np.random.default_rng(3 + L)
    perms = [SR.translation(L), SR.reflection(L), list(range(1, L + 1)), [int(x) for x in rng.permutation(L) + 1],
             [int(x) for x in rng.permutation(L) + 1]]
    if L > 4:
        perms += [SR.stable_partition(L, [L - 1, L]), SR.stable_partition(L, [2, 3]), SR.stable_partition(L, list(range(1, L + 1, 2)))]
    rows = [SR.source_rows(L, nup, perm) for perm in perms]
    for cplx in (False, True):
        psi = rng.standard_normal(m.N) + (1j * rng.standard_normal(m.N) if cplx else 0.0)
        dev = torch.from_numpy(psi).to(torch.device("cuda", m.ctx.device))
        for perm, src in zip(perms, rows):
            want = psi[src]
            out = np.full_like(psi, np.nan)
            assert raw(pkg, m, psi, perm, out) == 0
            assert out.dtype == psi.dtype and np.array_equal(out.view(np.float64), want.view(np.float64))
            got = pkg.permute_sites(dev, m, perm)
            assert got.dtype == dev.dtype and np.array_equal(got.cpu().numpy().view(np.float64), want.view(np.float64))
            assert np.array_equal(pkg.permute_sites(psi, m, perm).view(np.float64), want.view(np.float64))
    # a float32 / integer vector is promoted like everywhere else
    assert pkg.permute_sites(np.arange(m.N), m, perms[0]).dtype == np.float64


def test_statuses(pkg):
    import torch
    E = pkg._lib
    L, nup = 12, 6
    m = pkg.XXZChain(L, nup=nup)
    rng = np.random.default_rng(11)
    host = rng.standard_normal(m.N) + 1j * rng.standard_normal(m.N)
    dev = torch.from_numpy(host).to(torch.device("cuda", m.ctx.device))
    good = SR.translation(L)
    sharded = pkg.XXZChain(L, nup=nup)
    sharded.set_shard(0, 2)
    bare = pkg.XXZChain(L, nup=nup, ctx=None)
    for x in (host, dev):
        new = (lambda: np.full_like(x, np.nan)) if x is host else (lambda: nan_like(x))
        assert raw(pkg, m, x, good, new()) == 0
        for bad in ([1] * L, [0] + good[1:], [L + 1] + good[1:], good[:-1] + [good[0]], [-3] + good[1:]):
            assert raw(pkg, m, x, bad, new()) == E.SD_EARG                     # not a bijection of 1..L
        assert raw(pkg, m, x, None, new()) == E.SD_EARG                        # NULL pointers
        assert raw(pkg, m, None, good, new()) == E.SD_EARG
        assert raw(pkg, m, x, good, None) == E.SD_EARG
        assert raw(pkg, m, x, good, new(), ctx=None) == E.SD_EARG
        for dt in (0, 3, 7):
            assert raw(pkg, m, x, good, new(), dtype=dt) == E.SD_EARG
        assert raw(pkg, m, x, good, new(), n=m.N - 1) == E.SD_EDIM
        assert raw(pkg, m, x, good, new(), n=m.N + 1) == E.SD_EDIM
        assert raw(pkg, m, x, good, x) == E.SD_EARG                            # out is psi
        assert raw(pkg, sharded, x, good, new()) == E.SD_EARG
        assert raw(pkg, bare, x, good, new(), ctx=m.ctx.h) == E.SD_EARG
        out = new()
        assert raw(pkg, m, x, good, out) == 0                                  # the context is still usable
        if x is dev:
            torch.cuda.synchronize()
            out = out.cpu().numpy()
        assert np.array_equal(out.view(np.float64), SR.permute(host, L, nup, good).view(np.float64))
    # partial overlap: two windows of one buffer that share all but one element
    buf = torch.zeros(m.N + 1, dtype=torch.complex128, device=dev.device)
    assert raw(pkg, m, buf[:m.N], good, buf[1:]) == E.SD_EARG
    assert raw(pkg, m, buf[1:], good, buf[:m.N]) == E.SD_EARG
    hbuf = np.zeros(m.N + 1, dtype=np.complex128)
    assert raw(pkg, m, hbuf[:m.N], good, hbuf[1:]) == E.SD_EARG
    assert pkg.lib().sd_site_permute_dev(m.ctx.h, None, E.SD_C128, dev.data_ptr(), m.N, None, dev.data_ptr()) == E.SD_EARG
    # the Python mirror
    with pytest.raises(pkg.ArgumentError):
        pkg.permute_sites(host, m, good[:-1])
    with pytest.raises(pkg.ArgumentError):
        pkg.permute_sites(host, m, [1] * L)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.permute_sites(host[:-1], m, good)
    with pytest.raises(pkg.ArgumentError):
        pkg.permute_sites(dev, m, good, out=dev)
    with pytest.raises(pkg.ArgumentError):
        pkg.permute_sites(dev, m, good, out=torch.empty(m.N, dtype=torch.float64, device=dev.device))
