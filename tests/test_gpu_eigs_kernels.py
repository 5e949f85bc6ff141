"""The three kernels of csrc/kernels_eigs.hip through their public forms (sd_basis_rotate_dev, sd_block_dots_dev,
sd_block_axpy_dev), in the conventions of test_gpu_blas1_kernels.py: outputs, padding and guard elements are NaN before the
call, a NaN where a value is due or a value where none is due fails, inputs must come back unchanged.

  rotation     bit for bit against eigs_ref.rotate_ref (ascending j from a zero accumulator, multiply then add)
  block dots   against math.fsum of the restatement's own terms, bar n_terms 2^-53 sum |term|: any order of n_terms - 1 additions
               meets it, so it is a condition and not a measurement; two identical calls give identical bits
  block axpy   bit for bit against eigs_ref.block_axpy_ref

Sizes: N in {1, 2, 3, 255, 256, 257}; then where the capped grids (2048 blocks of 256 threads) wrap: 524 289 and 524 290 (one
item per row or element), 1 048 577 and 1 048 578 (the 16-byte forms: one item per pair of doubles; 1 048 577 with ld = N + 3
is the pair form with an odd tail row).  ld in {N, N + 3}: N + 3 flips the parity of ld, hence the form.

Figures on an MI355X: every rotation and subtraction cell bit for bit; block dots, largest |dot - fsum| / bar: 0.34 (N = 3, where
the bar is 3 ulp), 1.5e-3 (N = 255 ... 257), 1.8e-8 (past the caps).  50 tests in 17 s, the slowest cell 1.6 s (the fsum of the
complex terms at 524 289 elements)."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import eigs_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
U = 2.0 ** -53
SMALL = [1, 2, 3, 255, 256, 257]
WRAP = [R.MAX_BLOCKS * 256 + 1, R.MAX_BLOCKS * 256 + 2, 2 * R.MAX_BLOCKS * 256 + 1, 2 * R.MAX_BLOCKS * 256 + 2]
MK_ALL = [(1, 1), (2, 1), (2, 2), (9, 8), (33, 32), (128, 1), (128, 32)]
MK_WRAP = [(3, 2), (24, 10)]
_dp = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def e(pkg):
    import torch
    from types import SimpleNamespace
    ctx = pkg.default_context()
    yield SimpleNamespace(pkg=pkg, ctx=ctx, torch=torch, dev=torch.device("cuda", ctx.device), lib=pkg.lib())
    _dot_inputs.cache_clear()
    torch.cuda.empty_cache()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def rotate(e, buf, off, ld, n, m, Q, k):
    e.ctx.set_stream(e.torch.cuda.current_stream().cuda_stream)
    Qf = np.asfortranarray(Q[:, :k], dtype=np.float64)
    return e.lib.sd_basis_rotate_dev(e.ctx.h, buf.data_ptr() + 8 * off, ld, n, m, Qf.ctypes.data_as(_dp), k)


def rotation_cell(e, rng, N, m, k, ld, off, Q=None, data=None):
    """one rotation of an (m, N) basis stored `ld` apart, `off` doubles past an aligned base; everything else NaN.  Returns
    (data, Q, result rows) after the bit-for-bit checks of the untouched parts."""
    t = e.torch
    data = rng.standard_normal((m, N)) if data is None else data
    Q = rng.standard_normal((m, k)) if Q is None else Q
    host = np.full(off + m * ld + 3, NAN)
    cols = host[off:off + m * ld].reshape(m, ld)
    cols[:, :N] = data
    buf = t.from_numpy(host).to(e.dev)
    assert buf.data_ptr() % 256 == 0
    e.pkg.check(rotate(e, buf, off, ld, N, m, Q, k), e.ctx.h)
    got = buf.cpu().numpy()
    want = host.copy()
    want[off:off + m * ld].reshape(m, ld)[:k, :N] = 0.0          # the rotated part is compared by the caller
    chk = got.copy()
    res = chk[off:off + m * ld].reshape(m, ld)[:k, :N].copy()
    chk[off:off + m * ld].reshape(m, ld)[:k, :N] = 0.0
    assert np.array_equal(bits(chk), bits(want)), "a column >= k, a padding row or a guard element changed"
    return data, Q, res


@pytest.mark.parametrize("N", SMALL)
def test_rotation_bit_for_bit_small(e, N):
    rng = np.random.default_rng(1000 + N)
    cells = 0
    for (m, k) in MK_ALL:
        for ld in (N, N + 3):
            for off in (0, 1):                                   # off = 1: a base that is not 16-byte aligned
                data, Q, res = rotation_cell(e, rng, N, m, k, ld, off)
                assert np.array_equal(bits(res), bits(R.rotate_ref(data, Q, k))), (N, m, k, ld, off)
                cells += 1
    assert cells == 28


def test_rotation_of_a_complex_basis_as_2n_doubles(e):
    """Ritz coefficients are real: a ComplexF64 basis is rotated as 2 N doubles, which is the complex product with a real Q"""
    rng = np.random.default_rng(7)
    N, m, k = 257, 9, 8
    z = rng.standard_normal((m, N)) + 1j * rng.standard_normal((m, N))
    data = np.ascontiguousarray(z).view(np.float64).reshape(m, 2 * N)
    _, Q, res = rotation_cell(e, rng, 2 * N, m, k, 2 * N, 0, data=data)
    assert np.array_equal(bits(res), bits(R.rotate_ref(data, Q, k)))
    want = (z.T @ Q).T
    assert np.abs(res.view(np.complex128) - want).max() <= 4 * m * U * np.abs(z).max() * np.abs(Q).max() * m


@pytest.mark.parametrize("N", WRAP)
def test_rotation_bit_for_bit_where_the_grid_wraps(e, N):
    """Both forms past 2048 blocks: one row per thread wraps at 524 289 rows, one row pair per thread at 1 048 577."""
    rng = np.random.default_rng(N)
    for (m, k) in MK_WRAP:
        for ld in (N, N + 3):
            pair = ld % 2 == 0
            items = (N + 1) // 2 if pair else N
            if N >= WRAP[2] or not pair:
                assert items > R.MAX_BLOCKS * 256                # this cell wraps
            data, Q, res = rotation_cell(e, rng, N, m, k, ld, 0)
            assert np.array_equal(bits(res), bits(R.rotate_ref(data, Q, k))), (N, m, k, ld)


def test_rotation_permutation_zero_rows_and_nan(e):
    rng = np.random.default_rng(3)
    N, m, k = 257, 9, 8
    # a permutation matrix reproduces the permuted columns exactly
    perm = rng.permutation(m)
    Q = np.zeros((m, k))
    Q[perm[:k], np.arange(k)] = 1.0
    data, _, res = rotation_cell(e, rng, N, m, k, N + 3, 0, Q=Q)
    assert np.array_equal(bits(res), bits(data[perm[:k]]))
    # a zero row of Q: the column's finite data leaves no trace
    Q = rng.standard_normal((m, k))
    Q[4, :] = 0.0
    data, _, res = rotation_cell(e, rng, N, m, k, N, 0, Q=Q)
    other = data.copy()
    other[4] = rng.standard_normal(N) * 1e6
    _, _, res2 = rotation_cell(e, rng, N, m, k, N, 0, Q=Q, data=other)
    assert np.array_equal(bits(res), bits(res2))
    # ... but a NaN in it propagates: the kernel multiplies and adds every term (0 * NaN = NaN).  A later "skip zero weights"
    # optimisation would change this and must be a visible change.
    other = data.copy()
    other[4, 100] = NAN
    _, _, res3 = rotation_cell(e, rng, N, m, k, N, 0, Q=Q, data=other)
    assert np.isnan(res3[:, 100]).all()
    keep = np.arange(N) != 100
    assert np.array_equal(bits(res3[:, keep]), bits(res[:, keep]))


def test_rotation_argument_errors(e):
    t = e.torch
    buf = t.zeros(129 * 8 + 8, dtype=t.float64, device=e.dev)
    Q = np.zeros((129, 33))
    for (m, k) in ((2, 3), (129, 1), (40, 33), (0, 0), (3, 0)):
        rc = rotate(e, buf, 0, 8, 8, m, Q[:max(m, 1)], k)
        assert rc == 1, (m, k)                                                     # SD_EARG
        with pytest.raises(e.pkg.ArgumentError, match="basis rotation"):
            e.pkg.check(rc, e.ctx.h)
    assert t.count_nonzero(buf).item() == 0


# ---- block dots / block axpy ----

@functools.lru_cache(maxsize=2)
def _dot_inputs(N, cplx):
    """8 columns and w of N elements with the fsum of every column's dot terms (shared by the cells of one N: read-only)"""
    rng = np.random.default_rng(50 + N + cplx)
    if cplx:
        V = rng.standard_normal((8, N)) + 1j * rng.standard_normal((8, N))
        w = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    else:
        V, w = rng.standard_normal((8, N)), rng.standard_normal(N)
    sums = []
    for (re, im) in R.block_dots_terms(V, w):
        sums.append((math.fsum(re), math.fsum(im), len(re) * U * math.fsum(np.abs(re)), len(im) * U * math.fsum(np.abs(im))))
    V.setflags(write=False)
    w.setflags(write=False)
    return V, w, sums


def device_cols(e, V, ld):
    t = e.torch
    cplx = np.iscomplexobj(V)
    out = t.full((V.shape[0], ld), complex(NAN, NAN) if cplx else NAN, dtype=t.complex128 if cplx else t.float64, device=e.dev)
    out[:, :V.shape[1]] = t.from_numpy(np.array(V))
    return out


def device_vec(e, w):
    t = e.torch
    cplx = np.iscomplexobj(w)
    buf = t.full((len(w) + 4,), complex(NAN, NAN) if cplx else NAN, dtype=t.complex128 if cplx else t.float64, device=e.dev)
    buf[2:2 + len(w)] = t.from_numpy(np.array(w))
    return buf, buf[2:2 + len(w)]


def same_bits(t, host):
    return np.array_equal(bits(t.cpu().numpy().view(np.float64)), bits(np.ascontiguousarray(host).view(np.float64)))


def dots_cells(e, N, cplx):
    V, w, sums = _dot_inputs(N, cplx)
    code = 2 if cplx else 1
    worst = 0.0
    for ld in (N, N + 3):
        Vd = device_cols(e, V, ld)
        v0 = Vd.cpu().numpy()
        wbuf, wd = device_vec(e, w)
        w0 = wbuf.cpu().numpy()
        for ncols in (1, 7, 8):
            outs = []
            for _ in range(2):
                out = np.full(2 * 8 + 2, NAN)
                e.ctx.set_stream(e.torch.cuda.current_stream().cuda_stream)
                e.pkg.check(e.lib.sd_block_dots_dev(e.ctx.h, code, Vd.data_ptr(), ld, ncols, wd.data_ptr(), N, out.ctypes.data_as(_dp)),
                            e.ctx.h)
                outs.append(out)
            assert np.array_equal(bits(outs[0]), bits(outs[1])), "two identical calls differ"
            out = outs[0]
            assert np.isnan(out[2 * ncols:]).all(), "written past 2 per column"
            for c in range(ncols):
                sre, sim, bre, bim = sums[c]
                assert abs(out[2 * c] - sre) <= bre, (N, ld, ncols, c, out[2 * c], sre, bre)
                worst = max(worst, abs(out[2 * c] - sre) / bre)
                if cplx:
                    assert abs(out[2 * c + 1] - sim) <= bim, (N, ld, ncols, c, out[2 * c + 1], sim, bim)
                    worst = max(worst, abs(out[2 * c + 1] - sim) / bim)
                else:
                    assert out[2 * c + 1] == 0.0
        assert same_bits(Vd, v0) and same_bits(wbuf, w0), "an input changed"
    print(f"N={N} complex={cplx}: largest |dot - fsum| / bar = {worst:.3g}")
    return V, w, sums


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("N", SMALL)
def test_block_dots_small(e, N, cplx):
    V, w, sums = dots_cells(e, N, cplx)
    if cplx:
        # a missing conjugate fails: the plain product sum of column 0 lies outside the bar of the Hermitian one
        plain = math.fsum(np.concatenate([V[0].real * w.real, -(V[0].imag * w.imag)]))
        assert abs(plain - sums[0][0]) > sums[0][2]


@pytest.mark.parametrize("N", WRAP)
def test_block_dots_where_the_grid_wraps_f64(e, N):
    dots_cells(e, N, False)


@pytest.mark.parametrize("N", WRAP[:2])
def test_block_dots_where_the_grid_wraps_c128(e, N):
    """one complex element per thread: the grid wraps at 524 289 elements"""
    dots_cells(e, N, True)


def axpy_cells(e, N, cplx, ncols_list=(1, 7, 8)):
    V, w, _ = _dot_inputs(N, cplx)
    rng = np.random.default_rng(N)
    code = 2 if cplx else 1
    for ld in (N, N + 3):
        Vd = device_cols(e, V, ld)
        v0 = Vd.cpu().numpy()
        for ncols in ncols_list:
            coef = rng.standard_normal(8) + 1j * rng.standard_normal(8)
            cf = np.ascontiguousarray(coef).view(np.float64).copy()
            wbuf, wd = device_vec(e, w)
            e.ctx.set_stream(e.torch.cuda.current_stream().cuda_stream)
            e.pkg.check(e.lib.sd_block_axpy_dev(e.ctx.h, code, wd.data_ptr(), Vd.data_ptr(), ld, ncols, cf.ctypes.data_as(_dp), N),
                        e.ctx.h)
            got = wbuf.cpu().numpy()
            assert np.isnan(got[:2].view(np.float64)).all() and np.isnan(got[2 + N:].view(np.float64)).all(), "a guard element was written"
            want = R.block_axpy_ref(np.array(w), V[:ncols], coef[:ncols] if cplx else coef[:ncols].real)
            assert np.array_equal(bits(got[2:2 + N].view(np.float64)), bits(want.view(np.float64))), (N, ld, ncols)
        assert same_bits(Vd, v0), "an input changed"


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("N", SMALL)
def test_block_axpy_bit_for_bit_small(e, N, cplx):
    axpy_cells(e, N, cplx)


@pytest.mark.parametrize("N", WRAP)
def test_block_axpy_where_the_grid_wraps_f64(e, N):
    axpy_cells(e, N, False)


@pytest.mark.parametrize("N", WRAP[:2])
def test_block_axpy_where_the_grid_wraps_c128(e, N):
    axpy_cells(e, N, True)


def test_block_kernels_argument_errors(e):
    t = e.torch
    x = t.zeros(64, dtype=t.float64, device=e.dev)
    out = np.zeros(32)
    for ncols in (0, 9):
        assert e.lib.sd_block_dots_dev(e.ctx.h, 1, x.data_ptr(), 4, ncols, x.data_ptr(), 4, out.ctypes.data_as(_dp)) == 1
        assert e.lib.sd_block_axpy_dev(e.ctx.h, 1, x.data_ptr(), x.data_ptr(), 4, ncols, out.ctypes.data_as(_dp), 4) == 1
    assert e.lib.sd_block_dots_dev(e.ctx.h, 3, x.data_ptr(), 4, 1, x.data_ptr(), 4, out.ctypes.data_as(_dp)) == 1
