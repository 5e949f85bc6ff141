"""The yardstick of tests/test_gpu_blas1_kernels.py: numpy restatements of what the comments of csrc/kernels_blas1.hip fix -- the
order of the list sums (gs_sum_cols, k_bgs_reduce, k_mdot_reduce), the per-element arithmetic of every pass as separately rounded
IEEE operations in the stated order (the library is compiled with -ffp-contract=off; numpy rounds after every ufunc) -- the two
Gram-Schmidt chains in np.longdouble, a forward error bound for them, and the build of tests/blas1_shim.cpp.
tests/test_blas1_ref_host.py proves every function here against exact rational arithmetic, without a GPU."""
import ctypes as C
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53                      # unit roundoff of an IEEE double
SD_BGS_B = 8                        # columns of a Gram-Schmidt block
SD_MDOT_MAXC = 16                   # columns of a k_mdot launch
SD_CCOMB_MAXC = 16                  # columns of a k_ccombine launch
SD_GEMV_MAXC = 256                  # columns of a k_gemv_cols launch
LD = np.longdouble
assert np.finfo(LD).nmant >= 63, "np.longdouble must be the 80-bit extended type (64-bit significand) or wider"


# ---- list sums ----
def sum_cols(lst, nb, stride, col):
    """column `col` of a list of nb rows of `stride` doubles, summed in the order of gs_sum_cols / k_bgs_reduce / k_mdot_reduce:
    lane l of 64 adds the entries l, l + 64, ... one after the other to 0.0; then for off = 32, 16, ..., 1 lane l < off adds lane
    l + off; the result is lane 0's."""
    x = np.asarray(lst, dtype=np.float64).reshape(-1)[col::stride][:nb]
    assert len(x) == nb
    lanes = np.zeros(64)
    for lo in range(0, nb, 64):
        chunk = x[lo:lo + 64]
        lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
    off = 32
    while off > 0:
        lanes[:off] = lanes[:off] + lanes[off:2 * off]
        off >>= 1
    return float(lanes[0])


# ---- elementwise forms (Float64) ----
def proj(x, cf, cols):
    """the blocked projection: x = x - cf[c] * v_c for c ascending (k_gs_pass, k_proj_dots, k_sub_dot)"""
    x = np.array(x, dtype=np.float64)
    for c, v in zip(cf, cols):
        x = x - np.float64(c) * v
    return x


def update(w, a, vj, b=None, vjm1=None):
    """(w - a*vj) - b*vjm1, or w - a*vj without vjm1 (k_gs_update; sd_k_sub2 with and without u)"""
    x = w - np.float64(a) * vj
    if vjm1 is not None:
        x = x - np.float64(b) * vjm1
    return x


def correct(w, d, vjm1):
    """w - d*vjm1 (k_gs_correct)"""
    return w - np.float64(d) * vjm1


def scale(w, b):
    """w / b, a true division (k_gs_scale, sd_k_scale_div)"""
    return w / np.float64(b)


def gemv_cols(V, coef, y=None):
    """y[i] = sum_k V[k][i] * coef[k] as sd_k_gemv_cols forms it: groups of 256 columns, s = 0.0 in the first group and s = y in
    the later ones, then s += V[k][i] * coef[k] with k ascending.  V: (ncols, N), one row per column.  y (any content, NaN in the
    tests) is what the vector held before: no group may use it, and with ncols = 0 nothing is launched and it stays."""
    s = None if y is None else np.array(y, dtype=np.float64)
    for k0 in range(0, len(coef), SD_GEMV_MAXC):
        s = np.zeros(V.shape[1]) if k0 == 0 else s
        for k in range(k0, min(k0 + SD_GEMV_MAXC, len(coef))):
            s = s + V[k] * np.float64(coef[k])
    return s


# ---- elementwise forms (ComplexF64, component-wise) ----
def parts(z):
    return np.ascontiguousarray(z.real), np.ascontiguousarray(z.imag)


def join(re, im):
    z = np.empty(len(re), dtype=np.complex128)
    z.real, z.imag = re, im
    return z


def ccombine(cols, cr, ci, y=None, init=True):
    """acc += (cr*x.re - ci*x.im, cr*x.im + ci*x.re) column by column, from 0 when init is set and from y otherwise (k_ccombine;
    sd_k_ccombine sets init on the first group of 16 alone, so all groups together are one call of this with init=True)"""
    n = len(cols[0]) if len(cols) else len(y)
    ar, ai = (np.zeros(n), np.zeros(n)) if init else parts(y)
    for x, r, i in zip(cols, cr, ci):
        xr, xi = parts(x)
        r, i = np.float64(r), np.float64(i)
        tr, ti = r * xr - i * xi, r * xi + i * xr
        ar, ai = ar + tr, ai + ti
    return join(ar, ai)


def cheb_init(x0, x1, c0, c1, have1):
    """t = 0; t += c0*x0; if have1: t += c1*x1, component-wise (k_cheb_init)"""
    return ccombine([x0, x1] if have1 else [x0], [c0.real, c1.real], [c0.imag, c1.imag])


def promote(x, nc):
    """a complex vector from nc = 1 (real, zero imaginary parts) or nc = 2 (interleaved re, im) doubles (k_promote)"""
    x = np.asarray(x, dtype=np.float64)
    return join(x, np.zeros(len(x))) if nc == 1 else join(x[0::2], x[1::2])


# ---- the Gram-Schmidt chains in extended precision ----
def _chain_longdouble(w, V, ncols, block):
    x = np.asarray(w, dtype=np.float64).astype(LD)
    coefs = []
    for c0 in range(0, ncols - 1, block):
        cs = range(c0, min(c0 + block, ncols - 1))
        cf = [(V[c].astype(LD) * x).sum(dtype=LD) for c in cs]          # the dots with w as it stands when the block begins
        for c, f in zip(cs, cf):
            x = x - f * V[c].astype(LD)
        coefs += cf
    last = (V[ncols - 1].astype(LD) * x).sum(dtype=LD)
    return x, coefs, last


def bgs_longdouble(w, V, ncols):
    """sd_k_bgs_chain / sd_k_gs_chain in np.longdouble: columns 0..ncols-2 of V (one row per column) projected out of w in blocks
    of 8, the coefficients of a block being its dots with w as it stands when the block begins, subtraction in column order
    -> (w_new, coefficients, V[ncols-1] . w_new), all longdouble"""
    return _chain_longdouble(w, V, ncols, SD_BGS_B)


def mgs_longdouble(w, V, ncols):
    """sd_k_mgs_chain in np.longdouble: the sequential chain, every coefficient from the current w"""
    return _chain_longdouble(w, V, ncols, 1)


def chain_bound(w, V, ncols, block):
    """|got_i - ref_i| <= bound_i for the double-precision chain against the longdouble one: -> bound (N doubles).

    With u = 2^-53, n_proj = ncols - 1 projected columns, c_c the coefficients and N the length:
      bound_i = 1.01 * [ sum_c (delta_c + rho_c) |v_ci|  +  2 (n_proj + 1) u (|w_i| + sum_c |c_c v_ci|) ]
      delta_c = N u sum_i |v_ci w_i|       any order of N products and N - 1 additions of the dot with the block's own w
      rho_c   = sum over columns k of EARLIER blocks of (delta_k + rho_k) (|G_ck| + N u)  +  |v_c|_2 |R|_2
    The second term of bound_i, R_i, covers the two roundings per column of x - c*v (u|c v| + u|x_new| <= 2u(|x| + |c v|), and
    |x| <= |w| + sum |c v| at every stage).  rho_c is the propagated term: a later block's coefficient is formed from the computed
    w, which carries the earlier blocks' coefficient errors (delta_k + rho_k) v_k and rounding errors R.  Dotted with v_c the first
    are multiplied by G_ck = v_c . v_k (near zero: the columns are orthonormal; computed here in double, hence the + N u), the
    second by at most |v_c|_2 |R|_2 (Cauchy-Schwarz).  The factor 1.01 covers the second-order terms (products of two of the
    above, below 1e-6 of the bound) and the longdouble reference's own error (N 2^-64 per dot against N 2^-53 here)."""
    w = np.asarray(w, dtype=np.float64)
    N, nproj = len(w), ncols - 1
    x = w.copy()
    absum = np.zeros(N)                 # sum_c |c_c v_ci|
    coef_err = np.zeros(nproj)          # delta_c + rho_c
    G = np.abs(V[:nproj] @ V[:nproj].T) + N * U if nproj else np.zeros((0, 0))
    delta, cf = np.zeros(nproj), np.zeros(nproj)
    for c0 in range(0, nproj, block):
        cs = range(c0, min(c0 + block, nproj))
        for c in cs:
            cf[c] = float(V[c] @ x)
            delta[c] = N * U * float(np.abs(V[c] * x).sum())
        for c in cs:
            x = x - cf[c] * V[c]
            absum += np.abs(cf[c] * V[c])
    R = 2 * (nproj + 1) * U * (np.abs(w) + absum)
    Rn = float(np.linalg.norm(R))
    for c0 in range(0, nproj, block):
        for c in range(c0, min(c0 + block, nproj)):
            coef_err[c] = delta[c] + float(G[c, :c0] @ coef_err[:c0]) + float(np.linalg.norm(V[c])) * Rn
    first = np.zeros(N)
    for c in range(nproj):
        first += coef_err[c] * np.abs(V[c])
    return 1.01 * (first + R)


# ---- the shim ----
_vp, _dp, _i, _i64, _d = C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_double      # device and host addresses as integers
SHIM_PROTOTYPES = {
    "b1_addr_of_sd_device_count": (_vp, []),
    "b1_gs_blocks": (_i, [_i64]),
    "b1_lanczos_fold_blocks": (_i, [_i64]),
    "b1_gs_chain": (_i, [_vp, _dp, _dp, _i64, _i, _i64, _dp, _dp, _dp, _dp]),
    "b1_gs_update": (_i, [_vp, _dp, _dp, _dp, _i64, _dp, _dp, _dp, _dp, _dp, _dp]),
    "b1_gs_scale": (_i, [_vp, _dp, _dp, _i64, _dp, _dp]),
    "b1_mgs_chain": (_i, [_vp, _dp, _dp, _i64, _i, _i64, _i]),
    "b1_bgs_chain": (_i, [_vp, _dp, _dp, _i64, _i, _i64, _i]),
    "b1_read_scalars": (_i, [_vp, _i, _i, _dp]),
    "b1_mdot": (_i, [_vp, _dp, _i64, _i, _dp, _i64, _dp]),
    "b1_gemv_cols": (_i, [_vp, _dp, _dp, _i64, _i, _dp]),
    "b1_ccombine": (_i, [_vp, _dp, _dp, _i64, _i, _dp, _dp]),
    "b1_cheb_init": (_i, [_vp, _dp, _dp, _dp, _i64, _d, _d, _d, _d, _i]),
    "b1_promote": (_i, [_vp, _dp, _dp, _i, _i64]),
    "b1_sub2": (_i, [_vp, _dp, _dp, _dp, _i64, _d, _d]),
    "b1_scale_div": (_i, [_vp, _dp, _dp, _i64, _d]),
    "b1_dotu": (_i, [_vp, _dp, _dp, _i64, _i]),
    "b1_imag_count": (_i, [_vp, _dp, _i64, _i]),
    "b1_dot_to": (_i, [_vp, _i, _dp, _dp, _i64, _dp]),
    "b1_nrm2sq_to": (_i, [_vp, _dp, _i64, _dp]),
    "b1_lanczos_fold": (_i, [_vp, _dp, _dp, _dp, _i64, _i, _dp, _dp, _dp, _dp, _dp, _dp]),
    "b1_lanczos_fold_p": (_i, [_vp, _dp, _dp, _dp, _i64, _i, _i64, _i, _dp, _i, _dp, _dp, _i, _dp, _dp, _i64, _dp, _i]),
    "b1_lanczos_fold_scalars_p": (_i, [_vp, _i, _i, _dp, _i, _dp, _i, _dp, _dp, _i64]),
    "b1_lanczos_fold_scalars": (_i, [_vp, _i, _dp, _dp, _dp, _dp]),
}


def build_shim(pkg, outdir):
    """tests/blas1_shim.cpp compiled with the host compiler and linked against the library the package has loaded -> the ctypes
    handle.  A compile or link failure is an assertion failure; so is a shim bound to another instance of the library."""
    pkg.lib()                                                              # libspindyn.so is loaded first
    lib_path = os.path.abspath(pkg._lib.LIB_PATH)
    libdir, out = os.path.dirname(lib_path), os.path.join(str(outdir), "libblas1_shim.so")
    cmd = ["g++", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "blas1_shim.cpp"),
           "-o", out, "-L", libdir, "-l:" + os.path.basename(lib_path), "-Wl,-rpath," + libdir, "-Wl,--no-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    shim = C.CDLL(out)
    for name, (res, args) in SHIM_PROTOTYPES.items():
        fn = getattr(shim, name)
        fn.restype, fn.argtypes = res, args
    seen_by_package = C.cast(pkg.lib().sd_device_count, C.c_void_p).value
    assert shim.b1_addr_of_sd_device_count() == seen_by_package, "the shim is bound to another instance of libspindyn.so"
    return shim
