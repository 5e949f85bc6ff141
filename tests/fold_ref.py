"""The yardstick of tests/test_gpu_fold_kernels.py: numpy restatements of the Lanczos fold family of csrc/kernels_blas1.hip --
fold_resolve (alpha = dot / nc, a true division), fold_elem<FORM, HAVE_U> (the three-term update per element, every operation
rounded on its own: the library is compiled with -ffp-contract=off, numpy rounds after every ufunc), the order in which a block of
256 threads sums a list of pairs (sum_list / block_reduce2 and sum_lists3) and the per-block |w|^2 partials of k_lanczos_fold_p.
No square root is taken here: where one is needed the caller brings the device's own.
tests/test_fold_ref_host.py proves every function here against exact rational arithmetic, without a GPU."""
import numpy as np

from blas1_ref import join, parts

BS = 256                            # threads of every fold block
WAVE = 64


# ---- the inputs of the GPU cells (here, so that the CPU proofs can show that these very inputs tell the forms and orders apart) ----
DOT = (0.8314, -0.4127)             # <u_cur|t> of the cells that pass summed scalars


def norms(N, balanced=False):
    """(|u_cur|^2, |u_prev|^2) of the GPU cells: O(N), the squared norms of the normal vectors they go with -- then
    beta v_prev = b_c u_prev / b_p is O(1) per element, w = t / b_c is O(N^-1/2) and alpha v O(N^-3/2), each still far above the
    last bit of the result.  balanced: O(1), so that alpha and beta are O(1) and the three terms of the update are of one size
    (the regime in which the two associations of forms 0 and 1 differ most often)."""
    s = 1.0 if balanced else float(N)
    return 1.3719 * s, 0.7731 * s


def vectors(N, seed):
    """t, uc, up: seeded complex normal vectors of N elements, read-only"""
    rng = np.random.default_rng([seed, N])
    out = []
    for _ in range(3):
        z = np.empty(N, dtype=np.complex128)
        z.view(np.float64)[:] = rng.standard_normal(2 * N)
        z.setflags(write=False)
        out.append(z)
    return out


def dot_list(n, seed):
    """n pairs whose sums are O(1) in both components, every entry finite and non-zero (flat: re, im, re, im, ...)"""
    rng = np.random.default_rng([seed, n, 1])
    x = rng.standard_normal(2 * n) / np.sqrt(n) + 0.7 / n
    assert x.all()
    return x


def n2_list(n, seed, total):
    """n pairs (p, 0.0) with p > 0 summing to about `total`, as the |w|^2 producers leave them"""
    rng = np.random.default_rng([seed, n, 2])
    x = np.zeros(2 * n)
    x[0::2] = rng.uniform(0.5, 1.5, n) * (total / n)
    return x


def alpha(form, dot, nc=None):
    """fold_resolve: (ar, ai) = (dot[0] / nc, dot[1] / nc in form 2 and 0.0 otherwise); nc = None stands for a null n2c, i.e. 1.0"""
    nc = np.float64(1.0 if nc is None else nc)
    with np.errstate(divide="ignore", invalid="ignore"):                 # a column that broke down divides by zero: plain IEEE
        return float(np.float64(dot[0]) / nc), float(np.float64(dot[1]) / nc) if form == 2 else 0.0


def fold_elem(form, t, uc, up, ar, ai, bc, bp):
    """fold_elem<form, up is not None> on complex vectors, component-wise:  w = t / bc, v = uc / bc, u = up / bp (true divisions;
    bc = 1.0 / bp = 1.0 for a null n2c / n2p), beta = bc, and then
      form 0   w - (ar*v + bc*u)            without u:  w - ar*v
      form 1   (w - ar*v) - bc*u            without u:  w - ar*v
      form 2   (wx - (ar*vx - ai*vy)) - bc*ux,  (wy - (ar*vy + ai*vx)) - bc*uy       without u: the first bracket alone"""
    ar, ai, bc, bp = np.float64(ar), np.float64(ai), np.float64(bc), np.float64(bp)
    tx, ty = parts(t)
    cx, cy = parts(uc)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        wx, wy, vx, vy = tx / bc, ty / bc, cx / bc, cy / bc
        if up is not None:
            px, py = parts(up)
            ux, uy = px / bp, py / bp
        if form == 0:
            if up is not None:
                return join(wx - (ar * vx + bc * ux), wy - (ar * vy + bc * uy))
            return join(wx - ar * vx, wy - ar * vy)
        if form == 1:
            rx, ry = wx - ar * vx, wy - ar * vy
        else:
            assert form == 2
            rx, ry = wx - (ar * vx - ai * vy), wy - (ar * vy + ai * vx)
        if up is not None:
            rx, ry = rx - bc * ux, ry - bc * uy
        return join(rx, ry)


def block_reduce256(lanes):
    """block_reduce2 of a 256-thread block on the last axis of `lanes` (..., 256): in each of the four waves lane l < off adds lane
    l + off for off = 32, 16, ..., 1; then 0.0 + wave0 + wave1 + wave2 + wave3 in that order -> (...)"""
    w = np.array(lanes, dtype=np.float64).reshape(lanes.shape[:-1] + (BS // WAVE, WAVE))
    with np.errstate(invalid="ignore", over="ignore"):
        off = WAVE // 2
        while off > 0:
            w[..., :off] = w[..., :off] + w[..., off:2 * off]
            off >>= 1
        s = np.zeros(w.shape[:-2])
        for k in range(BS // WAVE):
            s = s + w[..., k, 0]
    return s


def sum_list256(lst, n, comp):
    """component `comp` of a list of n pairs as sum_list and sum_lists3 add it: thread th of 256 adds the entries th, th + 256,
    ... one after the other to 0.0; then block_reduce256"""
    x = np.asarray(lst, dtype=np.float64).reshape(-1)[comp::2][:n]
    assert len(x) == n
    lanes = np.zeros(BS)
    with np.errstate(invalid="ignore", over="ignore"):
        for lo in range(0, n, BS):
            chunk = x[lo:lo + BS]
            lanes[:len(chunk)] = lanes[:len(chunk)] + chunk
    return float(block_reduce256(lanes))


def norm_terms(r):
    """the term an element adds to |w|^2: fl(fl(r.x^2) + fl(r.y^2))"""
    rx, ry = parts(r)
    with np.errstate(invalid="ignore", over="ignore"):
        return rx * rx + ry * ry


def fold_p_partials(r, N, nb):
    """the nb per-block |w|^2 partials k_lanczos_fold_p writes for the updated vector r: thread th of block b adds norm_terms for
    i = b*256 + th, + nb*256, ... one after the other to 0.0; then block_reduce256 -> nb doubles"""
    terms = norm_terms(r[:N])
    stride = nb * BS
    trips = -(-N // stride)
    s = np.zeros(stride)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(trips):
            chunk = terms[k * stride:(k + 1) * stride]
            s[:len(chunk)] = s[:len(chunk)] + chunk
    return block_reduce256(s.reshape(nb, BS))
