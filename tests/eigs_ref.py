"""numpy restatements of the thick-restart eigen-solver: the arithmetic of its three kernels in the order the
library fixes, and the whole algorithm of sd_lanczos_eigenpairs with numpy's eigh for the projected problem."""
import numpy as np

U = 2.0 ** -53          # unit roundoff
BLOCK_COLS = 8          # columns of one Gram-Schmidt block
MAX_KEEP = 32
MAX_BLOCKS = 2048       # most blocks (256 threads) of one pass of the kernels: where their grid-stride loops wrap


def rotate_ref(V, Q, k):
    """V: (m, ld) array of columns (row c = column c of the basis), Q: (m, k).  Returns the k new columns over the whole ld:
    sum_j V[j] * Q[j, c] in ascending j from a zero accumulator, one multiply then one add per term."""
    m = V.shape[0]
    out = np.zeros((k, V.shape[1]))
    for c in range(k):
        acc = np.zeros(V.shape[1])
        for j in range(m):
            acc = acc + V[j] * Q[j, c]
        out[c] = acc
    return out


def block_dots_terms(V, w):
    """The products a block dot sums, per column: complex vectors give (re terms, im terms) of conj(v) * w -- two real
    products per element and part -- real ones (terms, [])."""
    out = []
    for v in V:
        if np.iscomplexobj(w):
            re = np.concatenate([v.real * w.real, v.imag * w.imag])
            im = np.concatenate([v.real * w.imag, -(v.imag * w.real)])
            out.append((re, im))
        else:
            out.append((v * w, np.zeros(0)))
    return out


def block_axpy_ref(w, V, coef):
    """w - sum_c coef[c] V[c] in ascending c: real x = x - cr v; complex re = (re - cr v.re) + ci v.im, im = (im - cr v.im) - ci v.re."""
    if np.iscomplexobj(w):
        re, im = w.real.copy(), w.imag.copy()
        for v, cf in zip(V, coef):
            cr, ci = float(np.real(cf)), float(np.imag(cf))
            re = (re - cr * v.real) + ci * v.imag
            im = (im - cr * v.imag) - ci * v.real
        return re + 1j * im
    x = w.copy()
    for v, cf in zip(V, coef):
        x = x - float(np.real(cf)) * v
    return x


def trlan_ref(apply, N, nev, basis_size, tol, confirm, seed_vectors, max_applies=0):
    """sd_lanczos_eigenpairs in numpy.  apply(x) -> H x; seed_vectors: an iterable of vectors of length N, the first is the
    start vector and the following ones the fresh vectors of breakdowns and confirmation steps.  Returns (E, X, info) with info
    a dict: restarts, applies, next_level (or None), scale, converged."""
    seeds = iter(seed_vectors)
    mb = min(basis_size, N)
    first = np.asarray(next(seeds))
    V = np.zeros((N, mb), dtype=first.dtype)
    st = {"c": 0, "l": 0, "scale": 0.0, "scale_run": 0.0, "applies": 0, "restarts": 0}
    lam, th, s = [], [], []

    def cgs2(x, ncols):
        h = np.zeros(ncols, dtype=V.dtype)
        for _ in range(2):
            g = V[:, :ncols].conj().T @ x
            x = x - V[:, :ncols] @ g
            h += g
        return x, h

    def seat(x):
        if st["c"] > 0:
            x, _ = cgs2(x, st["c"])
        nrm = np.linalg.norm(x)
        if not (nrm > 0 and np.isfinite(nrm)):
            return False
        V[:, st["c"]] = x / nrm
        st["l"] = 0
        return True

    def run(target):
        """-> 'ok' | 'stopped' | 'exhausted'"""
        nonlocal th, s
        while st["c"] < target:
            c, l = st["c"], st["l"]
            mact = mb - c
            T = np.zeros((mact, mact))
            for i in range(l):
                T[i, i] = th[i]
                T[l, i] = T[i, l] = s[i]
            ja, beta, broke, w = l, 0.0, False, None
            for j in range(c + l, mb):
                if max_applies > 0 and st["applies"] >= max_applies:
                    return "stopped"
                w = apply(V[:, j])
                st["applies"] += 1
                w, h = cgs2(w, j + 1)
                alpha, beta = float(np.real(h[j])), float(np.linalg.norm(w))
                jj = j - c
                T[jj, jj] = alpha
                ja = jj + 1
                st["scale_run"] = max(st["scale_run"], abs(alpha))
                if not beta > 1e-12 * st["scale_run"]:
                    broke = True
                    break
                st["scale_run"] = max(st["scale_run"], beta)
                if j + 1 < mb:
                    T[jj + 1, jj] = T[jj, jj + 1] = beta
                    V[:, j + 1] = w / beta
            ev, Z = np.linalg.eigh(T[:ja, :ja])
            st["scale"] = max(st["scale"], abs(ev[0]), abs(ev[-1]))
            st["scale_run"] = max(st["scale_run"], st["scale"])
            bl = 0.0 if broke else beta
            need = target - c
            nconv = 0
            while nconv < ja and nconv < need and abs(bl * Z[ja - 1, nconv]) <= tol * st["scale"]:
                nconv += 1
            kk = nconv
            if not broke:
                buffer = min(8, max(2, (mact - need) // 3))
                kk = max(nconv, min(need + buffer, MAX_KEEP, mact - 1))
            if kk > 0:
                V[:, c:c + kk] = V[:, c:c + ja] @ Z[:, :kk]
                st["restarts"] += 1
            lam.extend(ev[:nconv])
            st["c"] = c = c + nconv
            if broke:
                if c >= target:
                    st["l"] = 0
                    return "ok"
                if not (c < N and c < mb):
                    return "exhausted"
                nxt = next(seeds, None)
                if nxt is None or not seat(np.asarray(nxt, dtype=V.dtype)):
                    return "exhausted"
            else:
                st["l"] = l = kk - nconv
                th = list(ev[nconv:kk])
                s = [bl * Z[ja - 1, nconv + i] for i in range(l)]
                if c + l >= mb:
                    return "exhausted" if c < target else "ok"
                V[:, c + l] = w / beta
        return "ok"

    if not seat(first.copy()):
        raise ZeroDivisionError("starting vector has zero norm")
    state = run(nev)
    next_level = None
    while confirm and state == "ok" and nev <= st["c"] < N and (mb - st["c"] >= 2 or mb == N) and st["c"] < mb:
        c0 = st["c"]
        nxt = next(seeds, None)
        if nxt is None or not seat(np.asarray(nxt, dtype=V.dtype)):
            break
        state = run(c0 + 1)
        if st["c"] == c0:
            break
        mu = lam[-1]
        if mu <= sorted(lam[:c0])[nev - 1] + tol * st["scale"]:
            continue
        next_level = mu
        lam.pop()
        st["c"] = c0
        break
    c = st["c"]
    order = np.argsort(np.asarray(lam[:c]), kind="stable")
    if c > nev:                       # a locked level beyond the window is the next one
        next_level = lam[order[nev]]
    order = order[:nev]
    E = np.asarray([lam[i] for i in order])
    X = V[:, order] / np.linalg.norm(V[:, order], axis=0) if len(order) else V[:, :0]
    info = {"restarts": st["restarts"], "applies": st["applies"], "next_level": next_level, "scale": st["scale"],
            "converged": len(order)}
    return E, X, info
