"""Entanglement of any set of sites: sd_subsystem_gram[_dev] and the Python mirror against tests/subsystem_ref.py (dense
numpy in extended precision, proven on the CPU by tests/test_subsystem_ref_host.py), at small shapes where the whole rho_S is compared.

The permutation copies bits, so the bars are those of tests/test_gpu_entanglement.py unchanged (u = 2^-53):
  Gram entries: |G - G_ref| <= 4 (K + 4) u sqrt(G_aa G_bb), K the environment dimension of the block.
  Eigenvalues: |lambda - lambda_ref| <= eps = d (largest entry bound of the block) / tr.
  S_1: within sum over the eigenvalues of eta(eps), eta(t) = -t ln t; mutual information: the three entropy bars added.
  Negativity: | ||rho^T_B||_1 - ||rho_ref^T_B||_1 | <= sqrt(2^s) ||Delta||_F, Delta bounded entrywise by the Gram bound / tr -- the trace
    norm is 1-Lipschitz in ||.||_1 <= sqrt(D) ||.||_F and the partial transpose preserves ||.||_F -- and ln is 1-Lipschitz above 1
    (the trace norm of a Hermitian matrix of trace 1 is at least 1).
Shapes: L=12 nup=6 and L=13 nup=5 each with a tiled and a per-row plan (SD_SUFFIX_BITS), and the full basis at L=10."""
import ctypes as C
import math

import numpy as np
import pytest

import entanglement_ref as ER
import subsystem_ref as SR

pytestmark = pytest.mark.gpu

_ip = C.POINTER(C.c_int)
SIDE = {"A": 0, "B": 1, "auto": 2}
WORST = {"entry": 0.0, "eig": 0.0, "S": 0.0, "I": 0.0, "EN": 0.0}
# name -> L, nup, SD_SUFFIX_BITS, sd_model_path (0 per row -- also the full basis below L = 12, whose rows are its configurations --, 1 tiled)
SHAPES = {"L12n6-tiled": (12, 6, 8, 1), "L12n6-rows": (12, 6, 4, 0), "L13n5-tiled": (13, 5, 8, 1), "L13n5-rows": (13, 5, 5, 0),
          "full-L10": (10, None, None, 0)}
_models, _states, _refs = {}, {}, {}


def site_sets(L):
    return {"middle block": [5, 6, 7, 8], "two end blocks": [1, 2, L - 1, L], "every other site": list(range(1, L + 1, 2)),
            "last site": [L], "last two sites": [L - 1, L], "descending": [7, 4, 2], "all but one": [s for s in range(1, L + 1) if s != 3]}


def model_of(pkg, name):
    if name not in _models:
        L, nup, ls, path = SHAPES[name]
        with pytest.MonkeyPatch.context() as mp:                # the plan reads SD_SUFFIX_BITS when the model is built
            if ls is None:
                mp.delenv("SD_SUFFIX_BITS", raising=False)
            else:
                mp.setenv("SD_SUFFIX_BITS", str(ls))
            _models[name] = pkg.XXZChain(L, nup=nup)
        assert pkg.lib().sd_model_path(_models[name].h) == path, name
    return _models[name]


def state_of(L, nup, cplx):
    """a seeded random vector, normalised; the same array for every test that asks"""
    if (L, nup, cplx) not in _states:
        n = len(SR.basis(L, nup))
        rng = np.random.default_rng(20261020 + 1000 * L + 7 * (nup if nup is not None else 63) + cplx)
        psi = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)
        psi = np.ascontiguousarray(psi / np.linalg.norm(psi))
        psi.setflags(write=False)
        _states[(L, nup, cplx)] = psi
    return _states[(L, nup, cplx)]


def ref_of(L, nup, sites, side, cplx):
    """{m: (G_ref, K)} keyed like the library's blocks: m = up spins among the listed sites; side B blocks are those of the other sites
    (ascending), computed once and shared"""
    key = (L, nup, tuple(sites), side, cplx)
    if key not in _refs:
        psi = state_of(L, nup, cplx)
        rest = [s for s in range(1, L + 1) if s not in sites]
        A = SR.rho_blocks(psi, L, nup, list(sites)) if side != "B" else None
        B = SR.rho_blocks(psi, L, nup, rest) if side != "A" else None
        out = {}
        for m in (A if A is not None else {(-1 if nup is None else nup - mb): 0 for mb in B}):
            mb = -1 if nup is None else nup - m
            sd = side if side != "auto" else ("A" if A[m][0].shape[0] <= B[mb][0].shape[0] else "B")
            G, K = A[m] if sd == "A" else B[mb]
            if not cplx:
                G = G.real
            out[m] = (G, K)
        _refs[key] = out
    return _refs[key]


def raw_gram(pkg, m, psi, sites, side, n=None, dtype=None, n_el=None, null_out=False, ctx="model", n_sites=None):
    """status and the packed output of sd_subsystem_gram[_dev] called directly; psi a numpy array (host form) or a torch tensor (_dev)"""
    import torch
    dev = isinstance(psi, torch.Tensor)
    cplx = psi.is_complex() if dev else np.iscomplexobj(psi)
    s = None if sites is None else np.ascontiguousarray(sites, dtype=np.intc)
    k = (len(s) if s is not None else 1) if n_sites is None else n_sites
    if n_el is None:
        nb, ne = C.c_int(), C.c_int64()
        rc = pkg.lib().sd_cut_blocks(m.h, k, side, None, 0, C.byref(nb), C.byref(ne))
        n_el = ne.value if rc == 0 else 1
    out = np.full(n_el, np.nan, dtype=np.complex128 if cplx else np.float64)
    code = (pkg._lib.SD_C128 if cplx else pkg._lib.SD_F64) if dtype is None else dtype
    if dev and m.ctx is not None:
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ptr = psi.data_ptr() if dev else psi.ctypes.data
    h = m.ctx.h if ctx == "model" else ctx
    fn = pkg.lib().sd_subsystem_gram_dev if dev else pkg.lib().sd_subsystem_gram
    rc = fn(h, m.h, code, ptr, len(psi) if n is None else n, None if s is None else s.ctypes.data_as(_ip), k, side,
            None if null_out else out.ctypes.data)
    return rc, out


def split(out, blocks):
    return {b.m: out[b.offset:b.offset + b.d * b.d].reshape(b.d, b.d) for b in blocks}


def ratio_to_bound(G, G_ref, K, cplx):
    bound = ER.entry_bound(G_ref, K)
    err = np.abs(np.asarray(G - G_ref, dtype=np.clongdouble if cplx else np.longdouble)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    return float(ratio.max())


def check_blocks(tag, got, ref, cplx):
    worst = 0.0
    assert sorted(got) == sorted(ref), tag
    for mm, (G_ref, K) in ref.items():
        G = got[mm]
        assert G.shape == G_ref.shape, (tag, mm)
        worst = max(worst, ratio_to_bound(G, G_ref, K, cplx))
        if cplx:
            assert np.array_equal(G, G.conj().T), (tag, mm, "not Hermitian to the bit")
            assert (np.diag(G).imag == 0.0).all(), (tag, mm)
        else:
            assert G.dtype == np.float64 and np.array_equal(G, G.T), (tag, mm, "not symmetric to the bit")
    WORST["entry"] = max(WORST["entry"], worst)
    print(f"{tag}: largest |G - G_ref| / bound = {worst:.3e} (bar 1; largest so far {WORST['entry']:.3e})")
    assert worst <= 1.0, (tag, worst)


@pytest.mark.parametrize("name", list(SHAPES))
def test_gram_of_every_site_set_against_the_restatement(pkg, name):
    import torch
    L, nup, _, _ = SHAPES[name]
    m = model_of(pkg, name)
    for cplx in (True, False):
        psi = state_of(L, nup, cplx)
        dev = torch.from_numpy(np.array(psi)).to(torch.device("cuda", m.ctx.device))
        for sname, sites in site_sets(L).items():
            for side in ("A", "auto"):
                if side == "A" and max(math.comb(len(sites), k) for k in range(len(sites) + 1)) > 16384:
                    continue
                blocks = pkg.cut_blocks(m, len(sites), side)             # the layout is the cut's, by contract
                ref = ref_of(L, nup, sites, side, cplx)
                rc, host_out = raw_gram(pkg, m, psi, sites, SIDE[side])
                assert rc == 0, pkg.lib().sd_last_error(m.ctx.h)
                rc, dev_out = raw_gram(pkg, m, dev, sites, SIDE[side])
                assert rc == 0, pkg.lib().sd_last_error(m.ctx.h)
                assert not np.isnan(host_out).any()                      # every entry written
                check_blocks(f"{name} {sname} side {side} {'c128' if cplx else 'f64'}", split(host_out, blocks), ref, cplx)
                assert np.array_equal(host_out, dev_out), (name, sname, side, "host and device forms differ")
                rc, again = raw_gram(pkg, m, dev, sites, SIDE[side])
                assert rc == 0 and np.array_equal(dev_out, again), (name, sname, side, "the same call twice")
                G = pkg.subsystem_gram(dev, m, sites, side)              # the Python mirror returns the same blocks
                for b in blocks:
                    assert np.array_equal(G[b.m], split(dev_out, blocks)[b.m])


@pytest.mark.parametrize("name", list(SHAPES))
def test_prefix_and_suffix_against_the_cut_kernel(pkg, name):
    import torch
    L, nup, _, _ = SHAPES[name]
    m = model_of(pkg, name)
    for cplx in (True, False):
        psi = state_of(L, nup, cplx)
        dev = torch.from_numpy(np.array(psi)).to(torch.device("cuda", m.ctx.device))
        for k in (1, 4, L // 2, L - 3):
            # sites = 1..k in order: the identity, no copy, the cut's bits
            for side in ("A", "B", "auto"):
                a, b = pkg.subsystem_gram(dev, m, list(range(1, k + 1)), side), pkg.cut_gram(dev, m, k, side)
                assert sorted(a) == sorted(b) and all(np.array_equal(a[mm], b[mm]) for mm in a), (name, k, side)
                a = pkg.subsystem_gram(psi, m, list(range(1, k + 1)), side)
                assert all(np.array_equal(a[mm], b[mm]) for mm in a), (name, k, side, "host form")
            # sites = k+1..L: rho of the suffix, which the cut kernel gives as side B
            sub, cut = pkg.subsystem_gram(dev, m, list(range(k + 1, L + 1)), "A"), pkg.cut_gram(dev, m, k, "B")
            ref = ref_of(L, nup, list(range(k + 1, L + 1)), "A", cplx)
            worst = 0.0
            for ms, G in sub.items():
                mc = -1 if nup is None else nup - ms
                G_ref, K = ref[ms]
                bound = ER.entry_bound(G_ref, K)
                assert G.shape == cut[mc].shape
                with np.errstate(divide="ignore", invalid="ignore"):
                    r = np.where(bound > 0, np.abs(G - cut[mc]) / bound, np.where(np.abs(G - cut[mc]) > 0, np.inf, 0.0))
                worst = max(worst, float(r.max()))
            print(f"{name} sites {k + 1}..{L} {'c128' if cplx else 'f64'}: largest |G_sub - G_cutB| / bound = {worst:.3e} (bar 1)")
            assert worst <= 1.0, (name, k, worst)


def eta(t):
    return -t * math.log(t) if t > 0.0 else 0.0


def entropy_bar(ref_blocks):
    """(sum over the eigenvalues of eta(eps), {m: eps}) of the blocks {m: (G_ref, K)}"""
    tr = sum(float(np.trace(g).real) for g, _ in ref_blocks.values())
    bar, eps = 0.0, {}
    for mm, (G_ref, K) in ref_blocks.items():
        d = G_ref.shape[0]
        eps[mm] = d * float(ER.entry_bound(G_ref, K).max()) / tr
        assert eps[mm] < 1 / math.e
        bar += d * eta(eps[mm])
    return bar, eps


def ref_spectrum(ref_blocks, cplx):
    tr = sum(float(np.trace(g).real) for g, _ in ref_blocks.values())
    return {mm: np.clip(np.linalg.eigvalsh(np.asarray(g, dtype=np.complex128 if cplx else np.float64))[::-1] / tr, 0.0, None)
            for mm, (g, _) in ref_blocks.items()}


@pytest.mark.parametrize("name", list(SHAPES))
def test_spectra_entropies_and_complements(pkg, name):
    L, nup, _, _ = SHAPES[name]
    m = model_of(pkg, name)
    for cplx in (True, False):
        psi = state_of(L, nup, cplx)
        for sname, sites in site_sets(L).items():
            rest = [s for s in range(1, L + 1) if s not in sites]
            ref = ref_of(L, nup, sites, "auto", cplx)
            s_bar, eps = entropy_bar(ref)
            want = ref_spectrum(ref, cplx)
            got = pkg.subsystem_spectrum(psi, m, sites)
            assert sorted(got) == sorted(want)
            worst = 0.0
            for mm in want:
                assert got[mm].shape == want[mm].shape and (np.diff(got[mm]) <= 0).all() and (got[mm] >= 0).all()
                err = float(np.abs(got[mm] - want[mm]).max())
                worst = max(worst, err / eps[mm] if eps[mm] > 0 else (0.0 if err == 0 else math.inf))
            S, S_ref = pkg.subsystem_entropy(psi, m, sites), ER.entropy(want, 1)
            S_rest = pkg.subsystem_entropy(psi, m, rest)
            r_bar, _ = entropy_bar(ref_of(L, nup, rest, "auto", cplx))
            WORST["eig"] = max(WORST["eig"], worst)
            WORST["S"] = max(WORST["S"], abs(S - S_ref) / s_bar)
            print(f"{name} {sname} {'c128' if cplx else 'f64'}: largest |lambda - lambda_ref| / eps = {worst:.3e} (bar 1); |S - S_ref| = "
                  f"{abs(S - S_ref):.3e} (bar {s_bar:.3e}); |S(S) - S(rest)| = {abs(S - S_rest):.3e} (bar {s_bar + r_bar:.3e})")
            assert worst <= 1.0, (name, sname, worst)
            assert abs(S - S_ref) <= s_bar, (name, sname, S, S_ref, s_bar)
            assert abs(S - S_rest) <= s_bar + r_bar, (name, sname, S, S_rest)
            many = pkg.subsystem_entropy(psi, m, sites, q=[1, 2, math.inf])
            assert many[0] == S and many[0] >= many[1] >= many[2] >= 0.0
    print(f"largest ratios so far: {WORST}")


PAIRS = [([1], [2]), ([1], ["L"]), ([3], [8]), ([2, 3], [4, 5]), ([1, 2], [7, 8]), ([4, 2], ["L", 9]), ([1, 3, 5], [2, 4, 6])]


@pytest.mark.parametrize("name", ["L12n6-tiled", "L13n5-rows", "full-L10"])
def test_mutual_information_and_negativity_against_the_restatement(pkg, name):
    L, nup, _, _ = SHAPES[name]
    m = model_of(pkg, name)
    for cplx in (True, False):
        psi = state_of(L, nup, cplx)
        for A, B in PAIRS:
            A, B = [L if x == "L" else x for x in A], [L if x == "L" else x for x in B]
            bars = [entropy_bar(ref_of(L, nup, S, "auto", cplx))[0] for S in (A, B, A + B)]
            I, I_ref = pkg.mutual_information(psi, m, A, B), SR.mutual_information(psi, L, nup, A, B)
            # the negativity: Delta of rho_{A u B} (side A, dense) bounded entrywise by the Gram bound / tr
            refAB = ref_of(L, nup, A + B, "A", cplx)
            tr = sum(float(np.trace(g).real) for g, _ in refAB.values())
            fro = math.sqrt(sum(float((ER.entry_bound(g, K) ** 2).sum()) for g, K in refAB.values())) / tr
            en_bar = math.sqrt(2.0 ** (len(A) + len(B))) * fro
            EN, EN_ref = pkg.logarithmic_negativity(psi, m, A, B), SR.log_negativity(psi, L, nup, A, B)
            WORST["I"] = max(WORST["I"], abs(I - I_ref) / sum(bars))
            WORST["EN"] = max(WORST["EN"], abs(EN - EN_ref) / en_bar)
            print(f"{name} A={A} B={B} {'c128' if cplx else 'f64'}: I = {I:.12f}, |I - I_ref| = {abs(I - I_ref):.3e} (bar {sum(bars):.3e}); "
                  f"E_N = {EN:.12f}, |E_N - E_N_ref| = {abs(EN - EN_ref):.3e} (bar {en_bar:.3e})")
            assert abs(I - I_ref) <= sum(bars), (name, A, B, I, I_ref)
            assert abs(EN - EN_ref) <= en_bar, (name, A, B, EN, EN_ref)
            assert I >= -sum(bars) and EN >= -en_bar
    print(f"largest ratios so far: {WORST}")


def test_known_answers_and_the_dense_matrix(pkg):
    """singlets on (1, L) and (2, 3), the rest polarised: I({1}:{L}) = 2 ln 2, E_N({1},{L}) = ln 2, I({1}:{2}) = 0, and the two-site
    matrix of the singlet; the dense matrix of a random state against the restatement's, entry by entry"""
    L, nup = 12, 6
    m = model_of(pkg, "L12n6-tiled")
    psi = SR.singlet_product_state(L, nup, [(1, L), (2, 3)])
    tol = 64 * 2.0 ** -53                      # a handful of amplitudes 1/2, sums of at most 4 products, one log
    assert abs(pkg.mutual_information(psi, m, [1], [L]) - 2 * math.log(2)) <= tol
    assert abs(pkg.logarithmic_negativity(psi, m, [1], [L]) - math.log(2)) <= tol
    assert abs(pkg.mutual_information(psi, m, [1], [2])) <= tol
    assert abs(pkg.logarithmic_negativity(psi, m, [1], [2])) <= tol
    want = np.zeros((4, 4))
    want[1, 1] = want[2, 2] = 0.5
    want[1, 2] = want[2, 1] = -0.5
    assert np.abs(pkg.two_site_density_matrix(psi, m, 1, L) - want).max() <= tol
    assert np.abs(pkg.two_site_density_matrix(psi, m, L, 1) - want).max() <= tol
    for cplx in (True, False):
        x = state_of(L, nup, cplx)
        for sites in ([5, 6, 7, 8], [L, 2, 7], [9, 4]):
            R = pkg.dense_density_matrix(pkg.subsystem_density_matrix(x, m, sites), len(sites))
            R_ref = np.asarray(SR.rho(x, L, nup, sites), dtype=np.complex128)
            assert R.shape == R_ref.shape and abs(np.trace(R).real - 1.0) <= 1e-14
            ref = ref_of(L, nup, sites, "A", cplx)
            bound = max(float(ER.entry_bound(g, K).max()) for g, K in ref.values())
            assert np.abs(R - R_ref / np.trace(R_ref).real).max() <= 2 * bound          # the entry and the trace it is divided by
            PT = pkg.partial_transpose(R, 1, len(sites) - 1)
            assert np.array_equal(PT, SR.partial_transpose(R, 1, len(sites) - 1))
    mf = model_of(pkg, "full-L10")
    x = state_of(10, None, True)
    R = pkg.dense_density_matrix(pkg.subsystem_density_matrix(x, mf, [10, 1, 4]), 3)
    assert np.abs(R - np.asarray(SR.rho(x, 10, None, [10, 1, 4]), dtype=np.complex128)).max() <= 1e-14


def test_statuses(pkg):
    import torch
    E = pkg._lib
    L, nup = 12, 6
    m = model_of(pkg, "L12n6-tiled")
    host = np.array(state_of(L, nup, True))
    dev = torch.from_numpy(host).to(torch.device("cuda", m.ctx.device))
    sharded = pkg.XXZChain(L, nup=nup)
    sharded.set_shard(0, 2)
    bare = pkg.XXZChain(L, nup=nup, ctx=None)
    good = [5, 6, 7, 8]
    n_el = sum(b.d * b.d for b in pkg.cut_blocks(m, 4))
    for x in (host, dev):
        assert raw_gram(pkg, m, x, good, 2)[0] == 0
        for bad in ([5, 5, 6, 7], [0, 6, 7, 8], [5, 6, 7, L + 1], [-1, 2, 3, 4]):
            assert raw_gram(pkg, m, x, bad, 2)[0] == E.SD_EARG
        assert raw_gram(pkg, m, x, good, 2, n_sites=0, n_el=n_el)[0] == E.SD_EARG
        assert raw_gram(pkg, m, x, list(range(1, L + 1)), 2, n_el=n_el)[0] == E.SD_EARG          # n_sites = L
        assert raw_gram(pkg, m, x, None, 2, n_sites=4)[0] == E.SD_EARG
        for side in (-1, 3):
            assert raw_gram(pkg, m, x, good, side, n_el=n_el)[0] == E.SD_EARG
        for dt in (0, 3):
            assert raw_gram(pkg, m, x, good, 2, dtype=dt)[0] == E.SD_EARG
        assert raw_gram(pkg, m, x, good, 2, n=m.N - 1)[0] == E.SD_EDIM
        assert raw_gram(pkg, m, x, good, 2, n=m.N + 1)[0] == E.SD_EDIM
        assert raw_gram(pkg, m, x, good, 2, null_out=True)[0] == E.SD_EARG
        assert raw_gram(pkg, m, x, good, 2, ctx=None)[0] == E.SD_EARG
        assert raw_gram(pkg, sharded, x, good, 2, n_el=n_el)[0] == E.SD_EARG
        assert raw_gram(pkg, bare, x, good, 2, ctx=m.ctx.h)[0] == E.SD_EARG
        assert raw_gram(pkg, m, x, good, 2)[0] == 0                          # the context is still usable
    # a block above SD_CUT_MAX_DIM: 16 sites of the full basis at L = 20 on side A have d = 2^16 (refused before psi is read)
    big = pkg.XXZChain(20, nup=None)
    s16 = np.ascontiguousarray(range(3, 19), dtype=np.intc)
    out = np.empty(4, dtype=np.complex128)
    assert pkg.lib().sd_subsystem_gram(big.ctx.h, big.h, 2, host.ctypes.data, big.N, s16.ctypes.data_as(_ip), 16, 0, out.ctypes.data) == E.SD_EARG
    # the Python layer
    for bad in ([], [1, 1], [0], [L + 1], list(range(1, L + 1)), [1.5], "ab"):
        with pytest.raises(pkg.ArgumentError):
            pkg.subsystem_entropy(host, m, bad)
    with pytest.raises(pkg.ArgumentError):
        pkg.subsystem_gram(host, m, good, side="left")
    with pytest.raises(pkg.ArgumentError):
        pkg.mutual_information(host, m, [1, 2], [2, 3])                      # not disjoint
    with pytest.raises(pkg.ArgumentError):
        pkg.logarithmic_negativity(host, m, [1, 2], [2, 3])
    big13 = model_of(pkg, "L13n5-tiled")
    with pytest.raises(pkg.ArgumentError):
        pkg.logarithmic_negativity(np.array(state_of(13, 5, True)), big13, list(range(1, 8)), list(range(8, 14)))   # 13 sites
    with pytest.raises(pkg.ArgumentError):
        pkg.dense_density_matrix({0: np.eye(1)}, 13)
    with pytest.raises(pkg.ArgumentError):
        pkg.subsystem_entropy(host, m, good, q=0)
    with pytest.raises(pkg.DimensionMismatch):
        pkg.subsystem_gram(host[:-1], m, good)
    with pytest.raises(pkg.ArgumentError):
        pkg.subsystem_entropy(np.zeros(m.N), m, good)                        # zero norm
    # mutual information of two lists that cover the system: S(A u B) = 0 for a pure state
    A, B = [1, 3, 5, 7, 9, 11], [2, 4, 6, 8, 10, 12]
    assert abs(pkg.mutual_information(host, m, A, B) - 2 * pkg.subsystem_entropy(host, m, A)) <= 1e-12
