"""Entanglement across a chain cut: sd_cut_gram / sd_cut_gram_dev and the Python mirror (entanglement.py) against
tests/entanglement_ref.py, the extended-precision restatement proven on the CPU by tests/test_entanglement_ref_host.py.

Bars (derived, not tuned; u = 2^-53).
  Gram entries: |G - G_ref| <= 4 (K + 4) u sqrt(G_aa G_bb), K the block's summation length.  A K-term complex dot product in any
    summation order (four real products per term, each rounded once or fused) has the forward error gamma_{K+2} sum |x_k||y_k| <=
    gamma_{K+2} sqrt(G_aa G_bb) by Cauchy-Schwarz; 4 (K + 4) u covers gamma_{K+2} with the pieces' final additions and the restatement's
    own rounding (64-bit mantissa, 2^-11 of u per term).
  Structure: Hermitian to the bit with the diagonal's imaginary parts == 0.0; real symmetric to the bit for Float64; the same call
    twice gives np.array_equal results.
  Identities: sum_m tr G_m against the library's squared norm and tr G_m against the counting statistics of the same cut, 1e-12
    relative (the bar of section 20: sums of non-negative terms).
  Eigenvalues: |lambda - lambda_ref| <= eps = d (largest entry bound of the block) / tr, by Weyl with ||Delta||_2 <= ||Delta||_F <= d max.
  S_1: within sum over the eigenvalues of eta(eps), eta(t) = -t ln t, from |eta(x) - eta(y)| <= eta(|x - y|) for |x - y| <= 1/e.
Every shape first asserts, through sd_cut_blocks / sd_cut_plan_info, the edge it is there to cross."""
import ctypes as C
import math

import numpy as np
import pytest

import entanglement_ref as ER

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
KC, TARGET = 16, 2048          # SD_CUT_KC, SD_CUT_TARGET_ITEMS
SIDE = {"A": 0, "B": 1, "auto": 2}
WORST = {"ratio": 0.0}

# name -> (L, nup, cut, sides)
SHAPES = {
    "L16n8-cut8": (16, 8, 8, ("auto", "B")),
    "L16n8-cut12": (16, 8, 12, ("A", "B", "auto")),
    "L22n11-cut2": (22, 11, 2, ("auto",)),
    "L14n3-cut4": (14, 3, 4, ("auto",)),
    "L14n3-cut10": (14, 3, 10, ("auto",)),
    "full-L12-cut3": (12, None, 3, ("A", "B")),
    "full-L12-cut6": (12, None, 6, ("A", "B")),
    "full-L12-cut9": (12, None, 9, ("A", "B")),
    "L7n0-cut3": (7, 0, 3, ("A", "B", "auto")),
    "L7n7-cut3": (7, 7, 3, ("A", "B", "auto")),
    "L2n1-cut1": (2, 1, 1, ("A", "B", "auto")),
}

_models, _states, _refs = {}, {}, {}


def model_of(pkg, L, nup):
    if (L, nup) not in _models:
        _models[(L, nup)] = pkg.XXZChain(L, nup=nup)
    return _models[(L, nup)]


def state_of(L, nup, cplx):
    """a seeded random vector, normalised; the same array for every test that asks"""
    if (L, nup, cplx) not in _states:
        n = len(ER.basis(L, nup))
        rng = np.random.default_rng(20261020 + 1000 * L + 7 * (nup if nup is not None else 63) + cplx)
        psi = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)
        psi = np.ascontiguousarray(psi / np.linalg.norm(psi))
        psi.setflags(write=False)
        _states[(L, nup, cplx)] = psi
    return _states[(L, nup, cplx)]


def ref_of(L, nup, cut, side, cplx):
    key = (L, nup, cut, side, cplx)
    if key not in _refs:
        _refs[key] = ER.gram_blocks(state_of(L, nup, cplx), L, nup, cut, side)
    return _refs[key]


def raw_gram(pkg, m, psi, cut, side, n=None, dtype=None, n_el=None, null_out=False, ctx="model"):
    """status and the packed output of sd_cut_gram[_dev] called directly; psi a numpy array (host form) or a torch tensor (_dev)"""
    import torch
    dev = isinstance(psi, torch.Tensor)
    cplx = psi.is_complex() if dev else np.iscomplexobj(psi)
    if n_el is None:
        nb, ne = C.c_int(), C.c_int64()
        rc = pkg.lib().sd_cut_blocks(m.h, cut, side, None, 0, C.byref(nb), C.byref(ne))
        n_el = ne.value if rc == 0 else 1
    out = np.full(n_el, np.nan, dtype=np.complex128 if cplx else np.float64)
    code = (pkg._lib.SD_C128 if cplx else pkg._lib.SD_F64) if dtype is None else dtype
    if dev and m.ctx is not None:
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    ptr = None if psi is None else (psi.data_ptr() if dev else psi.ctypes.data)
    h = m.ctx.h if ctx == "model" else ctx
    fn = pkg.lib().sd_cut_gram_dev if dev else pkg.lib().sd_cut_gram
    rc = fn(h, m.h, code, ptr, len(psi) if n is None else n, cut, side, None if null_out else out.ctypes.data)
    return rc, out


def split(out, blocks):
    return {b.m: out[b.offset:b.offset + b.d * b.d].reshape(b.d, b.d) for b in blocks}


def assert_edges(pkg, name, m, cut, side):
    """the edge each shape is there to cross, by name"""
    blocks = pkg.cut_blocks(m, cut, side)
    n_items, max_ns, _ = pkg.cut_plan_info(m, cut, side)
    ds = [b.d for b in blocks]
    Ks = [b.dB if b.side == "A" else b.dA for b in blocks]
    full = m.nup is None
    forms = {("ACROSS" if (b.side == "B") == full else "INSIDE") for b in blocks}
    if name == "L16n8-cut8" and side == "auto":
        assert ds == [1, 8, 28, 56, 70, 56, 28, 8, 1]                  # both tile sizes; 70 = one full and one partial tile of 64
        assert 1 in Ks and any(1 < k < KC for k in Ks) and forms == {"ACROSS"}
    if name == "L16n8-cut12" and side == "A":                          # many tile pairs, K = 1, 4, 6 below the chunk, no split
        assert forms == {"ACROSS"} and set(ds) == {495, 792, 924} and set(Ks) == {1, 4, 6} and max_ns == 1 and n_items == 374
    if name == "L16n8-cut12" and side in ("B", "auto"):                # the INSIDE form, summed over 495 .. 924 segments
        assert {b.side for b in blocks} == {"B"} and forms == {"INSIDE"} and set(ds) == {1, 4, 6} and set(Ks) == {495, 792, 924}
        assert max_ns > 1
    if name == "L22n11-cut2":
        assert max(ds) <= 2 and max(Ks) == 184756 and max_ns > 1
        items = np.zeros(n_items, dtype=pkg.entanglement.CUT_ITEM)
        n = C.c_int64()
        assert pkg.lib().sd_cut_plan_items(m.h, cut, SIDE[side], items.ctypes.data, n_items, C.byref(n)) == 0
        last = items[items["piece"] == items["ns"] - 1]
        assert ((last["k1"] - last["k0"]) % KC != 0).any()             # a last piece that is not a multiple of the chunk
    if name.startswith("L14n3"):
        assert {b.side for b in blocks} == {"A", "B"}                  # the auto side differs between the blocks
    if name.startswith("full"):
        assert len(blocks) == 1 and blocks[0].m == -1 and forms == ({"INSIDE"} if side == "A" else {"ACROSS"})
    if name.startswith(("L7", "L2n1")):
        assert set(ds) == {1} and set(Ks) == {1}
    return blocks


def check_blocks(tag, got, ref, cplx):
    """every block against the restatement; prints the largest ratio to the bound before it asserts"""
    worst = 0.0
    for mm, (G_ref, K) in ref.items():
        G = got[mm]
        assert G.shape == G_ref.shape, (tag, mm)
        bound = ER.entry_bound(G_ref, K)
        err = np.abs(np.asarray(G - G_ref, dtype=np.clongdouble if cplx else np.longdouble)).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
        worst = max(worst, float(ratio.max()))
        if cplx:
            assert np.array_equal(G, G.conj().T), (tag, mm, "not Hermitian to the bit")
            assert (np.diag(G).imag == 0.0).all(), (tag, mm)
        else:
            assert G.dtype == np.float64 and np.array_equal(G, G.T), (tag, mm, "not symmetric to the bit")
    WORST["ratio"] = max(WORST["ratio"], worst)
    print(f"{tag}: largest |G - G_ref| / bound = {worst:.3e} (bar 1; largest so far {WORST['ratio']:.3e})")
    assert worst <= 1.0, (tag, worst)


@pytest.mark.parametrize("cplx", [True, False], ids=["c128", "f64"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_gram_against_the_restatement(pkg, name, cplx):
    import torch
    L, nup, cut, sides = SHAPES[name]
    m = model_of(pkg, L, nup)
    psi = state_of(L, nup, cplx)
    dev = torch.from_numpy(np.array(psi)).to(torch.device("cuda", m.ctx.device))
    for side in sides:
        blocks = assert_edges(pkg, name, m, cut, side)
        ref = ref_of(L, nup, cut, side, cplx)
        assert sorted(ref) == [b.m for b in blocks]
        rc, host_out = raw_gram(pkg, m, psi, cut, SIDE[side])
        assert rc == 0, pkg.lib().sd_last_error(m.ctx.h)
        rc, dev_out = raw_gram(pkg, m, dev, cut, SIDE[side])
        assert rc == 0, pkg.lib().sd_last_error(m.ctx.h)
        assert not np.isnan(host_out).any()                               # every entry written
        check_blocks(f"{name} side {side} {'c128' if cplx else 'f64'} host", split(host_out, blocks), ref, cplx)
        assert np.array_equal(host_out, dev_out), (name, side, "host and device forms differ")
        rc, again = raw_gram(pkg, m, dev, cut, SIDE[side])
        assert rc == 0 and np.array_equal(dev_out, again), (name, side, "the same call twice")
        # the Python mirror returns the same blocks
        G = pkg.cut_gram(dev, m, cut, side)
        for b in blocks:
            assert np.array_equal(G[b.m], split(dev_out, blocks)[b.m])


@pytest.mark.parametrize("name", ["L16n8-cut8", "L16n8-cut12", "L14n3-cut4", "L14n3-cut10", "full-L12-cut6", "L2n1-cut1"])
def test_identities_against_other_kernels(pkg, name):
    import torch
    L, nup, cut, sides = SHAPES[name]
    m = model_of(pkg, L, nup)
    for cplx in (True, False):
        psi = 1.7 * np.array(state_of(L, nup, cplx))                     # nothing is divided by <psi|psi>
        dev = torch.from_numpy(psi).to(torch.device("cuda", m.ctx.device))
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        n2 = C.c_double()
        pkg.check(pkg.lib().sd_nrm2sq_dev(m.ctx.h, 2 if cplx else 1, dev.data_ptr(), len(dev), C.byref(n2)), m.ctx.h)
        P = pkg.counting_statistics(dev, m, [range(1, cut + 1)], normalize=False)[0]
        Pn = pkg.cut_counting_statistics(dev, m)[cut - 1]
        for side in sides:
            G = pkg.cut_gram(dev, m, cut, side)
            tr = {mm: float(np.trace(g).real) for mm, g in G.items()}
            total = sum(tr.values())
            print(f"{name} side {side}: |sum tr G - |psi|^2| / |psi|^2 = {abs(total - n2.value) / n2.value:.2e} (bar 1e-12)")
            assert abs(total - n2.value) <= 1e-12 * n2.value
            if nup is not None:
                for mm, t in tr.items():
                    assert abs(t - P[mm]) <= 1e-12 * P[mm], (name, side, mm, t, P[mm])
                    assert abs(t / total - Pn[mm]) <= 1e-12 * Pn[mm], (name, side, mm)
                assert P.sum() == pytest.approx(sum(P[mm] for mm in tr), rel=1e-15)     # no weight outside the blocks
            rho = pkg.reduced_density_matrix(dev, m, cut, side=side if side != "auto" else "A")
            assert abs(sum(float(np.trace(r).real) for r in rho.values()) - 1.0) <= 1e-14


def eta(t):
    return -t * math.log(t) if t > 0.0 else 0.0


def check_spectrum(pkg, tag, psi, m, L, nup, cut):
    """entanglement_spectrum and the entropies of psi against the restatement, inside the derived bars"""
    cplx = np.iscomplexobj(psi)
    ref_blocks = ER.gram_blocks(psi, L, nup, cut, "auto")
    tr = sum(float(np.trace(g).real) for g, _ in ref_blocks.values())
    ref = ER.spectrum(psi, L, nup, cut)
    got = pkg.entanglement_spectrum(psi, m, cut)
    assert sorted(got) == sorted(ref)
    s_bar, worst = 0.0, 0.0
    for mm, (G_ref, K) in ref_blocks.items():
        d = G_ref.shape[0]
        eps = d * float(ER.entry_bound(G_ref, K).max()) / tr
        assert got[mm].shape == (d,) and (np.diff(got[mm]) <= 0).all() and (got[mm] >= 0).all()
        err = float(np.abs(got[mm] - ref[mm]).max())
        worst = max(worst, err / eps if eps > 0 else (0.0 if err == 0 else math.inf))
        assert eps < 1 / math.e
        s_bar += d * eta(eps)
    S, S_ref = pkg.entanglement_entropy(psi, m, cut), ER.entropy(ref, 1)
    print(f"{tag} cut {cut} {'c128' if cplx else 'f64'}: largest |lambda - lambda_ref| / eps = {worst:.3e} (bar 1); "
          f"|S - S_ref| = {abs(S - S_ref):.3e} (bar {s_bar:.3e})")
    assert worst <= 1.0, (tag, cut, worst)
    assert abs(S - S_ref) <= s_bar, (tag, cut, S, S_ref, s_bar)
    sr = pkg.symmetry_resolved_entanglement(psi, m, cut)
    # the same eigenvalues summed in another grouping: at most n terms, each rounded a few times
    n_eig = sum(len(v) for v in got.values())
    assert abs(sr["S_total"] - S) <= 8 * U * n_eig * max(1.0, S) and sr["S_total"] == sr["S_number"] + sr["S_config"]
    assert abs(sr["S_number"] - pkg.number_entropy(psi, m, range(1, cut + 1))) <= 1e-12 * max(1.0, sr["S_number"]) * (L + 1)
    return S


def test_spectra_and_entropies_end_to_end(pkg):
    L, nup = 12, 6
    m = pkg.XXZChain(L, Jxy=1.0, Jz=1.0, hz=0.0, nup=nup, boundary="open")
    E0, gs = pkg.groundstate(m)
    gs = np.asarray(gs.cpu() if hasattr(gs, "cpu") else gs)
    prof = []
    for cut in range(1, L):
        prof.append(check_spectrum(pkg, "groundstate L=12", gs, m, L, nup, cut))
        check_spectrum(pkg, "groundstate L=12", gs.astype(np.complex128) * np.exp(0.3j), m, L, nup, cut)
    assert np.allclose(pkg.entanglement_profile(gs, m), prof, rtol=0, atol=0)
    assert max(prof) > 0.3 and min(prof) > 0.0
    assert pkg.schmidt_gap(gs, m, L // 2) > 0.0
    many = pkg.entanglement_entropy(gs, m, 6, q=[1, 2, math.inf])
    assert many[0] >= many[1] >= many[2] > 0.0 and many[0] == prof[5]
    # the Neel state is a product state: S = 0 exactly at every cut and every q, one eigenvalue 1
    neel = np.asarray(pkg.neel_state(m)).astype(np.complex128)
    for cut in range(1, L):
        for q in (1, 2, math.inf):
            assert pkg.entanglement_entropy(neel, m, cut, q) == 0.0
        sp = np.concatenate(list(pkg.entanglement_spectrum(neel, m, cut).values()))
        assert sorted(sp)[-1] == 1.0 and np.count_nonzero(sp) == 1
        assert pkg.schmidt_gap(neel, m, cut) == 1.0
    # the singlet of two sites: ln 2, all of it number entropy
    m2 = pkg.XXZChain(2, nup=1)
    st = list(ER.basis(2, 1))
    s = np.zeros(2)
    s[st.index(1)], s[st.index(2)] = 1 / math.sqrt(2), -1 / math.sqrt(2)
    check_spectrum(pkg, "singlet", s, m2, 2, 1, 1)
    assert abs(pkg.entanglement_entropy(s, m2, 1) - math.log(2)) <= 16 * U
    sr = pkg.symmetry_resolved_entanglement(s, m2, 1)
    assert sr["S_config"] == 0.0 and abs(sr["S_number"] - math.log(2)) <= 16 * U


def test_statuses(pkg):
    import torch
    E = pkg._lib
    L, nup = 12, 6
    m = model_of(pkg, L, nup)
    host = np.array(state_of(L, nup, True))
    dev = torch.from_numpy(host).to(torch.device("cuda", m.ctx.device))
    sharded = pkg.XXZChain(L, nup=nup)
    sharded.set_shard(0, 2)
    no_tables = pkg.XXZChain(L, nup=nup, ctx=None)
    n_el = sum(b.d * b.d for b in pkg.cut_blocks(m, 6))
    for x in (host, dev):
        assert raw_gram(pkg, m, x, 6, 2)[0] == 0
        for cut in (0, L, -3):
            assert raw_gram(pkg, m, x, cut, 2)[0] == E.SD_EARG
        for side in (-1, 3):
            assert raw_gram(pkg, m, x, 6, side, n_el=n_el)[0] == E.SD_EARG
        for dt in (0, 3):
            assert raw_gram(pkg, m, x, 6, 2, dtype=dt)[0] == E.SD_EARG
        assert raw_gram(pkg, m, x, 6, 2, n=m.N - 1)[0] == E.SD_EDIM
        assert raw_gram(pkg, m, x, 6, 2, n=m.N + 1)[0] == E.SD_EDIM
        assert raw_gram(pkg, m, x, 6, 2, null_out=True)[0] == E.SD_EARG
        assert raw_gram(pkg, m, x, 6, 2, ctx=None)[0] == E.SD_EARG
        assert raw_gram(pkg, sharded, x, 6, 2, n_el=n_el)[0] == E.SD_EARG
        assert raw_gram(pkg, no_tables, x, 6, 2, ctx=m.ctx.h)[0] == E.SD_EARG
        assert raw_gram(pkg, m, x, 6, 2)[0] == 0                          # the context is still usable
    fn = pkg.lib().sd_cut_gram
    out = np.empty(n_el, dtype=np.complex128)
    assert fn(m.ctx.h, m.h, 2, None, m.N, 6, 2, out.ctypes.data) == E.SD_EARG
    assert fn(m.ctx.h, None, 2, host.ctypes.data, m.N, 6, 2, out.ctypes.data) == E.SD_EARG
    # a block above SD_CUT_MAX_DIM: side B of the full basis at L = 20, cut 4 has d = 2^16 (refused before psi is read)
    big = pkg.XXZChain(20, nup=None)
    assert fn(big.ctx.h, big.h, 2, host.ctypes.data, big.N, 4, 1, out.ctypes.data) == E.SD_EARG
    # the Python layer raises before any launch
    for bad in (0, L, 1.5):
        with pytest.raises(pkg.ArgumentError):
            pkg.entanglement_entropy(host, m, bad)
    with pytest.raises(pkg.ArgumentError):
        pkg.reduced_density_matrix(host, m, 6, side="left")
    with pytest.raises(pkg.ArgumentError):
        pkg.entanglement_entropy(host, m, 6, q=0)
    with pytest.raises(pkg.ArgumentError):
        pkg.entanglement_entropy(host, m, 6, q=[1, -2])
    with pytest.raises(pkg.DimensionMismatch):
        pkg.cut_gram(host[:-1], m, 6)
    with pytest.raises(pkg.ArgumentError):
        pkg.entanglement_entropy(np.zeros(m.N), m, 6)                     # zero norm
