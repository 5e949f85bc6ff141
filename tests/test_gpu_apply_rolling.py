"""The ROLLING far-bond ring of the packed ComplexF64 launch (k_apply_tiled, PACK; SD_PACK_RING = D register sets, D in 2..4).  The
first D entries of a tile's far-bond list go out in the prologue, before the barrier; a list of nf >= D entries then runs
rem = (nf - D) mod D head steps, (nf - D) div D loop iterations of D steps (a step: wait for the oldest set, accumulate it, issue the
next entry into it) and a drain of the D sets; a list of nf < D entries is closed by EMPTY bonds in the prologue.  Order and
arithmetic are those of the class launches, so plain applies are compared BIT-EXACT (np.array_equal) with the CPU oracle.
SD_LEN_CLASSES=2 makes the small plans take the packed launch, as in test_gpu_apply_pipelined.py.

What can go wrong is the prologue's phase, the head steps and the drain for each (list length, D), so the shapes are chosen by the
list lengths they hold (test_list_lengths_cover_every_path, on the host):
  L=20 nup=10, 12 suffix bits (p = 8): every length 1..8
  L=20 nup=8                         : the one-row tile P = 0xFF (suffix filling 0).  Its prefix bonds cannot flip but its straddling
                                       bond can (site 8 up, site 9 down), so its list has ONE entry, not none: no tile of a sector
                                       with 0 < nup < L has an empty list.  Length 0 -- the prologue of EMPTY bonds only -- is what the
                                       idle slots of L=20 nup=7 and the chain without hops run.
  L=18 nup=9, 10 and 11 suffix bits  : one- and two-slot teams
  L=20 nup=7                         : idle slots
Lengths 0..8 give every remainder of nf - D and every nf < D for D = 2, 3, 4, whatever D the library was built with.
Couplings: Jxy = Jz = 1 (hop amplitude 0.5: the fused multiply-add form), Jxy = 0.9, Jz = 0.7 (the unfused form), and Jxy = 0, where
the diagonal must come out untouched.

Limit of this file, as of its predecessors: nothing here can tell WHICH launch ran; a kernel trace (`profiles/run_profile.sh`) is
what shows one launch per apply."""
import numpy as np
import pytest

SHAPES = [
    # (L, nup, SD_SUFFIX_BITS or None)
    (20, 10, None),
    (20, 8, None),
    (18, 9, "10"),
    (18, 9, "11"),
    (20, 7, None),
]
COUPLINGS = [(1.0, 1.0), (0.9, 0.7)]

_cache = {}


def cvec(n, seed):
    rng = np.random.default_rng(seed)
    return rng.standard_normal(n) + 1j * rng.standard_normal(n)


def packed_env(monkeypatch, bits):
    monkeypatch.setenv("SD_LEN_CLASSES", "2")
    if bits is None:
        monkeypatch.delenv("SD_SUFFIX_BITS", raising=False)
    else:
        monkeypatch.setenv("SD_SUFFIX_BITS", bits)


def reference(O, L, nup, Jxy, Jz):
    """(oracle model, psi, H psi by the oracle): computed once per shape and shared, never modified"""
    key = (L, nup, Jxy, Jz)
    if key not in _cache:
        r = O.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)
        psi = cvec(r.N, 3000 + 10 * L + nup)
        want = O.apply_H(r, psi)
        psi.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (r, psi, want)
    return _cache[key]


def list_lengths(L, nup, LS):
    """{prefix P: length of its far-bond list}, by the rule the plan resolves the lists with: a prefix bond (b, b+1) flips where
    the two prefix bits differ; the straddling bond (p, p+1) flips where the partner prefix has a feasible suffix filling and this
    tile has rows whose first suffix site differs from prefix bit p."""
    from math import comb
    p = L - LS
    out = {}
    for P in range(1 << p):
        t = nup - bin(P).count("1")
        if not 0 <= t <= LS:
            continue                                  # no such tile
        n = bin((P ^ (P >> 1)) & ((1 << (p - 1)) - 1)).count("1")
        bitp = (P >> (p - 1)) & 1
        tq = t + 1 if bitp else t - 1                 # the partner prefix has bit p flipped
        nU = comb(LS - 1, t - 1) if t >= 1 else 0     # rows whose first suffix site is up
        mine = comb(LS, t) - nU if bitp else nU
        if 0 <= tq <= LS and mine > 0:
            n += 1
        out[P] = n
    return out


def test_list_lengths_cover_every_path():
    """Host only.  For every ring depth D = 2, 3, 4 the two L=20 shapes hold lists of every length 1..8, i.e. every remainder of
    nf - D for nf >= D and every 0 < nf < D; the tile P = 0xFF of nup=8 is the one-row tile with a one-entry list."""
    a, b = list_lengths(20, 10, 12), list_lengths(20, 8, 12)
    assert set(a.values()) == set(range(1, 9))
    assert b[0xFF] == 1                               # suffix filling 8 - 8 = 0: one row (nup=10: filling 2 at least, 66 rows)
    lengths = set(a.values()) | set(b.values())
    assert min(lengths) == 1                          # an empty list: idle slots and the chain without hops only
    lengths.add(0)
    for D in (2, 3, 4):
        assert {nf for nf in lengths if nf < D} == set(range(D))
        assert {(nf - D) % D for nf in lengths if nf >= D} == set(range(D))
        assert {(nf - D) // D for nf in lengths if nf >= D} >= {0, 1}    # the loop skipped and run


@pytest.mark.gpu
@pytest.mark.parametrize("Jxy,Jz", COUPLINGS)
@pytest.mark.parametrize("L,nup,bits", SHAPES)
def test_rolling_apply_bit_exact_vs_oracle(pkg, O, monkeypatch, L, nup, bits, Jxy, Jz):
    packed_env(monkeypatch, bits)
    m = pkg.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)
    assert m.device_path == "tiled"
    r, psi, want = reference(O, L, nup, Jxy, Jz)
    assert m.N == r.N
    out = np.empty_like(psi)
    pkg.apply_H(out, psi, m)
    assert np.array_equal(out, want), f"max diff {np.abs(out - want).max()}"


@pytest.mark.gpu
def test_rolling_chain_without_hops_leaves_the_diagonal(pkg, O, monkeypatch):
    """Jxy = 0: H is diagonal.  Every ring entry is an EMPTY bond or carries J = 0; the result is the oracle's diagonal product."""
    packed_env(monkeypatch, None)
    L, nup = 20, 7
    m = pkg.XXZChain(L, Jxy=0.0, Jz=0.7, nup=nup)
    r, psi, want = reference(O, L, nup, 0.0, 0.7)
    out = np.empty_like(psi)
    pkg.apply_H(out, psi, m)
    assert np.array_equal(out, want), f"max diff {np.abs(out - want).max()}"


@pytest.mark.gpu
def test_rolling_apply_rescaled_bit_exact(pkg, O, monkeypatch):
    packed_env(monkeypatch, None)
    L, nup, Jxy, Jz = 20, 10, 0.9, 0.7
    m = pkg.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)
    r, psi, _ = reference(O, L, nup, Jxy, Jz)
    out = np.empty_like(psi)
    pkg.apply_rescaled_H(out, psi, pkg.apply_H, m, 4.3, -0.7)
    assert np.array_equal(out, O.apply_rescaled_H(r, psi, 4.3, -0.7))


@pytest.mark.gpu
def test_rolling_lanczos_tridiag_vs_oracle(pkg, O, monkeypatch):
    """Four Lanczos steps (the dot epilogue's per-team partial sums) at the packed tests' bar of 1e-9."""
    packed_env(monkeypatch, None)
    L, nup, Jxy, Jz = 20, 8, 0.9, 0.7
    m = pkg.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)
    r, psi, _ = reference(O, L, nup, Jxy, Jz)
    al, be, _ = pkg.lanczos_tridiag(pkg.apply_H, m, psi, lanc_m=4)
    al2, be2, _ = O.lanczos_tridiag(r, psi, lanc_m=4)
    assert np.abs(al - al2).max() <= 1e-9 and np.abs(be - be2).max() <= 1e-9


@pytest.mark.gpu
def test_rolling_batched_launch_equals_single_launches(pkg, O, monkeypatch):
    """Three vectors in one batched launch (grid.y = 3) equal, to the bit, three recursions of single launches: the early table
    request and the registers reused after the ring see another vector's rows, never another vector's offsets."""
    packed_env(monkeypatch, None)
    L, nup = 20, 10
    m = pkg.XXZChain(L, nup=nup)
    _, psi, _ = reference(O, L, nup, 1.0, 1.0)
    q = pkg.momenta(m)[1:4]
    assert len(q) == 3
    omega = np.arange(0.0, 4.0, 0.1)
    try:
        m.ctx.set_q_batch(True)
        n0 = m.ctx.apply_count()
        S_batch = pkg.lanczos_sqw(psi, m, q, omega, lanc_m=6, eta=0.05)
        n_batch = m.ctx.apply_count() - n0
        m.ctx.set_q_batch(False)
        n0 = m.ctx.apply_count()
        S_serial = pkg.lanczos_sqw(psi, m, q, omega, lanc_m=6, eta=0.05)
        assert n_batch == m.ctx.apply_count() - n0
        assert np.isfinite(S_batch).all()
        assert np.array_equal(S_batch, S_serial)
    finally:
        m.ctx.set_q_batch(True)
