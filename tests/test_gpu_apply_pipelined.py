"""The far-bond ring of the packed ComplexF64 launch (k_apply_tiled, PACK): the loads of D consecutive entries of a tile's far-bond
list are issued unconditionally in one loop iteration and accumulated in list order; the list is closed to a multiple of D by
EMPTY bonds (zero records, J = 0).  Order and arithmetic are those of the class launches, so plain applies are compared BIT-EXACT
(np.array_equal) with the CPU oracle.  SD_LEN_CLASSES=2 makes the small plans take the packed launch, as in
test_gpu_apply_packed.py.

What can go wrong is the closing of the list, so the shapes are chosen by the list lengths they hold:
  L=20 nup=10, 12 suffix bits (p = 8): the list of a tile is its unequal neighbours among the eight prefix bits plus the straddling
                                       bond -- every length 1..8 occurs (checked below), i.e. every remainder mod 2 and mod 3
  L=18 nup=9, 10 and 11 suffix bits  : p = 8 and 7 with one- and two-slot teams
  L=20 nup=7                         : queues that end in partly filled blocks: idle slots, whose ring holds EMPTY bonds only
each with Jxy = Jz = 1 (hop amplitude 0.5: the fused multiply-add form) and Jxy = 0.9, Jz = 0.7 (the unfused form); and a chain
with Jxy = 0, where the ring must leave the diagonal untouched whether the model carries no hops or hops of amplitude zero.

Limit of this file, as of test_gpu_apply_packed.py: nothing here can tell WHICH launch ran; a kernel trace
(`profiles/run_profile.sh`) is what shows one launch per apply."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [
    # (L, nup, SD_SUFFIX_BITS or None)
    (20, 10, None),
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
        psi = cvec(r.N, 2000 + 10 * L + nup)
        want = O.apply_H(r, psi)
        psi.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (r, psi, want)
    return _cache[key]


def test_list_lengths_cover_every_remainder():
    """L=20 nup=10 at 12 suffix bits: prefix P of p = 8 sites, suffix filling t = 10 - popcount(P) in 2..10, so the straddling bond
    flips in every tile and the list length is 1 + the unequal neighbours among the prefix bits."""
    p, LS, nup = 8, 12, 10
    lengths = set()
    for P in range(1 << p):
        t = nup - bin(P).count("1")
        assert 1 <= t <= LS - 1                      # both values of the first suffix site occur: the straddling bond flips
        lengths.add(1 + bin((P ^ (P >> 1)) & ((1 << (p - 1)) - 1)).count("1"))
    assert lengths == set(range(1, 9))


@pytest.mark.parametrize("Jxy,Jz", COUPLINGS)
@pytest.mark.parametrize("L,nup,bits", SHAPES)
def test_ring_apply_bit_exact_vs_oracle(pkg, O, monkeypatch, L, nup, bits, Jxy, Jz):
    packed_env(monkeypatch, bits)
    m = pkg.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)
    assert m.device_path == "tiled"
    r, psi, want = reference(O, L, nup, Jxy, Jz)
    assert m.N == r.N
    out = np.empty_like(psi)
    pkg.apply_H(out, psi, m)
    assert np.array_equal(out, want), f"max diff {np.abs(out - want).max()}"


@pytest.mark.parametrize("L,nup,bits", [(20, 10, None), (20, 7, None)])
def test_ring_chain_without_hops_leaves_the_diagonal(pkg, O, monkeypatch, L, nup, bits):
    """Jxy = 0: H is diagonal.  Every ring entry is an EMPTY bond or carries J = 0; the result is the oracle's diagonal product."""
    packed_env(monkeypatch, bits)
    m = pkg.XXZChain(L, Jxy=0.0, Jz=0.7, nup=nup)
    r, psi, want = reference(O, L, nup, 0.0, 0.7)
    out = np.empty_like(psi)
    pkg.apply_H(out, psi, m)
    assert np.array_equal(out, want), f"max diff {np.abs(out - want).max()}"


@pytest.mark.parametrize("Jxy,Jz", COUPLINGS)
def test_ring_apply_rescaled_bit_exact(pkg, O, monkeypatch, Jxy, Jz):
    packed_env(monkeypatch, None)
    L, nup = 20, 10
    m = pkg.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)
    r, psi, _ = reference(O, L, nup, Jxy, Jz)
    out = np.empty_like(psi)
    pkg.apply_rescaled_H(out, psi, pkg.apply_H, m, 4.3, -0.7)
    assert np.array_equal(out, O.apply_rescaled_H(r, psi, 4.3, -0.7))


def test_ring_lanczos_tridiag_vs_oracle(pkg, O, monkeypatch):
    """Four Lanczos steps (the dot epilogue's per-team partial sums) at the packed tests' bar of 1e-9."""
    packed_env(monkeypatch, None)
    L, nup, Jxy, Jz = 20, 10, 0.9, 0.7
    m = pkg.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)
    r, psi, _ = reference(O, L, nup, Jxy, Jz)
    al, be, _ = pkg.lanczos_tridiag(pkg.apply_H, m, psi, lanc_m=4)
    al2, be2, _ = O.lanczos_tridiag(r, psi, lanc_m=4)
    assert np.abs(al - al2).max() <= 1e-9 and np.abs(be - be2).max() <= 1e-9
