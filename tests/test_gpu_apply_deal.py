"""The packed ComplexF64 launch with its orbits dealt to the XCD queues by the committed cost (csrc/xcd_deal.hpp,
SD_ORBIT_DEAL_COST in basis.cpp).  The dealing decides which queue an orbit joins, hence which tiles share a workgroup and where
the queues' idle slots fall; it is a bijection of the tile list and changes no arithmetic, so plain applies are compared
BIT-EXACT (np.array_equal) with the CPU oracle.  The planner's self-check of the block table runs inside every construction.
SD_LEN_CLASSES=2 makes small plans take the packed launch (tests/test_gpu_apply_packed.py).

Shapes: the smallest at which the dealing can go wrong.
  L=20 nup=10, 12 suffix bits : p = 8, two quad-active blocks: a few large orbits over eight queues; 1-, 2- and 4-slot teams
  L=20 nup=7,  12 suffix bits : short queues, idle slots at the queue ends
  L=22 nup=11, 12 suffix bits : p = 10, two blocks and a leftover pair; queues of unequal length close ranks at the end
  L=18 nup=9,  11 suffix bits : p = 7, fewer orbits than would fill every queue evenly
Couplings (1, 1): hop amplitude 1/2, the fused multiply-add form; (0.9, 0.7): the unfused form.
One library is at hand, so the dot epilogue's per-tile partial sums are checked through <v|Hv> against the oracle at 1e-9, the bar
of tests/test_gpu_apply_packed.py.  The dealing itself (every cost, the bound, the rows loop) is covered on the host by
tests/test_xcd_deal_host.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [
    # (L, nup, SD_SUFFIX_BITS or None)
    (20, 10, None),
    (20, 7, None),
    (22, 11, None),
    (18, 9, "11"),
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


@pytest.mark.parametrize("Jxy,Jz", COUPLINGS)
@pytest.mark.parametrize("L,nup,bits", SHAPES)
def test_dealt_apply_bit_exact_vs_oracle(pkg, O, monkeypatch, L, nup, bits, Jxy, Jz):
    packed_env(monkeypatch, bits)
    m = pkg.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)          # deals the orbits, builds the block table and runs its self-check
    assert m.device_path == "tiled"
    r, psi, want = reference(O, L, nup, Jxy, Jz)
    assert m.N == r.N
    out = np.empty_like(psi)
    pkg.apply_H(out, psi, m)
    assert np.array_equal(out, want), f"max diff {np.abs(out - want).max()}"


@pytest.mark.parametrize("Jxy,Jz", COUPLINGS)
@pytest.mark.parametrize("L,nup,bits", SHAPES)
def test_dealt_dot_epilogue_vs_oracle(pkg, O, monkeypatch, L, nup, bits, Jxy, Jz):
    """<v|Hv> from the per-tile partial sums of the fused dot epilogue (filed under the tile's index, whatever block and queue the
    tile was dealt to): alpha_1 of the Lanczos recursion against the oracle's product, and four steps of coefficients, at 1e-9."""
    packed_env(monkeypatch, bits)
    m = pkg.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)
    r, psi, want = reference(O, L, nup, Jxy, Jz)
    al, be, _ = pkg.lanczos_tridiag(pkg.apply_H, m, psi, lanc_m=4)
    nrm = np.linalg.norm(psi)
    e1 = np.vdot(psi / nrm, want / nrm).real
    print(f"L={L} nup={nup} Jxy={Jxy}: alpha_1 - <v|Hv> = {al[0] - e1:.3e}")
    assert abs(al[0] - e1) <= 1e-9
    al2, be2, _ = O.lanczos_tridiag(r, psi, lanc_m=4)
    assert np.abs(al - al2).max() <= 1e-9 and np.abs(be - be2).max() <= 1e-9


def test_dealt_batched_launch_equals_single_launches(pkg, O, monkeypatch):
    """Three vectors in one batched launch (grid.y = 3: the momenta of lanczos_sqw share every apply) equal, to the bit, three
    recursions of single launches."""
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
