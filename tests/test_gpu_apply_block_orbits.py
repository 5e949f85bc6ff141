"""The packed ComplexF64 launch under the block-orbit tile order (csrc/orbit_key.hpp): orbits built from four-site blocks of the
prefix reach about 150 tiles and change which tiles share a workgroup and in which order the eight queues hold them.  The order
is a bijection of the tile list and no arithmetic changes, so plain applies are compared BIT-EXACT (np.array_equal) with the CPU
oracle; the planner's self-check of the block table (every tile once, consecutive slots) runs inside every model construction.
SD_LEN_CLASSES=2 makes small plans take the packed launch (tests/test_gpu_apply_packed.py).

Shapes: the smallest at which the order can go wrong.
  L=20 nup=10, 12 suffix bits : p = 8, two four-site blocks, both quad-active at half filling; 1-, 2- and 4-slot teams
  L=20 nup=7,  12 suffix bits : blocks with no or four up spins fall back to pairs; idle slots at the queue ends
  L=22 nup=11, 12 suffix bits : p = 10, two blocks and a leftover pair
  L=18 nup=9,  11 suffix bits : p = 7, one block, a pair and a single site
The orbit rule itself (all prefixes, all capacities) is covered on the host by tests/test_orbit_key_host.py."""
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
        psi = cvec(r.N, 2000 + 10 * L + nup)
        want = O.apply_H(r, psi)
        psi.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (r, psi, want)
    return _cache[key]


@pytest.mark.parametrize("Jxy,Jz", COUPLINGS)
@pytest.mark.parametrize("L,nup,bits", SHAPES)
def test_block_orbit_apply_bit_exact_vs_oracle(pkg, O, monkeypatch, L, nup, bits, Jxy, Jz):
    packed_env(monkeypatch, bits)
    m = pkg.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)          # builds the block table and runs its self-check
    assert m.device_path == "tiled"
    r, psi, want = reference(O, L, nup, Jxy, Jz)
    assert m.N == r.N
    out = np.empty_like(psi)
    pkg.apply_H(out, psi, m)
    assert np.array_equal(out, want), f"max diff {np.abs(out - want).max()}"


def test_block_orbit_apply_rescaled_bit_exact(pkg, O, monkeypatch):
    packed_env(monkeypatch, None)
    L, nup, Jxy, Jz = 20, 10, 0.9, 0.7
    m = pkg.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)
    r, psi, _ = reference(O, L, nup, Jxy, Jz)
    out = np.empty_like(psi)
    pkg.apply_rescaled_H(out, psi, pkg.apply_H, m, 4.3, -0.7)
    assert np.array_equal(out, O.apply_rescaled_H(r, psi, 4.3, -0.7))


def test_block_orbit_batched_launch_equals_single_launches(pkg, O, monkeypatch):
    """Three vectors in one batched launch (grid.y = 3) equal, to the bit, three recursions of single launches."""
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


@pytest.mark.parametrize("L,nup,bits", SHAPES)
def test_block_orbit_lanczos_coefficients_vs_oracle(pkg, O, monkeypatch, L, nup, bits):
    """alpha, beta over four Lanczos steps within 1e-9: the fused dot epilogue files each team's partial sums under the tile's
    index in single_rec, which the order of the block table must not disturb."""
    packed_env(monkeypatch, bits)
    Jxy, Jz = 0.9, 0.7
    m = pkg.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)
    r, psi, _ = reference(O, L, nup, Jxy, Jz)
    al, be, _ = pkg.lanczos_tridiag(pkg.apply_H, m, psi, lanc_m=4)
    al2, be2, _ = O.lanczos_tridiag(r, psi, lanc_m=4)
    assert np.abs(al - al2).max() <= 1e-9 and np.abs(be - be2).max() <= 1e-9
