"""The packed ComplexF64 launch of k_apply_tiled: one launch for all tile lengths, a workgroup = four wave slots of 256 rows,
tiles packed into the slots through the plan's block table (1, 2 or 4 consecutive slots per tile).  SD_LEN_CLASSES=2 splits the
length classes of small plans too, which is what makes a small plan take the packed launch.  No arithmetic differs from the class
launches, so plain applies are compared BIT-EXACT (np.array_equal) with the CPU oracle; the planner's self-check of the block
table runs inside every model construction here (a failed check is an error of the constructor).

Shapes: the smallest at which the form can go wrong.
  L=20 nup=10, 12 suffix bits : 256 tiles of 66..924 rows -- 1-, 2- and 4-slot teams mixed in one launch, teams starting in slots 1-3
  L=20 nup=7,  12 suffix bits : unbalanced fillings -- many one-slot tiles beside a few long ones, queues ending in partly filled blocks
  L=18 nup=9,  10 suffix bits : every tile <= 252 rows -- four independent one-wave teams per block
  L=18 nup=9,  11 suffix bits : 462-row tiles -- two-slot teams next to one-slot teams
each with Jxy = Jz = 1 (hop amplitude 0.5: the fused multiply-add form) and Jxy = 0.9, Jz = 0.7 (the unfused form).

Limit of this file: nothing here can tell WHICH launch ran.  Every assertion also holds for the class launches, `device_path` is
"tiled" for both, and the library exports no launch count (the ABI is pinned).  That these plans take the packed launch rests on
the eligibility rule of sd_build_plan / sd_upload_model (unsharded, packed partner tables, chain bonds only, classes split -- which
SD_LEN_CLASSES=2 forces -- and ComplexF64); a kernel trace (`profiles/run_profile.sh`) is what shows one launch per apply."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPES = [
    # (L, nup, SD_SUFFIX_BITS or None)
    (20, 10, None),
    (20, 7, None),
    (18, 9, "10"),
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
        psi = cvec(r.N, 1000 + 10 * L + nup)
        want = O.apply_H(r, psi)
        psi.setflags(write=False)
        want.setflags(write=False)
        _cache[key] = (r, psi, want)
    return _cache[key]


@pytest.mark.parametrize("Jxy,Jz", COUPLINGS)
@pytest.mark.parametrize("L,nup,bits", SHAPES)
def test_packed_apply_bit_exact_vs_oracle(pkg, O, monkeypatch, L, nup, bits, Jxy, Jz):
    packed_env(monkeypatch, bits)
    m = pkg.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)          # builds the block table and runs its self-check
    assert m.device_path == "tiled"
    r, psi, want = reference(O, L, nup, Jxy, Jz)
    assert m.N == r.N
    out = np.empty_like(psi)
    pkg.apply_H(out, psi, m)
    assert np.array_equal(out, want), f"max diff {np.abs(out - want).max()}"
    # Float64 keeps the class launches on the same plan
    x = np.ascontiguousarray(psi.real)
    outr = np.empty_like(x)
    pkg.apply_H(outr, x, m)
    assert np.array_equal(outr, O.apply_H(r, x))


@pytest.mark.parametrize("Jxy,Jz", COUPLINGS)
def test_packed_apply_rescaled_bit_exact(pkg, O, monkeypatch, Jxy, Jz):
    packed_env(monkeypatch, None)
    L, nup = 20, 10
    m = pkg.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)
    r, psi, _ = reference(O, L, nup, Jxy, Jz)
    out = np.empty_like(psi)
    pkg.apply_rescaled_H(out, psi, pkg.apply_H, m, 4.3, -0.7)
    assert np.array_equal(out, O.apply_rescaled_H(r, psi, 4.3, -0.7))


@pytest.mark.parametrize("L,nup,bits", SHAPES)
def test_packed_sum_epilogue_vs_oracle(pkg, O, monkeypatch, L, nup, bits):
    """<psi|H psi> by the fused dot epilogue (per-team partial sums filed under the tile's index): the Lanczos coefficients,
    alpha_1 = <v1|H v1> first, at the recursion tests' bar of 1e-9."""
    packed_env(monkeypatch, bits)
    Jxy, Jz = 0.9, 0.7
    m = pkg.XXZChain(L, Jxy=Jxy, Jz=Jz, nup=nup)
    r, psi, want = reference(O, L, nup, Jxy, Jz)
    al, be, _ = pkg.lanczos_tridiag(pkg.apply_H, m, psi, lanc_m=4)
    al2, be2, _ = O.lanczos_tridiag(r, psi, lanc_m=4)
    assert np.abs(al - al2).max() <= 1e-9 and np.abs(be - be2).max() <= 1e-9
    v1 = psi / np.linalg.norm(psi)
    e1 = np.vdot(v1, want / np.linalg.norm(psi)).real
    assert abs(al[0] - e1) <= 1e-9


def test_packed_batched_launch_equals_single_launches(pkg, O, monkeypatch):
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
