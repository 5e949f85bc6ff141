"""S^-_q / S^+_q between adjacent sectors (csrc/kernels_transverse.hip) where the loops of its three kernels wrap, and where source
and target are planned differently: sd_spm_q_dev called directly, with an output the test owns and fills with NaN first.

Shapes (default plan: 12 suffix sites, no tile longer than C(12, 6) = 924 rows; the outer loop of k_spm_tiled steps by 1024):
  S13  L=16 nup=8, SD_SUFFIX_BITS=13: both targets 8 tiles of 715..1716 rows, 7 of them > 1024   (second trip, partial slots)
  S14  L=17, nup=9 for S^-, nup=8 for S^+, SD_SUFFIX_BITS=14: targets of 8 tiles of 2002..3432 rows    (2 to 4 trips)
  Ts8  L=14 nup=7, SD_SUFFIX_BITS=8: both targets 64 tiles of 1..70 rows        (waves 2, 3 and the slots k >= 1 always idle)
  X+   L=30 nup=6 (per-row, 593 775 rows) -> nup=7 (tiled, 63 004 tiles, 2 035 800 rows)     (per-row source, tiled target)
  X-   L=30 nup=7 (tiled) -> nup=6 (per-row)                                                 (tiled source, per-row target)
  F29  full basis L=29, 536 870 912 rows: exactly two passes of the 2^20 blocks of k_spm_full
  R48+ L=48 nup=7 (73 629 072 rows) -> nup=8 (377 348 994 rows > 2^28): k_spm_rows wraps
  R48- L=48 nup=9 (1 677 106 640 rows, Float64, 13.4 GB) -> nup=8: the same target through the S^- instantiation
Every test first asserts that its shape still has the property it is there for.

Vectors come from the library's counter-based normal stream and stay on the device.  The bars are those of check_phi in
tests/test_gpu_transverse.py: at q = 0 real and imaginary parts under ==, otherwise max |got - want| <= 2e-15 max |want|; a NaN
left in the output fails both.  References: tests/transverse_ref.py on the host (the small shapes, and sampled rows of the cap
cells with psi gathered from the device vector), `spm_rows_t` of tests/rows_ref.py on the device over all rows (X+-), proven
against each other by tests/test_rows_ref_host.py.

Wall times of the cap cells on an MI355X, the whole test each (allocations, fills, three kernel calls, references):
  F29 Float64 0.4 s, F29 ComplexF64 0.3 s, R48+ 0.9 s, R48- 2.0 s."""
import gc
import math
import time

import numpy as np
import pytest

import rows_ref as RR
import transverse_ref as R

pytestmark = pytest.mark.gpu

NAN = float("nan")
XXZ = dict(Jxy=0.8, Jz=0.7, hz=0.3, boundary="periodic")
OPS = {"minus": (2, -1), "plus": (1, 1)}              # name -> (SD_SPIN_MINUS / SD_SPIN_PLUS, target nup - source nup)
CAP = 1 << 28                                          # launch_spm: at most 2^20 blocks of 256 rows per pass


def build(pkg, L, nup, ls):
    """XXZChain(L, nup) planned with `ls` suffix sites (None: the default); the plan reads SD_SUFFIX_BITS when the model is built"""
    with pytest.MonkeyPatch.context() as mp:
        if ls is None:
            mp.delenv("SD_SUFFIX_BITS", raising=False)
        else:
            mp.setenv("SD_SUFFIX_BITS", str(ls))
        return pkg.XXZChain(L, nup=nup, **XXZ)


def device_of(m):
    import torch
    return torch.device("cuda", m.ctx.device)


def fill_randn(pkg, m, N, cplx, seed):
    import torch
    x = torch.empty(N, dtype=torch.complex128 if cplx else torch.float64, device=device_of(m))
    m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, x.data_ptr(), (2 if cplx else 1) * N, seed, 0), m.ctx.h)
    return x


def nan_complex(N, dev):
    import torch
    out = torch.empty(N, dtype=torch.complex128, device=dev)
    torch.view_as_real(out).fill_(NAN)
    return out


def spm_into(pkg, src, dst, op, psi, q, out):
    """out = S^-+_q psi through the C ABI: the caller owns the output; it is filled with NaN before every call"""
    import torch
    torch.view_as_real(out).fill_(NAN)
    src.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
    code = pkg._lib.SD_C128 if psi.is_complex() else pkg._lib.SD_F64
    pkg.check(pkg.lib().sd_spm_q_dev(src.ctx.h, src.h, dst.h, OPS[op][0], code, psi.data_ptr(), len(psi), float(q), out.data_ptr(),
                                     len(out)), src.ctx.h)
    torch.cuda.synchronize()
    return out


def check_phi(got, want, q, what):
    """the bars of check_phi in test_gpu_transverse.py on numpy vectors; the figure is printed before it is asserted"""
    assert got.shape == want.shape and got.dtype == np.complex128
    top = np.abs(want).max()
    if q == 0.0:
        bad = np.nonzero((got.real != want.real) | (got.imag != want.imag))[0]
        assert len(bad) == 0, (what, len(bad), bad[:8].tolist())
    else:
        err = np.abs(got - want).max()
        print(f"{what}: {err:.2e} (bar {2e-15 * top:.2e})")
        assert err <= 2e-15 * top, (what, err, top)         # (a NaN in `got` makes err a NaN: the comparison fails)
    return top


def tile_lengths(m):
    lb, gb, ln = m.local_tiles()
    assert np.array_equal(lb, gb)                          # one device holds the whole sector
    return ln


# ---- 1. the outer loop of k_spm_tiled: tiles past 1024 rows, and tiles shorter than a wave ----
SMALL = {
    "S13": dict(L=16, src={"minus": 8, "plus": 8}, ls=13),
    "S14": dict(L=17, src={"minus": 9, "plus": 8}, ls=14),
    "Ts8": dict(L=14, src={"minus": 7, "plus": 7}, ls=8),
}


@pytest.mark.parametrize("op", ["minus", "plus"])
@pytest.mark.parametrize("name", ["S13", "S14", "Ts8"])
def test_tiled_targets_of_other_suffix_lengths_match_numpy(pkg, name, op):
    import torch
    spec = SMALL[name]
    L, nup, ls = spec["L"], spec["src"][op], spec["ls"]
    src = build(pkg, L, nup, ls)
    dst = build(pkg, L, nup + OPS[op][1], ls)
    assert pkg.lib().sd_model_path(dst.h) == 1
    ln = tile_lengths(dst)
    if name == "Ts8":
        assert len(ln) == 64 and ln.max() <= 128 and ln.min() == 1 and (ln > 64).any()       # never a row in waves 2, 3 or a slot k >= 1
    else:
        assert len(ln) == 8 and ln.max() > 1024 and (ln > 1024).sum() >= 7                   # a second trip ...
        assert ((ln > 1024) & (ln % 1024 != 0)).any()          # ... whose last one leaves some of a thread's four rows without a row
        if name == "S14":
            assert 1024 < ln.min() <= 2048 and ln.max() > 3072                               # 2 to 4 trips
    out = nan_complex(dst.N, device_of(dst))
    top = 0.0
    for cplx in (False, True):
        psi = fill_randn(pkg, src, src.N, cplx, 1000 * L + nup + cplx)
        host = psi.cpu().numpy()
        for q in (0.0, 2 * np.pi * 3 / L, 0.3):
            got = spm_into(pkg, src, dst, op, psi, q, out).cpu().numpy()
            top = max(top, check_phi(got, R.spm(L, nup, host, q, op), q, f"{name} {op} cplx={cplx} q={q:.3f}"))
    again = spm_into(pkg, src, dst, op, psi, 0.3, out).cpu().numpy()                         # same call twice: equal bits
    assert np.array_equal(got.view(np.float64), again.view(np.float64))
    assert top > 0.1                                                                         # never zeros against zeros
    # the Python mirror builds its own target when it is called, under whatever plan the environment asks for then: the same bits
    mirror = pkg.Sminus_q_vector(src, psi, 0.3) if op == "minus" else pkg.Splus_q_vector(src, psi, 0.3)
    assert torch.equal(torch.view_as_real(mirror), torch.view_as_real(out))


# ---- 2. source and target on different paths ----
@pytest.mark.parametrize("nup,cross_op", [(6, "plus"), (7, "minus")])
def test_per_row_and_tiled_plans_mixed_match_the_row_loop_on_all_rows(pkg, nup, cross_op):
    """X+ (nup = 6, S^+: per-row source, tiled target) and X- (nup = 7, S^-: tiled source, per-row target); the other operator of
    each source (per-row to per-row, tiled to tiled) runs beside it."""
    import torch
    L = 30
    src = build(pkg, L, nup, None)
    path = pkg.lib().sd_model_path
    for op in ("minus", "plus"):
        dst = build(pkg, L, nup + OPS[op][1], None)
        if op == cross_op:
            assert (path(src.h), path(dst.h)) == ((0, 1) if cross_op == "plus" else (1, 0))
            assert (src.N, dst.N) == ((593775, 2035800) if cross_op == "plus" else (2035800, 593775))
            tiled = dst if cross_op == "plus" else src
            ln = tile_lengths(tiled)
            assert len(ln) == 63004 and ln.min() == 1 and ln.max() == 924
        dev = device_of(dst)
        s_dst = RR.configurations_t(torch.arange(dst.N, dtype=torch.int64, device=dev), L, dst.nup)
        out = nan_complex(dst.N, dev)
        top = 0.0
        for cplx in (False, True):
            psi = fill_randn(pkg, src, src.N, cplx, 3000 + nup + cplx)
            for q in (0.0, 2 * np.pi * 3 / L):
                spm_into(pkg, src, dst, op, psi, q, out)
                re, im = RR.spm_rows_t(psi, s_dst, L, nup, q, op)
                what = f"L=30 nup={nup} {op} cplx={cplx} q={q:.3f}"
                if q == 0.0:
                    bad = (out.real != re) | (out.imag != im)
                    assert not bool(bad.any()), (what, int(bad.sum()), bad.nonzero().flatten()[:8].tolist())
                else:
                    err, bar = float((out - torch.complex(re, im)).abs().max()), 2e-15 * float(torch.complex(re, im).abs().max())
                    print(f"{what}: {err:.2e} (bar {bar:.2e})")
                    assert err <= bar, what
                top = max(top, float(re.abs().max()))
        first = out.clone()
        assert torch.equal(torch.view_as_real(spm_into(pkg, src, dst, op, psi, q, out)), torch.view_as_real(first))
        assert top > 0.1
        del out, first, s_dst


# ---- 3. two tiled plans with different suffix bits ----
def test_differently_tiled_source_and_target_give_the_same_bits(pkg):
    """Only the target's split enters the kernel: a target planned with 12, 13 or 8 suffix sites, or a source planned with 13,
    gives the bits of the pair planned alike.  (An adjacent_sector built after SD_SUFFIX_BITS changed is such a pair.)"""
    import torch
    L, nup, q = 16, 8, 0.3
    src = build(pkg, L, nup, None)
    src13 = build(pkg, L, nup, 13)
    assert len(tile_lengths(src)) == 16 and len(tile_lengths(src13)) == 8
    psi = fill_randn(pkg, src, src.N, True, 77)
    host = psi.cpu().numpy()
    for op in ("minus", "plus"):
        t = nup + OPS[op][1]
        dsts = {ls: build(pkg, L, t, ls) for ls in (None, 13, 8)}
        counts = {ls: len(tile_lengths(m)) for ls, m in dsts.items()}
        assert counts == {None: 16, 13: 8, 8: 255}                     # three different plans of the same sector
        assert tile_lengths(dsts[13]).max() > 1024 and tile_lengths(dsts[8]).max() <= 128
        dev = device_of(src)
        base = spm_into(pkg, src, dsts[None], op, psi, q, nan_complex(dsts[None].N, dev))
        top = check_phi(base.cpu().numpy(), R.spm(L, nup, host, q, op), q, f"L=16 {op} same plan")
        assert top > 0.1
        out = nan_complex(dsts[None].N, dev)
        for s, ls in ((src, 13), (src, 8), (src13, None), (src13, 13), (src13, 8)):
            spm_into(pkg, s, dsts[ls], op, psi, q, out)
            bad = (torch.view_as_real(out) != torch.view_as_real(base)).any(dim=1)
            assert not bool(bad.any()), (op, s is src13, ls, int(bad.sum()), bad.nonzero().flatten()[:8].tolist())
        assert torch.equal(torch.view_as_real(spm_into(pkg, src, dsts[None], op, psi, q, out)), torch.view_as_real(base))


# ---- 4. one-row and tiny targets ----
@pytest.mark.parametrize("L,nup,op", [(13, 1, "minus"), (13, 12, "plus"), (2, 1, "minus"), (2, 1, "plus"), (1, 1, "minus"), (1, 0, "plus")])
def test_one_row_and_tiny_targets_match_numpy(pkg, L, nup, op):
    src = build(pkg, L, nup, None)
    dst = build(pkg, L, nup + OPS[op][1], None)
    assert dst.N == 1 and dst.nup in (0, L) and src.N == L
    out = nan_complex(dst.N, device_of(dst))
    top = 0.0
    for cplx in (False, True):
        psi = fill_randn(pkg, src, src.N, cplx, 10 * L + nup + cplx)
        host = psi.cpu().numpy()
        for q in (0.0, 0.7):
            got = spm_into(pkg, src, dst, op, psi, q, out).cpu().numpy()
            top = max(top, check_phi(got, R.spm(L, nup, host, q, op), q, f"L={L} nup={nup} {op} cplx={cplx} q={q}"))
    again = spm_into(pkg, src, dst, op, psi, 0.7, out).cpu().numpy()
    assert np.array_equal(got.view(np.float64), again.view(np.float64))
    assert top > 0.1


# ---- 5. the capped grids of k_spm_full and k_spm_rows ----
def free_device_memory(pkg, need, what):
    import torch
    gc.collect()
    torch.cuda.empty_cache()                 # what earlier tests left in torch's caching allocator is not "in use" ...
    pkg.default_context().release_scratch()  # ... nor are the work vectors the library's context keeps between calls
    free, _ = torch.cuda.mem_get_info()
    if free < need + (3 << 30):
        pytest.skip(f"not enough device memory: {what} needs {need} bytes and 3 GiB of room, {free} are free")


def cap_rows(N, seed):
    """rows on both sides of the cap and of the last block, and 1500 random ones below and above the cap"""
    assert N > CAP
    rng = np.random.default_rng(seed)
    last = (N - 1) // 256 * 256                          # the first row of the last (partial or full) block
    rows = np.concatenate([[0, CAP - 1, CAP, CAP + 1, N - 1, last], rng.integers(0, CAP, 1500), rng.integers(CAP, N, 1500)])
    rows = np.unique(rows.astype(np.int64))
    assert (rows < CAP).sum() > 1400 and (rows >= CAP).sum() > 1400
    return rows


def check_sampled(pkg, src, dst, op, psi, out, rows, states, what):
    """q = 2 pi 3 / L and q = 0 on the random vector psi: no NaN left in any row, and the sampled rows against the numpy row loop"""
    import torch
    dev = psi.device
    L = src.L
    rows_t = torch.from_numpy(rows).to(dev)

    def psi_at(j):
        return psi[torch.as_tensor(j, device=dev)].cpu().numpy()
    top = 0.0
    for q in (2 * np.pi * 3 / L, 0.0):
        spm_into(pkg, src, dst, op, psi, q, out)
        assert not bool(torch.isnan(out.real).any()) and not bool(torch.isnan(out.imag).any()), (what, q)
        want = R.spm_rows(L, src.nup, psi_at, states, q, op)
        top = max(top, check_phi(out[rows_t].cpu().numpy(), want, q, f"{what} q={q:.3f}"))
    assert top > 0.1
    first = out[rows_t].clone()                                        # same call twice: equal bits (on the sampled rows)
    spm_into(pkg, src, dst, op, psi, 0.0, out)
    assert torch.equal(torch.view_as_real(out[rows_t]), torch.view_as_real(first))


def check_ones(pkg, src, dst, op, ones, out, count_of_rows, what):
    """psi = 1 everywhere, q = 0: every term is an exact 1.0, so the row is nf times the number of its terms, the imaginary
    part an exact 0 -- on ALL rows.  count_of_rows(lo, hi) -> the counts of rows lo..hi-1 as a float64 tensor, or a number."""
    import torch
    spm_into(pkg, src, dst, op, ones, 0.0, out)
    nf = 1.0 / math.sqrt(src.L)
    step = 1 << 26
    for lo in range(0, dst.N, step):
        hi = min(dst.N, lo + step)
        want = nf * count_of_rows(lo, hi)
        bad = (out.real[lo:hi] != want) | (out.imag[lo:hi] != 0.0)
        assert not bool(bad.any()), (what, lo, int(bad.sum()), (bad.nonzero().flatten()[:8] + lo).tolist())


@pytest.mark.parametrize("cplx", [False, True])
def test_full_basis_two_passes_of_the_capped_grid(pkg, cplx):
    """F29: 2^29 rows are exactly two passes of 2^20 blocks of 256."""
    import torch
    t0 = time.time()
    L = 29
    m = build(pkg, L, None, None)
    N = m.N
    assert pkg.lib().sd_model_path(m.h) == 2 and N == 2 * CAP and (N + 255) // 256 == 2 * (1 << 20)
    free_device_memory(pkg, 16 * N + (16 if cplx else 8) * N + 4 * 8 * (1 << 26), "the full basis of L = 29")
    dev = device_of(m)
    rows = cap_rows(N, L + cplx)                                       # the full basis needs no unrank: row = configuration
    psi = fill_randn(pkg, m, N, cplx, 2900 + cplx)
    out = nan_complex(N, dev)
    for op in ("minus", "plus"):
        check_sampled(pkg, m, m, op, psi, out, rows, rows, f"F29 {op} cplx={cplx}")
    if not cplx:
        psi.fill_(1.0)

        def ups(lo, hi):
            return RR.popcount_t(torch.arange(lo, hi, dtype=torch.int64, device=dev)).to(torch.float64)
        check_ones(pkg, m, m, "minus", psi, out, lambda lo, hi: L - ups(lo, hi), "F29 minus ones")
        check_ones(pkg, m, m, "plus", psi, out, ups, "F29 plus ones")
    del out, psi
    torch.cuda.empty_cache()
    print(f"F29 cplx={cplx}: {time.time() - t0:.1f} s")


@pytest.mark.parametrize("op", ["plus", "minus"])
def test_per_row_target_past_the_capped_grid(pkg, op):
    """R48+ (nup = 7, ComplexF64) and R48- (nup = 9, Float64) into L = 48, nup = 8: 377 348 994 rows > 2^28."""
    import torch
    t0 = time.time()
    L, t = 48, 8
    nup = t - OPS[op][1]
    cplx = op == "plus"
    src = build(pkg, L, nup, None)
    dst = build(pkg, L, t, None)
    N = dst.N
    assert pkg.lib().sd_model_path(dst.h) == 0 and pkg.lib().sd_model_path(src.h) == 0
    assert N == 377348994 and N > CAP and src.N == (73629072 if op == "plus" else 1677106640)
    free_device_memory(pkg, 16 * N + (16 if cplx else 8) * src.N, f"L = 48, nup = {nup} -> 8")
    dev = device_of(dst)
    rows = cap_rows(N, L + nup)
    states = R.unrank(rows, L, t)
    assert np.array_equal(R.rank(states, L, t), rows)
    psi = fill_randn(pkg, src, src.N, cplx, 4800 + nup)
    out = nan_complex(N, dev)
    check_sampled(pkg, src, dst, op, psi, out, rows, states, f"R48 {op}")
    ones = psi if not cplx else torch.empty(src.N, dtype=torch.float64, device=dev)
    ones.fill_(1.0)
    terms = float(L - t if op == "minus" else t)                       # the down (S^-) / up (S^+) sites of a target row
    check_ones(pkg, src, dst, op, ones, out, lambda lo, hi: terms, f"R48 {op} ones")
    del out, psi, ones
    torch.cuda.empty_cache()
    print(f"R48 {op}: {time.time() - t0:.1f} s")
