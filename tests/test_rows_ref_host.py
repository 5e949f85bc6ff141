"""The yardstick of tests/test_gpu_operator_grids.py and tests/test_gpu_transverse_grids.py, proven without a GPU: the row
restatements of tests/rows_ref.py (torch, run here on the CPU) against the numpy restatement of tests/typicality_ref.py -- itself
proven against Kronecker products by tests/test_typicality_host.py -- S^-+_q against tests/transverse_ref.py, and the two ports
of the combinadic order against each other."""
from math import comb

import numpy as np
import pytest
import torch

import rows_ref as RR
import transverse_ref as T
import typicality_ref as R


def chain(L, boundary="open", Jxy=1.0):
    hop = [(i, i + 1, Jxy / 2) for i in range(1, L)]
    if boundary == "periodic":
        hop.append((L, 1, Jxy / 2))
    return hop


def j1j2(L, J1=1.0, J2=0.4):
    return [(i, i % L + 1, J1 / 2) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2 / 2) for i in range(1, L + 1)]


def long_range(L):
    return [(i, j, 0.5 / (j - i) ** 2) for i in range(1, L + 1) for j in range(i + 1, L + 1)]


HOPS = {"open": lambda L: chain(L, "open", 0.8), "periodic": lambda L: chain(L, "periodic", 0.8), "j1j2": j1j2,
        "long_range": long_range, "self_hop": lambda L: chain(L, "periodic") + [(3, 3, 0.7)]}


@pytest.mark.parametrize("name,L,nup", [("open", 8, 4), ("periodic", 12, 6), ("periodic", 14, 7), ("periodic", 13, 1), ("periodic", 11, 10),
                                        ("j1j2", 12, 5), ("j1j2", 14, 3), ("long_range", 10, 5), ("long_range", 12, 2),
                                        ("periodic", 10, None), ("j1j2", 12, None), ("long_range", 9, None), ("self_hop", 9, 4),
                                        ("open", 9, 0), ("open", 9, 9)])
def test_current_rows_equal_the_numpy_row_loop_bit_for_bit(name, L, nup):
    hop = HOPS[name](L)
    states, index = R.basis(L, nup)
    N = len(states)
    plan = R.CurrentPlan(L, nup, hop, states, index)
    rng = np.random.default_rng(L)
    real = rng.standard_normal(N)
    cplx = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    wsets = [None, np.eye(len(hop))[len(hop) // 2], rng.standard_normal(len(hop))]
    rows = torch.arange(N, dtype=torch.int64)
    s = RR.configurations_t(rows, L, nup)
    assert np.array_equal(s.numpy().astype(np.uint64), states)
    got = RR.current_rows([torch.from_numpy(real), torch.from_numpy(cplx)], wsets, s, rows, L, nup, hop)
    for k, psi in enumerate((real, cplx)):
        for m, w in enumerate(wsets):
            want = plan.apply(psi, w)
            re, im = got[(k, m)]
            assert np.array_equal(re.numpy(), want.real) and np.array_equal(im.numpy(), want.imag), (name, L, nup, k, m)
    assert np.abs(plan.apply(cplx)).max() > 0.1 or nup in (0, L)           # a real comparison, not zeros against zeros


@pytest.mark.parametrize("L,nup", [(1, 0), (1, 1), (6, 3), (9, 0), (9, 9), (13, 4), (14, 7), (16, 15)])
def test_numpy_and_torch_ports_of_the_combinadic_order_agree(L, nup):
    N = comb(L, nup)
    rows = np.arange(N, dtype=np.int64)
    s = RR.unrank(rows, L, nup)
    states, _ = R.basis(L, nup)
    assert np.array_equal(s, states)                                     # both are the lexicographic-combination order
    st = RR.unrank_t(torch.from_numpy(rows), L, nup)
    assert np.array_equal(st.numpy().astype(np.uint64), s)
    assert np.array_equal(RR.rank(s, L, nup), rows)
    assert np.array_equal(RR.rank_t(st, L, nup).numpy(), rows)


@pytest.mark.parametrize("L,nup", [(39, 6), (34, 17)])
def test_rank_inverts_unrank_on_sampled_rows_of_the_large_sectors(L, nup):
    N = comb(L, nup)
    rng = np.random.default_rng(L)
    rows = np.unique(np.concatenate([np.arange(2048), np.arange(N - 2048, N), rng.integers(0, N, 20000),
                                     np.array([2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1]) % N]).astype(np.int64))
    s = RR.unrank(rows, L, nup)
    assert (np.array([bin(int(x)).count("1") for x in s[:500]]) == nup).all() and int(s.max()) < (1 << L)
    assert np.array_equal(RR.rank(s, L, nup), rows)
    assert (np.diff(s[:2048].astype(np.int64)) != 0).all()
    st = RR.unrank_t(torch.from_numpy(rows), L, nup)
    assert np.array_equal(st.numpy().astype(np.uint64), s)
    assert np.array_equal(RR.rank_t(st, L, nup).numpy(), rows)
    # the first row has the lowest sites up, the last row the highest
    assert int(s[0]) == (1 << nup) - 1 and int(s[-1]) == ((1 << nup) - 1) << (L - nup)


@pytest.mark.parametrize("L,nup", [(10, 5), (9, None), (12, 3)])
def test_szq_rows_and_site_signs_against_the_numpy_restatement(L, nup):
    states, _ = R.basis(L, nup)
    N = len(states)
    rng = np.random.default_rng(L)
    s = torch.from_numpy(states.astype(np.int64))
    for i in range(1, L + 1):
        assert np.array_equal(RR.site_sz(s, i).numpy(), R.sz_site(states, i))
    for psi in (rng.standard_normal(N), rng.standard_normal(N) + 1j * rng.standard_normal(N)):
        for q in (0.3, 2 * np.pi * 5 / L):
            want = R.sz_q(states, L, q) * psi
            got = RR.szq_rows(torch.from_numpy(psi), s, L, q).numpy()
            assert np.abs(got - want).max() <= 4e-16 * np.sqrt(L) * np.abs(psi).max()     # a few roundings of sums below sqrt(L)/2
    k = int(states[N // 3])
    sz = np.array([R.sz_site(states[N // 3:N // 3 + 1], i)[0] for i in range(1, L + 1)])
    assert np.array_equal(RR.lag_sums(k, L), np.array([np.sum(sz * np.roll(sz, -r)) for r in range(L)]))
    szs = np.array([R.sz_site(states, i) for i in range(1, L + 1)])
    for r in range(L):
        assert np.array_equal(RR.lag_sums_t(s, L, r).numpy(), np.sum(szs * np.roll(szs, -r, axis=0), axis=0))


@pytest.mark.parametrize("L,nup", [(10, 5), (10, 1), (10, 9), (10, None), (13, 6)])
@pytest.mark.parametrize("op", ["minus", "plus"])
def test_spm_rows_equal_the_numpy_restatement_bit_for_bit(L, nup, op):
    """`spm_rows_t` against tests/transverse_ref.py: the two share the definition only (another rank, another way of skipping
    the rows a site does not reach), so they are held to equality.  nup = 1 -> 0 and nup = L - 1 -> L are one-row targets."""
    N = (1 << L) if nup is None else comb(L, nup)
    nup_dst = None if nup is None else nup + (-1 if op == "minus" else 1)
    n_dst = (1 << L) if nup is None else comb(L, nup_dst)
    rng = np.random.default_rng(100 * L + (nup or 0))
    real = rng.standard_normal(N)
    cplx = rng.standard_normal(N) + 1j * rng.standard_normal(N)
    s_dst = RR.configurations_t(torch.arange(n_dst, dtype=torch.int64), L, nup_dst)
    if nup is not None:
        assert np.array_equal(s_dst.numpy(), T.sector_states(L, nup_dst))
    top = 0.0
    for psi in (real, cplx):
        for q in (0.0, 0.3, 2 * np.pi * 3 / L):
            want = T.spm(L, nup, psi, q, op)
            re, im = RR.spm_rows_t(torch.from_numpy(psi), s_dst, L, nup, q, op)
            assert re.dtype == torch.float64 and re.shape == (n_dst,) and im.shape == (n_dst,)
            assert np.array_equal(re.numpy(), want.real) and np.array_equal(im.numpy(), want.imag), (L, nup, op, q)
            top = max(top, np.abs(want).max())
    assert top > 0.1                                                       # a real comparison, not zeros against zeros


def test_popcount_of_wide_configurations():
    rng = np.random.default_rng(1)
    x = np.concatenate([rng.integers(0, 1 << 62, 5000), [0, 1, (1 << 62) - 1, (1 << 39) - 1, 1 << 61]]).astype(np.int64)
    assert np.array_equal(RR.popcount_t(torch.from_numpy(x)).numpy(), np.array([bin(int(v)).count("1") for v in x]))
    s = torch.from_numpy(x & ((1 << 39) - 1))
    want = np.array([RR.lag_sums(int(v), 39) for v in s.numpy()])
    for r in (0, 1, 7, 20, 38):
        assert np.array_equal(RR.lag_sums_t(s, 39, r).numpy(), want[:, r])


@pytest.mark.parametrize("op,mat", [("z", R.SZ), ("plus", R.SP), ("minus", R.SM), ("x", 0.5 * (R.SP + R.SM)),
                                    ("y", -0.5j * (R.SP - R.SM))])
def test_spin_operator_rows_equal_the_kronecker_form(op, mat):
    L = 7
    rng = np.random.default_rng(3)
    cplx = rng.standard_normal(1 << L) + 1j * rng.standard_normal(1 << L)
    for site in (1, 4, L):
        M = R.kron_site(L, site, mat)
        for psi in ((cplx,) if op == "y" else (cplx, cplx.real.copy())):
            got = RR.spin_operator_rows(torch.from_numpy(psi), site, op).numpy()
            assert np.array_equal(got, M @ psi)          # one non-zero term per row: copies, sign flips and halvings
