"""tests/basis_stats_ref.py proven on the CPU: against explicit Python loops over the oracle's basis for L <= 12, and on exact
states (a basis state, the uniform state, the L = 2 singlet).  The loops use math.fsum, so the bars below are the restatement's own
rounding: sums of at most N = 4096 non-negative terms, a few eps relative."""
import math

import numpy as np
import pytest

import basis_stats_ref as BR

CASES = [(2, 1), (6, 3), (9, 2), (10, 4), (12, 6), (8, None), (12, None)]


def random_state(N, cplx, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(N) + (1j * rng.standard_normal(N) if cplx else 0.0)
    return x if cplx else x.real.copy()


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("L,nup", CASES)
def test_against_loops_over_the_oracle_basis(O, L, nup, cplx):
    ref = O.XXZChain(L, nup=nup)
    states = [int(s) for s in ref.states]
    N = len(states)
    psi = random_state(N, cplx, 100 * L + (nup or 0))
    psi[N // 3] = 0.0                                          # a zero weight: its w ln w term is 0, and no shot may land on it
    w = [float(z.real) ** 2 + float(z.imag) ** 2 for z in psi]
    W = math.fsum(w)
    # moments
    qs = (0.5, 2.0, 3.0, 2.5)
    mom = BR.moments(psi, qs)
    assert abs(mom["W"] - W) <= 1e-14 * W
    wlnw = math.fsum(x * math.log(x) for x in w if x > 0)
    assert abs(mom["wlnw"] - wlnw) <= 1e-14 * math.fsum(abs(x * math.log(x)) for x in w if x > 0)
    assert mom["wmax"] == max(w) and mom["argmax"] == w.index(max(w))
    for k, q in enumerate(qs):
        want = math.fsum(x ** q for x in w if x > 0)
        assert abs(mom["sums"][k] - want) <= 1e-13 * want, (q, mom["sums"][k], want)
    # counting: all single sites, all cuts, a scattered mask, the empty and the full mask
    masks = [1 << i for i in range(L)] + [(1 << k) - 1 for k in range(1, L)] + [0b1011010110101 & ((1 << L) - 1), 0, (1 << L) - 1]
    P = BR.counting(psi, L, nup, masks)
    assert P.shape == (len(masks), L + 1)
    for k, mask in enumerate(masks):
        want = [math.fsum(x for x, s in zip(w, states) if bin(s & mask).count("1") == m) for m in range(L + 1)]
        assert np.abs(P[k] - np.array(want)).max() <= 1e-14 * W, (mask, P[k], want)
        lo, hi = BR.reachable(L, nup, mask)
        assert all(P[k, m] == 0.0 for m in range(L + 1) if m < lo or m > hi)
        if N >= 20:                                            # (in a basis of two rows the zeroed row may be a bin's only one)
            assert P[k, lo] > 0 and P[k, hi] > 0
    # snapshots: the interval rule accepts the rows of a plain sequential inversion and refuses their neighbours
    shots, seed = 500, 11 + L
    u = BR.uniforms(seed, 0, shots)
    C = np.cumsum(np.array(w))
    rows = []
    for k in range(shots):
        t, run, pick = u[k] * C[-1], 0.0, None
        for r, x in enumerate(w):
            run += x
            if x > 0 and run > t:
                pick = r
                break
        rows.append(pick if pick is not None else max(r for r, x in enumerate(w) if x > 0))
    rows = np.array(rows)
    worst, bad = BR.snapshot_violation(rows, psi, seed)
    assert worst <= 1.0 and bad == 0
    assert N // 3 not in rows
    if N >= 6:
        shifted = np.where(rows + 1 < N, rows + 1, rows - 1)
        assert BR.snapshot_violation(shifted, psi, seed)[0] > 1.0        # one row off fails
        onzero = rows.copy()
        onzero[0] = N // 3
        assert BR.snapshot_violation(onzero, psi, seed)[1] == 1          # a row of weight 0 is counted
        assert BR.snapshot_violation(np.append(rows[:-1], N), psi, seed)[1] == 1


def test_exact_states(O):
    # a basis state: every S_q is 0.0 exactly and P is one-hot
    L, nup = 10, 5
    ref = O.XXZChain(L, nup=nup)
    N = len(ref.states)
    for amp in (1.0, 1j, 2.0):
        psi = np.zeros(N, dtype=type(amp))
        psi[77] = amp
        mom = BR.moments(psi, (0.5, 2.0, 3.0))
        if abs(amp) == 1.0:
            for k, q in enumerate((0.5, 2.0, 3.0)):
                assert BR.entropy(mom, q, k) == 0.0
            assert BR.entropy(mom, 1) == 0.0 and BR.entropy(mom, math.inf) == 0.0
        assert mom["argmax"] == 77
        cfg = int(ref.states[77])
        cut = (1 << 4) - 1
        P = BR.counting(psi, L, nup, [cut])
        want = np.zeros(L + 1)
        want[bin(cfg & cut).count("1")] = abs(amp) ** 2
        assert np.array_equal(P[0], want)
        worst, bad = BR.snapshot_violation(np.full(40, 77), psi, 5)
        assert worst <= 1.0 and bad == 0
        assert BR.snapshot_violation(np.full(40, 76), psi, 5)[1] == 40
    # the uniform state: S_q = ln N
    psi = np.full(N, 1.0 / math.sqrt(N))
    mom = BR.moments(psi, (0.5, 2.0, 2.5))
    for k, q in enumerate((0.5, 2.0, 2.5)):
        assert abs(BR.entropy(mom, q, k) - math.log(N)) <= 1e-12
    assert abs(BR.entropy(mom, 1) - math.log(N)) <= 1e-12 and abs(BR.entropy(mom, math.inf) - math.log(N)) <= 1e-12
    assert mom["argmax"] == 0                                # the tie goes to the lowest row
    # the L = 2 singlet: each site is up with probability 1/2
    s2 = O.XXZChain(2, nup=1)
    assert [int(x) for x in s2.states] == [1, 2]
    psi = np.array([1.0, -1.0]) / math.sqrt(2.0)
    P = BR.counting(psi, 2, 1, [0b01, 0b10, 0b11])
    assert np.abs(P[0] - np.array([0.5, 0.5, 0.0])).max() <= 1e-15 and np.abs(P[1] - np.array([0.5, 0.5, 0.0])).max() <= 1e-15
    assert np.abs(P[2] - np.array([0.0, 1.0, 0.0])).max() <= 1e-15 and P[2, 0] == 0.0 and P[2, 2] == 0.0
