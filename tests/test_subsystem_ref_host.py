"""tests/subsystem_ref.py against explicit loops and states of known answer (no GPU): the restatement the GPU tests of DESIGN.md 22
compare with has to be right on its own."""
import math

import numpy as np
import pytest

import entanglement_ref as ER
import subsystem_ref as SR


def random_state(L, nup, cplx, seed):
    n = len(SR.basis(L, nup))
    rng = np.random.default_rng(seed)
    psi = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)
    return psi / np.linalg.norm(psi)


def test_basis_is_the_combinadic_order():
    for L, nup in ((6, 3), (7, 2), (5, None), (4, 0), (4, 4)):
        assert SR.basis(L, nup) == [int(x) for x in ER.basis(L, nup)]


@pytest.mark.parametrize("L,nup", [(6, 3), (7, 2), (5, None)])
def test_permute_against_explicit_loops(L, nup):
    """U|s> = |pi s>: the amplitude of configuration s lands on the configuration whose site perm[i] carries the spin of site i + 1"""
    rng = np.random.default_rng(5 + L)
    st = SR.basis(L, nup)
    psi = random_state(L, nup, True, 17)
    for perm in (SR.translation(L), SR.reflection(L), list(rng.permutation(L) + 1), list(range(1, L + 1))):
        want = np.zeros_like(psi)
        for k, s in enumerate(st):
            t = 0
            for i in range(L):
                if (s >> i) & 1:
                    t |= 1 << (perm[i] - 1)
            want[st.index(t)] = psi[k]
        assert np.array_equal(SR.permute(psi, L, nup, perm), want)
    # T rotates left by one, R reverses the bits
    mask = (1 << L) - 1
    T = SR.permute(psi, L, nup, SR.translation(L))
    R = SR.permute(psi, L, nup, SR.reflection(L))
    for k, s in enumerate(st):
        assert T[st.index(((s << 1) | (s >> (L - 1))) & mask)] == psi[k]
        assert R[st.index(int(format(s, "0%db" % L)[::-1], 2))] == psi[k]


def test_stable_partition_layout():
    assert SR.stable_partition(6, [3, 4]) == [3, 4, 1, 2, 5, 6]
    assert SR.stable_partition(6, [6, 2]) == [3, 2, 4, 5, 6, 1]
    assert SR.stable_partition(5, [1, 2, 3]) == [1, 2, 3, 4, 5]


@pytest.mark.parametrize("L,nup", [(6, 3), (7, 2), (5, None)])
def test_rho_against_explicit_loops(L, nup):
    st = SR.basis(L, nup)
    psi = random_state(L, nup, True, 23)
    amp = dict(zip(st, psi))
    for sites in ([2, 4], [L], [3, 1, L], [L, L - 1, 1, 2]):
        s = len(sites)
        rest = [x for x in range(1, L + 1) if x not in sites]
        want = np.zeros((1 << s, 1 << s), dtype=complex)
        for a in range(1 << s):
            for b in range(1 << s):
                for e in range(1 << len(rest)):
                    ca = sum(((a >> j) & 1) << (x - 1) for j, x in enumerate(sites)) | sum(((e >> j) & 1) << (x - 1) for j, x in enumerate(rest))
                    cb = sum(((b >> j) & 1) << (x - 1) for j, x in enumerate(sites)) | sum(((e >> j) & 1) << (x - 1) for j, x in enumerate(rest))
                    want[a, b] += amp.get(ca, 0.0) * np.conj(amp.get(cb, 0.0))
        got = np.asarray(SR.rho(psi, L, nup, sites), dtype=complex)
        assert np.abs(got - want).max() <= 1e-15
        assert abs(np.trace(got).real - 1.0) <= 1e-14


def test_rho_of_a_prefix_is_the_cut_restatement():
    """sites = 1..k: the blocks are those of tests/entanglement_ref.py, side A, entry for entry"""
    for L, nup, k in ((8, 4, 3), (7, 3, 5), (6, None, 2)):
        psi = random_state(L, nup, True, 31)
        got = SR.blocks(SR.rho(psi, L, nup, list(range(1, k + 1))), k, nup, L)
        ref = ER.gram_blocks(psi, L, nup, k, "A")
        assert sorted(got) == sorted(ref)
        for m in ref:
            assert got[m][1] == ref[m][1]
            assert np.abs(np.asarray(got[m][0] - ref[m][0], dtype=complex)).max() <= 1e-17


def test_rho_blocks_are_the_blocks_of_rho():
    for L, nup, sites in ((8, 4, [6, 2, 3]), (7, 3, [7, 6, 5, 4, 2, 1]), (6, None, [5, 1])):
        psi = random_state(L, nup, True, 37)
        R = SR.rho(psi, L, nup, sites)
        a, b = SR.rho_blocks(psi, L, nup, sites), SR.blocks(R, len(sites), nup, L)
        assert sorted(a) == sorted(b)
        covered = np.zeros(R.shape, dtype=bool)
        for m in a:
            assert a[m][1] == b[m][1] and np.array_equal(a[m][0], b[m][0])
            idx = np.arange(R.shape[0]) if nup is None else np.array(SR.basis(len(sites), m))
            covered[np.ix_(idx, idx)] = True
        assert (R[~covered] == 0).all()                       # nothing of rho lies outside the blocks


def test_partial_transpose_loops():
    rng = np.random.default_rng(3)
    R = rng.standard_normal((8, 8)) + 1j * rng.standard_normal((8, 8))
    PT = SR.partial_transpose(R, 1, 2)
    assert np.array_equal(SR.partial_transpose(PT, 1, 2), R)
    assert PT[1 + (2 << 1), 0 + (3 << 1)] == R[1 + (3 << 1), 0 + (2 << 1)]
    assert np.array_equal(SR.partial_transpose(R, 3, 0), R)
    assert np.array_equal(SR.partial_transpose(R, 0, 3), R.T)


def test_singlet_product_known_answers():
    """singlets on (1, L) and (2, 3), the rest polarised: I({1}:{L}) = 2 ln 2, E_N({1},{L}) = ln 2, I({1}:{2}) = 0"""
    L = 8
    for nup in (2, 4, 6):                      # 0, 2 or all 4 of the remaining sites up
        psi = SR.singlet_product_state(L, nup, [(1, L), (2, 3)])
        assert abs(np.linalg.norm(psi) - 1.0) <= 1e-15
        assert abs(SR.mutual_information(psi, L, nup, [1], [L]) - 2 * math.log(2)) <= 1e-14
        assert abs(SR.log_negativity(psi, L, nup, [1], [L]) - math.log(2)) <= 1e-14
        assert abs(SR.mutual_information(psi, L, nup, [1], [2])) <= 1e-14
        assert abs(SR.log_negativity(psi, L, nup, [1], [2])) <= 1e-14
        assert abs(SR.mutual_information(psi, L, nup, [2], [3]) - 2 * math.log(2)) <= 1e-14
        assert abs(SR.entropy(SR.rho(psi, L, nup, [1, L]))) <= 1e-14            # the pair is pure
        assert abs(SR.entropy(SR.rho(psi, L, nup, [1, 2])) - 2 * math.log(2)) <= 1e-14
        # the two-site matrix of the singlet in the basis index = bit(1) + 2 bit(L)
        R = np.asarray(SR.rho(psi, L, nup, [1, L]), dtype=complex)
        want = np.zeros((4, 4))
        want[1, 1] = want[2, 2] = 0.5
        want[1, 2] = want[2, 1] = -0.5
        assert np.abs(R - want).max() <= 1e-15


def test_entropy_of_complement_and_mutual_information_of_a_covering_pair():
    L, nup = 8, 3
    psi = random_state(L, nup, True, 41)
    A, B = [2, 5, 7], [1, 3, 4, 6, 8]
    assert abs(SR.entropy(SR.rho(psi, L, nup, A)) - SR.entropy(SR.rho(psi, L, nup, B))) <= 1e-12
    assert abs(SR.mutual_information(psi, L, nup, A, B) - 2 * SR.entropy(SR.rho(psi, L, nup, A))) <= 1e-12
