"""Proves the numpy restatement the GPU tests of the entanglement kernels compare against (tests/entanglement_ref.py): against
explicit loops, both sides against each other and against the singular values, and on states whose entropy is known in closed form.
The entropy functions of the package (host arithmetic) are fed the restatement's Gram matrices.  No device compute is called here."""
import itertools
import math

import numpy as np
import pytest

import entanglement_ref as ER

SHAPES = [(8, 4), (9, 3), (10, 5), (7, 7), (7, 0), (6, None), (2, 1)]


def rand_state(L, nup, cplx, seed=5):
    n = len(ER.basis(L, nup))
    rng = np.random.default_rng(seed + 100 * L + (nup or 0))
    psi = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0.0)
    return psi / np.linalg.norm(psi)


def loops(psi, L, nup, cut, side):
    """the definition, entry by entry: rows and columns in order of first appearance, Python complex arithmetic"""
    if nup is None:
        states = list(range(1 << L))
    else:
        states = [sum(1 << i for i in c) for c in itertools.combinations(range(L), nup)]
    amp = {s: complex(psi[r]) for r, s in enumerate(states)}
    mask = (1 << cut) - 1
    pre, suf = {}, {}
    for s in states:
        P, S = s & mask, s >> cut
        m = -1 if nup is None else bin(P).count("1")
        if P not in pre.setdefault(m, []):
            pre[m].append(P)
        if S not in suf.setdefault(m, []):
            suf[m].append(S)
    out = {}
    for m in pre:
        if side == "A":
            out[m] = np.array([[sum(amp[a | j << cut] * amp[b | j << cut].conjugate() for j in suf[m]) for b in pre[m]] for a in pre[m]])
        else:
            out[m] = np.array([[sum(amp[a | j << cut] * amp[a | k << cut].conjugate() for a in pre[m]) for k in suf[m]] for j in suf[m]])
    return out


@pytest.mark.parametrize("L,nup", SHAPES)
@pytest.mark.parametrize("cplx", [False, True])
def test_restatement_against_explicit_loops(L, nup, cplx):
    psi = rand_state(L, nup, cplx)
    assert list(ER.basis(L, nup)) == ([sum(1 << i for i in c) for c in itertools.combinations(range(L), nup)] if nup is not None
                                      else list(range(1 << L)))
    for cut in range(1, L):
        for side in "AB":
            want = loops(psi, L, nup, cut, side)
            got = ER.gram_blocks(psi, L, nup, cut, side)
            assert sorted(got) == sorted(want)
            for m, (G, K) in got.items():
                assert G.shape == want[m].shape
                assert np.abs(np.asarray(G, dtype=np.complex128) - want[m]).max() <= 1e-14
                assert G.dtype == (np.clongdouble if cplx else np.longdouble)
                assert K == (ER.gram_blocks(psi, L, nup, cut, "BA"[side == "B"])[m][0].shape[0])


@pytest.mark.parametrize("L,nup", SHAPES)
def test_both_sides_have_the_same_spectrum_and_it_is_the_squared_singular_values(L, nup):
    psi = rand_state(L, nup, True)
    for cut in range(1, L):
        sa, sb = ER.spectrum(psi, L, nup, cut, "A"), ER.spectrum(psi, L, nup, cut, "B")
        M = np.asarray(ER.matrix(psi, L, nup, cut), dtype=np.complex128)
        sv = np.sort(np.linalg.svd(M, compute_uv=False) ** 2)[::-1]
        all_a = np.sort(np.concatenate(list(sa.values())))[::-1]
        all_b = np.sort(np.concatenate(list(sb.values())))[::-1]
        r = min(len(all_a), len(all_b))
        assert np.abs(all_a[:r] - all_b[:r]).max() <= 1e-13 and np.abs(all_a[r:]).sum() + np.abs(all_b[r:]).sum() <= 1e-12
        assert np.abs(all_a[:min(r, len(sv))] - sv[:min(r, len(sv))]).max() <= 1e-13
        assert abs(all_a.sum() - 1.0) <= 1e-13
        for m in sa:
            k = min(len(sa[m]), len(sb[m]))
            assert np.abs(sa[m][:k] - sb[m][:k]).max() <= 1e-13
        auto = ER.spectrum(psi, L, nup, cut, "auto")
        for m in auto:
            assert len(auto[m]) == min(len(sa[m]), len(sb[m]))


def one_hot(L, nup, s):
    b = list(ER.basis(L, nup))
    psi = np.zeros(len(b))
    psi[b.index(s)] = 1.0
    return psi


def test_known_entropies(pkg):
    # a product state (one configuration): entropy 0 at every cut
    L, nup = 8, 4
    neel = sum(1 << i for i in range(0, L, 2))
    for cut in range(1, L):
        assert ER.entropy(ER.spectrum(one_hot(L, nup, neel), L, nup, cut)) == 0.0
    # the L = 2 singlet: ln 2
    b = list(ER.basis(2, 1))
    psi = np.zeros(2)
    psi[b.index(0b01)], psi[b.index(0b10)] = 1 / math.sqrt(2), -1 / math.sqrt(2)
    assert abs(ER.entropy(ER.spectrum(psi, 2, 1, 1)) - math.log(2)) <= 1e-15
    # (|P1 S1> + |P2 S2>) / sqrt 2 with P1 != P2, S1 != S2: ln 2, whether the prefixes share a popcount or not
    L, nup, cut = 8, 4, 4
    for (P1, S1), (P2, S2) in (((0b0011, 0b0101), (0b1100, 0b1010)), ((0b0001, 0b0111), (0b0111, 0b0001))):
        b = list(ER.basis(L, nup))
        psi = np.zeros(len(b), dtype=np.complex128)
        psi[b.index(P1 | S1 << cut)] = 1 / math.sqrt(2)
        psi[b.index(P2 | S2 << cut)] = 1j / math.sqrt(2)
        for side in ("A", "B", "auto"):
            sp = ER.spectrum(psi, L, nup, cut, side)
            assert abs(ER.entropy(sp) - math.log(2)) <= 1e-15
            assert abs(ER.entropy(sp, 2) - math.log(2)) <= 1e-15 and abs(ER.entropy(sp, math.inf) - math.log(2)) <= 1e-15


def test_package_entropy_functions_on_the_restatement(pkg):
    """entanglement.py's host arithmetic, fed the restatement's Gram matrices"""
    for L, nup, cut in ((8, 4, 4), (9, 3, 2), (10, 5, 7), (6, None, 3)):
        psi = 3.0 * rand_state(L, nup, True)                        # not normalised: the package divides by the total trace
        G = {m: np.asarray(g, dtype=np.complex128) for m, (g, _) in ER.gram_blocks(psi, L, nup, cut, "auto").items()}
        sp = pkg.spectrum_from_blocks(G)
        ref = ER.spectrum(psi, L, nup, cut)
        for m in ref:
            assert np.abs(sp[m] - ref[m]).max() <= 1e-14 and (np.diff(sp[m]) <= 0).all() and (sp[m] >= 0).all()
        for q in (1, 2, 0.5, 3, math.inf):
            assert abs(pkg.entropy_from_spectrum(sp, q) - ER.entropy(ref, q)) <= 1e-12
        many = pkg.entropy_from_spectrum(sp, [1, 2, math.inf])
        assert many.shape == (3,) and many[0] == pkg.entropy_from_spectrum(sp, 1)
        sr = pkg.symmetry_resolved_from_spectrum(sp)
        assert abs(sum(sr["p"].values()) - 1.0) <= 1e-13
        assert abs(sr["S_total"] - ER.entropy(ref, 1)) <= 1e-12 and abs(sr["S_number"] + sr["S_config"] - sr["S_total"]) == 0.0
        assert 0.0 <= sr["S_number"] <= sr["S_total"] + 1e-13
    # the known states through the package's functions
    b = list(ER.basis(2, 1))
    psi = np.zeros(2)
    psi[b.index(1)], psi[b.index(2)] = 1.0, -1.0
    sp = pkg.spectrum_from_blocks({m: np.asarray(g, dtype=np.float64) for m, (g, _) in ER.gram_blocks(psi, 2, 1, 1, "A").items()})
    assert abs(pkg.entropy_from_spectrum(sp) - math.log(2)) <= 1e-15
    sr = pkg.symmetry_resolved_from_spectrum(sp)
    assert abs(sr["S_number"] - math.log(2)) <= 1e-15 and sr["S_config"] == 0.0
    one = pkg.spectrum_from_blocks({0: np.array([[2.0]])})
    assert pkg.entropy_from_spectrum(one) == 0.0 and pkg.entropy_from_spectrum(one, math.inf) == 0.0
    with pytest.raises(pkg.ArgumentError):
        pkg.entropy_from_spectrum(one, 0.0)
    with pytest.raises(pkg.ArgumentError):
        pkg.spectrum_from_blocks({0: np.zeros((2, 2))})
