"""tests/ecurrent_ref.py, the restatement the energy-current tests compare against, proven on the CPU against dense
Kronecker-product operators: the term builder against (i/2) sum d [h_a, h_b] and, on lines, against i [H, sum x_a h_a]; the row
loop against the projected dense matrix; and the commutators that make J_E a check of the apply: [H, J_E] = 0 on the zero-field
XXZ ring and not with second neighbours or a field."""
import numpy as np
import pytest

import ecurrent_ref as ER
import typicality_ref as TR


def xxz(L, boundary, Jxy=0.8, Jz=0.7, hz=0.3):
    hop = [(i, i + 1, Jxy / 2) for i in range(1, L)]
    zz = [(i, i + 1, Jz) for i in range(1, L)]
    if boundary == "periodic" and L > 2:
        hop.append((L, 1, Jxy / 2))
        zz.append((L, 1, Jz))
    return hop, zz, np.full(L, hz)


def j1j2(L, J1=1.0, J2=0.4, h=0.1):
    hop = [(i, i % L + 1, J1 / 2) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2 / 2) for i in range(1, L + 1)]
    zz = [(i, i % L + 1, J1) for i in range(1, L + 1)] + [(i, (i + 1) % L + 1, J2) for i in range(1, L + 1)]
    return hop, zz, np.full(L, h)


def random_line(L, seed):
    rng = np.random.default_rng(seed)
    pairs = [(i, j) for i in range(1, L + 1) for j in range(i + 1, min(i + 3, L) + 1)]
    hop = [((i, j) if rng.random() < 0.5 else (j, i)) + (rng.standard_normal(),) for i, j in pairs]
    zz = [(i, j, rng.standard_normal()) for i, j in pairs]
    return hop, zz, rng.standard_normal(L)


CASES = [("xxz-open", L, xxz(L, "open"), False) for L in (3, 6, 7)]
CASES += [("xxz-ring", L, xxz(L, "periodic"), True) for L in (3, 6, 7)]
CASES += [("j1j2-ring", 7, j1j2(7), True), ("random-line", 6, random_line(6, 5), False)]


@pytest.mark.parametrize("name,L,lists,periodic", CASES, ids=[f"{c[0]}-L{c[1]}" for c in CASES])
def test_builder_against_dense_commutators(name, L, lists, periodic):
    hop, zz, field = lists
    terms = ER.energy_current_terms(L, hop, zz, field, periodic)
    J = ER.kron_terms(L, terms)
    D = ER.dense_energy_current(L, hop, zz, field, periodic)
    scale = np.abs(D).max()
    assert scale > 0.1
    err = np.abs(J - D).max()
    print(f"{name} L={L}: {len(terms)} terms, |J - dense| = {err:.2e} (bar {1e-13 * scale:.2e})")
    assert err <= 1e-13 * scale
    assert np.abs(J - J.conj().T).max() <= 1e-13 * scale                      # Hermitian
    if not periodic:
        B = ER.dense_boost_current(L, hop, zz, field)
        assert np.abs(J - B).max() <= 1e-13 * scale
    # the list's order and form: oriented, merged, no zeros, sorted
    keys = [(int(t["i"]), int(t["j"]), int(t["k"])) for t in terms]
    assert keys == sorted(set(keys)) and all(i < j and k not in (i, j) for i, j, k in keys) and np.all(terms["c"] != 0.0)


@pytest.mark.parametrize("cplx", [False, True], ids=["f64", "c128"])
@pytest.mark.parametrize("L,nup", [(8, 3), (8, 4), (9, 0), (9, 9), (8, None)])
def test_row_loop_against_projected_dense(L, nup, cplx):
    hop, zz, field = j1j2(L) if L == 8 else xxz(L, "periodic")
    terms = ER.energy_current_terms(L, hop, zz, field, True)
    # a hand list on top: a reversed pair, and a k = 0 term between two dressed terms of one group
    hand = np.array([(5, 2, 7, 0.3), (2, 5, 1, 0.7), (2, 5, 0, -0.4), (2, 5, 8, 1.1)], dtype=ER.DTERM)
    rng = np.random.default_rng(11 * L + (nup or 0))
    states, _ = TR.basis(L, nup)
    psi = rng.standard_normal(len(states)) + (1j * rng.standard_normal(len(states)) if cplx else 0.0)
    for tl in (terms, hand):
        want = TR.project(ER.kron_terms(L, tl), states) @ psi
        got = ER.apply_rows(tl, psi, L, nup)
        assert got.shape == want.shape
        assert np.abs(got - want).max() <= 1e-13 * np.linalg.norm(psi)
        if nup in (0, L):
            assert not got.any()


def test_commutators_with_H():
    L = 8

    def comm(lists):
        hop, zz, field = lists
        H = TR.kron_hamiltonian(L, hop, zz, field)
        J = ER.kron_terms(L, ER.energy_current_terms(L, hop, zz, field, True))
        return np.abs(H @ J - J @ H).max()

    ring0, ringh = comm(xxz(L, "periodic", Jxy=1.0, hz=0.0)), comm(xxz(L, "periodic", Jxy=1.0, hz=0.3))
    jj = comm(j1j2(L, h=0.0))
    print(f"|[H, J_E]|_max: zero-field XXZ ring {ring0:.2e}, hz = 0.3 {ringh:.3f}, J1-J2 ring {jj:.3f}")
    assert ring0 <= 1e-14
    assert jj >= 0.1
    assert ringh >= 0.1


def test_ambiguous_minimum_image_is_refused():
    hop = [(1, 5, 0.5), (5, 6, 0.5)]
    with pytest.raises(ER.Ambiguous):
        ER.energy_current_terms(8, hop, [], None, True)
    assert len(ER.energy_current_terms(8, hop, [], None, False)) == 1
