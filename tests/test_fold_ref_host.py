"""The yardstick of tests/test_gpu_fold_kernels.py, proven without a GPU: every function of tests/fold_ref.py against exact rational
arithmetic rounded once per stated operation (fractions.Fraction is exact, float(Fraction) is correctly rounded); and that the
inputs of the GPU cells can tell apart what those cells are there to tell apart -- form 0 from form 1, the block's summation order
from a plain left-to-right sum, the waves summed in reverse, a block's partial from its neighbour's."""
from fractions import Fraction as Fr

import numpy as np
import pytest

import fold_ref as F
from test_blas1_ref_host import add, cvec, div, mul, sub, vec

NDOT = [1, 63, 64, 65, 255, 256, 257, 1000, 4096]          # the list lengths of the GPU cells
NN2 = [1, 2, 255, 256, 257]
VARIANTS = [(form, have_u) for form in (0, 1, 2) for have_u in (False, True)]


def elem(form, have_u, t, c, p, ar, ai, bc, bp):
    """one element of fold_elem<form, have_u> in exact arithmetic, one rounding per operation -> (re, im)"""
    wx, wy, vx, vy = div(t.real, bc), div(t.imag, bc), div(c.real, bc), div(c.imag, bc)
    ux, uy = (div(p.real, bp), div(p.imag, bp)) if have_u else (None, None)
    if form == 0:
        if have_u:
            return sub(wx, add(mul(ar, vx), mul(bc, ux))), sub(wy, add(mul(ar, vy), mul(bc, uy)))
        return sub(wx, mul(ar, vx)), sub(wy, mul(ar, vy))
    if form == 1:
        rx, ry = sub(wx, mul(ar, vx)), sub(wy, mul(ar, vy))
    else:
        rx, ry = sub(wx, sub(mul(ar, vx), mul(ai, vy))), sub(wy, add(mul(ar, vy), mul(ai, vx)))
    if have_u:
        rx, ry = sub(rx, mul(bc, ux)), sub(ry, mul(bc, uy))
    return rx, ry


@pytest.mark.parametrize("form,have_u", VARIANTS)
def test_fold_elem_rounds_once_per_operation_in_the_order_of_its_form(form, have_u):
    rng = np.random.default_rng(10 * form + have_u)
    n = 200
    t, c, p = cvec(rng, n), cvec(rng, n), cvec(rng, n)
    for ar, ai, bc, bp in ((1.7, -0.31, 1.37, 0.83), (-0.123, 0.77, 1.0, 1.0), (0.9, 0.2, 13.1, 1.0)):
        got = F.fold_elem(form, t, c, p if have_u else None, ar, ai, bc, bp)
        for i in range(n):
            want = elem(form, have_u, complex(t[i]), complex(c[i]), complex(p[i]), ar, ai, bc, bp)
            assert (float(got[i].real), float(got[i].imag)) == want, (form, have_u, i)
    if form != 2:                                                           # a complex alpha's imaginary part is form 2's alone
        assert np.array_equal(F.fold_elem(form, t, c, p if have_u else None, 1.7, 0.5, 1.37, 0.83),
                              F.fold_elem(form, t, c, p if have_u else None, 1.7, 0.0, 1.37, 0.83))
    if not have_u:                                                          # without u neither beta nor b_p enters
        assert np.array_equal(F.fold_elem(form, t, c, None, 1.7, 0.5, 1.37, 0.83), F.fold_elem(form, t, c, None, 1.7, 0.5, 1.37, 7.0))


def test_alpha_is_a_true_division_with_the_imaginary_part_in_form_2_alone():
    rng = np.random.default_rng(3)
    for _ in range(200):
        d0, d1, nc = float(rng.standard_normal()), float(rng.standard_normal()), float(rng.uniform(0.1, 1e6))
        for form in (0, 1, 2):
            assert F.alpha(form, (d0, d1), nc) == (div(d0, nc), div(d1, nc) if form == 2 else 0.0)
            assert F.alpha(form, (d0, d1)) == (d0, d1 if form == 2 else 0.0)             # a null n2c: nc = 1.0
    ar, ai = F.alpha(2, (1.0, -2.0), 0.0)                                    # a column that broke down: IEEE, no exception
    assert ar == np.inf and ai == -np.inf


def exact_block_reduce(lanes):
    for w in range(4):
        off = 32
        while off:
            for lane in range(off):
                lanes[64 * w + lane] = add(lanes[64 * w + lane], lanes[64 * w + lane + off])
            off >>= 1
    s = 0.0
    for w in range(4):
        s = add(s, lanes[64 * w])
    return s


@pytest.mark.parametrize("n", sorted(set(NDOT + NN2)))
def test_sum_list256_is_the_thread_strided_sum_then_four_wave_trees_then_the_waves_in_order(n):
    lst = F.dot_list(n, 5) * 10.0 ** np.random.default_rng(n).integers(-3, 4, 2 * n)     # a spread of exponents as well
    for x in (lst, F.dot_list(n, 5)):
        for comp in (0, 1):
            lanes = [0.0] * 256
            for i in range(n):                                              # thread i % 256 meets its entries in ascending order
                lanes[i % 256] = add(lanes[i % 256], float(x[2 * i + comp]))
            assert F.sum_list256(x, n, comp) == exact_block_reduce(lanes), (n, comp)
    poisoned = np.concatenate([lst, np.full(6, np.nan)])                    # the other component and what lies past n are not read
    poisoned[1::2] = np.nan
    assert F.sum_list256(poisoned, n, 0) == F.sum_list256(lst, n, 0)


@pytest.mark.parametrize("N,nb", [(1, 1), (3, 1), (255, 1), (256, 1), (257, 1), (257, 2), (1025, 1), (1025, 3), (1300, 2)])
def test_fold_p_partials_are_the_grid_strided_sums_then_the_block_reduction(N, nb):
    rng = np.random.default_rng(N + nb)
    r = cvec(rng, N)
    got = F.fold_p_partials(np.concatenate([r, np.full(3, np.nan + 0j)]), N, nb)         # what lies past N is not read
    assert got.shape == (nb,)
    for b in range(nb):
        lanes = [0.0] * 256
        for th in range(256):
            for i in range(b * 256 + th, N, nb * 256):
                x, y = float(r[i].real), float(r[i].imag)
                lanes[th] = add(lanes[th], add(mul(x, x), mul(y, y)))
        assert float(got[b]) == exact_block_reduce(lanes), (N, nb, b)
    terms = F.norm_terms(r)
    assert all(float(terms[i]) == add(mul(float(r[i].real), float(r[i].real)), mul(float(r[i].imag), float(r[i].imag))) for i in range(N))


@pytest.mark.parametrize("balanced", [False, True])
@pytest.mark.parametrize("N", [1, 2, 3, 255, 256, 257, 1025, 2047, 2048, 2049, 4097, 524_293])
def test_the_gpu_inputs_tell_form_0_from_form_1(N, balanced):
    """w - (a v + b u) against (w - a v) - b u on the vectors and scalars of the GPU cells, in both of their regimes (np.sqrt
    stands in for the device's here): a launcher whose switch swapped the two cases is seen by every cell with a u from N = 255
    on (below that the two roundings may coincide on all 2 N components: printed)."""
    t, uc, up = F.vectors(N, 1)
    n2c, n2p = F.norms(N, balanced)
    ar, bc, bp = F.alpha(0, F.DOT, n2c)[0], float(np.sqrt(n2c)), float(np.sqrt(n2p))
    r0, r1 = (F.fold_elem(form, t, uc, up, ar, 0.0, bc, bp) for form in (0, 1))
    differ = int((r0.real != r1.real).sum() + (r0.imag != r1.imag).sum())
    print(f"N={N} balanced={balanced}: forms 0 and 1 differ in {differ} of {2 * N} components")
    assert differ > 0 or N < 255
    assert np.array_equal(F.fold_elem(0, t, uc, None, ar, 0.0, bc, bp), F.fold_elem(1, t, uc, None, ar, 0.0, bc, bp))


@pytest.mark.parametrize("n", [n for n in sorted(set(NDOT + NN2)) if n >= 63])
def test_the_gpu_lists_tell_the_block_order_from_other_orders(n):
    """On the lists of the GPU cells (seeds 0..5 of each length) the block's order gives other bits than a left-to-right sum and
    than the same trees with the four waves added in reverse (lengths above 64; one wave has nothing to reverse)."""
    plain = waves = 0
    for seed in range(6):
        for lst, comp in ((F.dot_list(n, seed), 0), (F.dot_list(n, seed), 1), (F.n2_list(n, seed, 3.0 * n), 0)):
            x = lst[comp::2]
            got = F.sum_list256(lst, n, comp)
            s = 0.0
            for v in x.tolist():
                s = s + v
            plain += got != s
            lanes = np.zeros(256)
            for lo in range(0, n, 256):
                lanes[:len(x[lo:lo + 256])] += x[lo:lo + 256]
            w = lanes.reshape(4, 64).copy()
            off = 32
            while off:
                w[:, :off] = w[:, :off] + w[:, off:2 * off]
                off >>= 1
            waves += got != (((0.0 + w[3, 0]) + w[2, 0]) + w[1, 0]) + w[0, 0]
    print(f"n={n}: of 18 sums {plain} differ from left to right, {waves} from the waves in reverse")
    assert plain > 0
    assert waves > 0 or n <= 128
