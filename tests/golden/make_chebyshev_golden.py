"""Regenerates tests/golden/chebyshev/real_coeffs_exact.npz: the Bessel functions J_k(z) behind the real-time Chebyshev
coefficients c_k = (2 - delta_k0) (-i)^k J_k(a dt) exp(-i b dt), evaluated with 70 digits and rounded once to Float64, and the
exact term count n_used(z) = the first k with k > z and |J_k(z)| < 2^-53.  Needs mpmath; the tests read only the npz.

    python tests/golden/make_chebyshev_golden.py

All k at once by Miller's backward recurrence f_{k-1} = (2k/z) f_k - f_{k+1} from f_{ktop+1} = 0, f_{ktop} = 1, normalised by
J_0 + 2 sum_{k>=1} J_2k = 1.  The start ktop lies so far into the Airy tail that J_ktop < 1e-90 J_z: the start's error is that
ratio squared.  In the oscillatory range k < z the recurrence is neutrally stable, rounding errors grow at most linearly in the
number of steps: 1e6 steps at 70 digits leave more than 60.  Every z <= 1100 is checked against mpmath's own besselj.

The file holds, per z (index i in the array "z"): "k<i>" (int32) and "J<i>" (Float64) of equal length, and "n_used"[i].
FULL z: k = 0 .. n_used + 8.  SAMPLED z: every k from floor(z) - 64 to n_used + 8, and a stride through the k below, 1200 in all.
"""
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 70

FULL = [0.5, 2.16, 30.0, 100.0, 400.0, 999.0, 1000.0, 1000.5, 1100.0]
SAMPLED = [5000.0, 2e4, 1e5, 1e6]
MAX_SAMPLED = 1200
MAX_BYTES = 112110            # the largest golden committed before this one
TWO53 = mp.mpf(2) ** -53


def bessel_j_all(z):
    """[J_0(z), ..., J_ktop(z)] as mpf, z > 0 a Float64 taken exactly"""
    zm = mp.mpf(z)
    ktop = int(z) + 256 + int(40 * z ** (1.0 / 3.0))
    f = [mp.mpf(0)] * (ktop + 2)
    f[ktop] = mp.mpf(1)
    for k in range(ktop, 0, -1):
        f[k - 1] = (2 * k) * f[k] / zm - f[k + 1]
    s = f[0] + 2 * mp.fsum(f[2:ktop + 1:2])
    return [x / s for x in f[:ktop + 1]]


def n_used_of(z, J):
    k = int(np.floor(z)) + 1
    while not abs(J[k]) < TWO53:
        k += 1
    # the rule must not hang on the last digit of any implementation that is good to 1e-6 of 2^-53
    for j in range(int(np.floor(z)) + 1, k + 9):
        assert abs(abs(J[j]) / TWO53 - 1) > 1e-6, (z, j)
    return k


def main():
    out = {"z": np.array(FULL + SAMPLED)}
    n_used = []
    for i, z in enumerate(FULL + SAMPLED):
        J = bessel_j_all(z)
        nu = n_used_of(z, J)
        assert nu + 8 < len(J) and abs(J[-1]) < mp.mpf(10) ** -80
        if z <= 1100:
            ks = sorted(set(range(0, nu + 9, 7)) | set(range(max(0, int(z) - 20), nu + 9)))
            worst = max(abs(J[k] - mp.besselj(k, mp.mpf(z))) for k in ks)
            assert worst < mp.mpf(10) ** -60, (z, worst)
            print(f"z={z:g}: n_used={nu}, worst deviation from mp.besselj {mp.nstr(worst, 3)} over {len(ks)} orders")
        # the second sum rule, J_0^2 + 2 sum J_k^2 = 1, is independent of the normalisation used
        defect = abs(J[0] ** 2 + 2 * mp.fsum(x * x for x in J[1:]) - 1)
        assert defect < mp.mpf(10) ** -60, (z, defect)
        if z in FULL:
            k = np.arange(nu + 9)
        else:
            tail = np.arange(int(z) - 64, nu + 9)
            assert len(tail) < MAX_SAMPLED
            k = np.concatenate([np.linspace(0, int(z) - 65, MAX_SAMPLED - len(tail)).astype(np.int64), tail])
            assert len(np.unique(k)) == len(k) == MAX_SAMPLED
            print(f"z={z:g}: n_used={nu}, sum-rule defect {mp.nstr(defect, 3)}, {len(k)} orders kept")
        out[f"k{i}"] = k.astype(np.int32)
        out[f"J{i}"] = np.array([float(J[j]) for j in k])
        n_used.append(nu)
    out["n_used"] = np.array(n_used, dtype=np.int64)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "chebyshev", "real_coeffs_exact.npz")
    os.makedirs(os.path.dirname(path), exist_ok=True)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < MAX_BYTES, size
    print(f"{path}: {size} bytes")


if __name__ == "__main__":
    main()
