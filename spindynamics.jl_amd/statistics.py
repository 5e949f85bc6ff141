"""S^z-basis statistics of one state: what reads the probability distribution |psi_s|^2 over the S^z configurations
rather than an operator expectation -- participation entropies, the full counting statistics of a subsystem's magnetisation with the
number entropy, and projective snapshots.  Each is one streaming pass of a kernel of its own over psi.
psi may be a numpy array (host) or a torch CUDA tensor (stays on the device).  Sites are 1-based, site i is bit i - 1 of a
configuration.  The library divides nothing by <psi|psi>; the functions here normalise."""
import ctypes as C
import math

import numpy as np

from ._lib import ArgumentError, check, lib
from .hamiltonian import _bind_torch_stream, _dtype_code, _is_torch

_dp = C.POINTER(C.c_double)
_u64p = C.POINTER(C.c_uint64)
_i64p = C.POINTER(C.c_int64)
MOMENT_MAX_Q = 8          # SD_MOMENT_MAX_Q
COUNT_MAX_MASKS = 256     # SD_COUNT_MAX_MASKS


def _call(name, psi, model, *args):
    """sd_<name>[_dev](ctx, model, dtype, psi, n, *args)"""
    if _is_torch(psi):
        _bind_torch_stream(model, psi)
        check(getattr(lib(), name + "_dev")(model.ctx.h, model.h, _dtype_code(psi), psi.data_ptr(), len(psi), *args), model.ctx.h)
    else:
        x = np.ascontiguousarray(psi)
        if x.dtype not in (np.float64, np.complex128):
            x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
        check(getattr(lib(), name)(model.ctx.h, model.h, _dtype_code(x), x.ctypes.data, len(x), *args), model.ctx.h)


def _moments(psi, model, qs):
    """(sum w, sum w ln w, max w, argmax row, [sum w^q for q in qs]) -- one kernel pass per MOMENT_MAX_Q exponents"""
    qs = [float(q) for q in qs]
    head, sums = None, []
    for k in range(0, max(len(qs), 1), MOMENT_MAX_Q):
        part = np.asarray(qs[k:k + MOMENT_MAX_Q], dtype=np.float64)
        out = np.empty(5 + len(part))
        _call("sd_basis_moments", psi, model, part.ctypes.data_as(_dp), len(part), out.ctypes.data_as(_dp))
        head = out[:4] if head is None else head
        sums += out[5:].tolist()
    return float(head[0]), float(head[1]), float(head[2]), int(head[3]), sums


def participation_entropy(psi, model, q=2):
    """The participation entropies S_q of |psi_s|^2 / <psi|psi> over the S^z configurations, the standard localisation diagnostics:
      S_q = ln(sum_s p_s^q) / (1 - q);   q = 1: the Shannon entropy -sum p ln p;   q = math.inf: -ln max_s p_s.
    q: a positive scalar -> a float, or a sequence -> a float64 array.  A basis state has S_q = 0, the uniform state S_q = ln N.
    One kernel pass for the whole list (in chunks of 8 exponents)."""
    scalar = np.ndim(q) == 0
    qs = [float(x) for x in np.atleast_1d(np.asarray(q, dtype=np.float64))]
    for x in qs:
        if not x > 0.0:
            raise ArgumentError(f"participation_entropy: q must be positive, got {x}")
    general = [x for x in qs if x != 1.0 and math.isfinite(x)]
    W, wlnw, wmax, _row, sums = _moments(psi, model, general)
    if not W > 0.0:
        raise ArgumentError("participation_entropy: the state has zero norm")
    by_q = dict(zip(general, sums))
    out = []
    for x in qs:
        if x == 1.0:
            out.append(math.log(W) - wlnw / W)
        elif math.isinf(x):
            out.append(-math.log(wmax / W))
        else:
            out.append(math.log(by_q[x] / W ** x) / (1.0 - x))
    return out[0] if scalar else np.array(out)


def inverse_participation_ratio(psi, model):
    """sum_s p_s^2 with p = |psi_s|^2 / <psi|psi>: 1 for a basis state, 1/N for the uniform state"""
    W, _wlnw, _wmax, _row, sums = _moments(psi, model, [2.0])
    if not W > 0.0:
        raise ArgumentError("inverse_participation_ratio: the state has zero norm")
    return sums[0] / (W * W)


def most_probable_configuration(psi, model):
    """(configuration, row, probability) of the most probable S^z configuration; ties go to the lowest row"""
    W, _wlnw, wmax, row, _ = _moments(psi, model, [])
    if not W > 0.0:
        raise ArgumentError("most_probable_configuration: the state has zero norm")
    return int(model.states_range(row, 1)[0]), row, wmax / W


def _site_mask(model, sites, what):
    mask = 0
    for s in sites:
        i = int(s)
        if i != s or i < 1 or i > model.L:
            raise ArgumentError(f"{what}: site {s} is outside 1..{model.L}")
        if (mask >> (i - 1)) & 1:
            raise ArgumentError(f"{what}: site {i} is repeated")
        mask |= 1 << (i - 1)
    return mask


def counting_statistics(psi, model, subsystems, normalize=True):
    """Full counting statistics: P[k, m] = the probability that subsystem k -- `subsystems[k]`, a list of 1-based sites -- holds m up
    spins, m = 0..L, i.e. the distribution of its magnetisation sum_{i in A} S^z_i = m - |A|/2.  -> a (K, L + 1) float64 array; the
    bins no configuration of the basis reaches are exact zeros.  normalize=False: the raw sums of |psi_s|^2.  All subsystems in one
    pass over psi (lists longer than 256 in several).  In the full basis a subsystem may hold at most 32 sites."""
    masks = [_site_mask(model, A, "counting_statistics") for A in subsystems]
    if not masks:
        raise ArgumentError("counting_statistics: no subsystem given")
    lo, nb = C.c_int(), C.c_int()
    for mk in masks:                                          # refused before any launch
        check(lib().sd_counting_range(model.h, mk, C.byref(lo), C.byref(nb)))
        if nb.value > 33:
            raise ArgumentError("counting_statistics: a subsystem of the full basis may hold at most 32 sites")
    P = np.empty((len(masks), model.L + 1))
    for k in range(0, len(masks), COUNT_MAX_MASKS):
        part = np.asarray(masks[k:k + COUNT_MAX_MASKS], dtype=np.uint64)
        out = np.empty((len(part), model.L + 1))
        _call("sd_counting_statistics", psi, model, part.ctypes.data_as(_u64p), len(part), out.ctypes.data_as(_dp))
        P[k:k + len(part)] = out
    if normalize:
        W = P[0].sum()                                        # every row sums to <psi|psi>
        if not W > 0.0:
            raise ArgumentError("counting_statistics: the state has zero norm")
        P /= W
    return P


def cut_counting_statistics(psi, model):
    """counting_statistics of the L - 1 cuts {1..k}, k = 1..L-1, in one call: row k - 1 is the distribution of the number of up spins
    left of the bond (k, k + 1)"""
    if model.L < 2:
        raise ArgumentError("cut_counting_statistics: the chain has no cut")
    return counting_statistics(psi, model, [range(1, k + 1) for k in range(1, model.L)])


def number_entropy(psi, model, subsystem):
    """S_N = -sum_m p_m ln p_m of the subsystem's counting statistics: the part of the entanglement entropy that needs no reduced
    density matrix"""
    p = counting_statistics(psi, model, [subsystem])[0]
    p = p[p > 0.0]
    return float(-(p * np.log(p)).sum()) + 0.0             # (a basis state: 0.0, not -0.0)


def magnetization_cumulants(P, sites, order=4):
    """Cumulants kappa_1..kappa_order of sum_{i in A} S^z_i = m - |A|/2 under the distribution P[m] (one row of counting_statistics;
    normalised here), |A| = `sites` (a count or a site list): the mean, the variance, then the higher cumulants from the central moments
    (kappa_3 = mu_3, kappa_4 = mu_4 - 3 mu_2^2, in general kappa_n = mu_n - sum_{k=2}^{n-2} C(n-1, k-1) kappa_k mu_{n-k}).  Host
    arithmetic."""
    P = np.asarray(P, dtype=np.float64)
    if P.ndim != 1 or order < 1:
        raise ArgumentError("magnetization_cumulants: P must be one distribution and order >= 1")
    nA = int(sites) if np.ndim(sites) == 0 else len(sites)
    W = P.sum()
    if not W > 0.0:
        raise ArgumentError("magnetization_cumulants: the distribution sums to zero")
    p = P / W
    x = np.arange(len(P)) - 0.5 * nA
    mean = float((p * x).sum())
    mu = [1.0, 0.0] + [float((p * (x - mean) ** n).sum()) for n in range(2, order + 1)]
    kappa = [0.0, mean]
    for n in range(2, order + 1):
        kappa.append(mu[n] - sum(math.comb(n - 1, k - 1) * kappa[k] * mu[n - k] for k in range(2, n - 1)))
    return np.array(kappa[1:order + 1])


def sample_configurations(psi, model, shots, seed=0, return_rows=False):
    """Projective snapshots: `shots` configurations drawn independently from |psi_s|^2 / <psi|psi>, what a quantum-gas microscope
    returns -> a uint64 array (with return_rows=True also the int64 rows).  The result is a function of (psi, seed, shots) alone --
    not of the device plan -- and shot k of a call is shot k of any longer call with the same seed."""
    if int(shots) != shots or shots < 0:
        raise ArgumentError("sample_configurations: shots must be a non-negative integer")
    if int(seed) != seed or not 0 <= seed < 2 ** 64:
        raise ArgumentError("sample_configurations: seed must be an integer in 0..2^64-1")
    shots = int(shots)
    rows = np.empty(shots, dtype=np.int64)
    cfg = np.empty(shots, dtype=np.uint64)
    _call("sd_sample_configurations", psi, model, shots, int(seed), rows.ctypes.data_as(_i64p), cfg.ctypes.data_as(_u64p))
    return (cfg, rows) if return_rows else cfg


def snapshot_spins(configs, L):
    """configurations -> a (shots, L) array of +-1/2, column i - 1 the spin of site i"""
    c = np.asarray(configs, dtype=np.uint64).reshape(-1)
    bits = (c[:, None] >> np.arange(L, dtype=np.uint64)[None, :]) & np.uint64(1)
    return bits.astype(np.float64) - 0.5
