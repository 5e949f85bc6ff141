"""Times the operator-string kernels against the dedicated kernels that compute the same operators.  A record, not
a gate: the dedicated kernels stay, the general one is expected to be slower, and this says by how much.

XXZ ring, ComplexF64, half filling.  Device events around each call, warm-up first, median of --reps runs.  Per size one JSON line:
  the model's energy-current list through energy_current (sd_dcurrent_apply_dev) and as strings through operator_apply;
  one bond through bond_operator and as three strings;
  hamiltonian_terms through operator_apply, and one plain apply (sd_bench_apply_dev);
  K = 26 chirality expectations (the L - 2 consecutive triples of the chain) in one operator_expectations pass.
The string calls include the upload of their tables and the stream synchronisation that returns them to the pool.

    python profiles/opstring_bench.py --L 28
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as g  # noqa: E402

from pair_correlations_bench import timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, nargs="+", default=[28])
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    import torch
    pkg = g.load_package()
    for L in a.L:
        nup = L // 2
        m = pkg.XXZChain(L, Jxy=1.0, Jz=1.0, nup=nup, boundary="periodic")
        dev = torch.device("cuda", m.ctx.device)
        psi = torch.empty(m.N, dtype=torch.complex128, device=dev)
        out = torch.empty_like(psi)
        m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)
        ms = C.c_float(0.0)
        applies = []
        for r in range(a.reps + 1):
            pkg.check(pkg.lib().sd_bench_apply_dev(m.ctx.h, m.h, 2, psi.data_ptr(), out.data_ptr(), m.N, 4, C.byref(ms)), m.ctx.h)
            if r:
                applies.append(ms.value)
        pkg.check(pkg.lib().sd_fill_randn_dev(m.ctx.h, psi.data_ptr(), 2 * m.N, 7, 0), m.ctx.h)   # the ping-pong overwrote psi
        apply_ms = statistics.median(applies)

        dterms = pkg.energy_current_terms(m, "periodic")
        fwd, bwd = [], []
        for t in dterms:
            i, j, k, c = int(t["i"]), int(t["j"]), int(t["k"]), float(t["c"])
            z = 1 << (k - 1) if k else 0
            fwd.append(pkg.Term(1 << (i - 1), 1 << (j - 1), z, complex(0.0, c), 0))
            bwd.append(pkg.Term(1 << (j - 1), 1 << (i - 1), z, complex(0.0, -c), 0))
        ec_strings = pkg.pack_terms(sorted(fwd + bwd, key=lambda t: (t.plus, t.minus)))
        ec_ded = timed(lambda: pkg.check(pkg.lib().sd_dcurrent_apply_dev(m.ctx.h, m.h, 2, psi.data_ptr(), m.N, dterms.ctypes.data,
                                                                         len(dterms), out.data_ptr()), m.ctx.h), a.reps)
        ec_str = timed(lambda: pkg.operator_apply(psi, m, ec_strings, out=out), a.reps)

        bond = pkg.pack_terms(pkg.op_string(1.0, ("z", 3), ("z", 4)) + pkg.op_string(0.5, ("+", 3), ("-", 4))
                              + pkg.op_string(0.5, ("-", 3), ("+", 4)))
        bond_ded = timed(lambda: pkg.bond_operator(psi, m, 3, 4, out=out), a.reps)
        bond_str = timed(lambda: pkg.operator_apply(psi, m, bond, out=out), a.reps)

        hterms = pkg.pack_terms(pkg.hamiltonian_terms(m))
        h_str = timed(lambda: pkg.operator_apply(psi, m, hterms, out=out), a.reps)

        triples = [(i, i + 1, i + 2) for i in range(1, L - 1)]
        chi = []
        for n, t in enumerate(triples):
            chi += pkg.chirality_terms(*t, op=n)
        chi = pkg.pack_terms(chi)
        chi_ms = timed(lambda: pkg.operator_expectations(psi, m, chi), a.reps)

        rec = {"L": L, "nup": nup, "N": m.N, "path": m.device_path, "apply_ms": apply_ms,
               "ecurrent_terms": len(dterms), "ecurrent_dedicated_ms": ec_ded[0], "ecurrent_strings_ms": ec_str[0],
               "ecurrent_strings_over_dedicated": ec_str[0] / ec_ded[0],
               "bond_dedicated_ms": bond_ded[0], "bond_strings_ms": bond_str[0], "bond_strings_over_dedicated": bond_str[0] / bond_ded[0],
               "hamiltonian_terms": len(hterms), "hamiltonian_strings_ms": h_str[0], "hamiltonian_strings_over_apply": h_str[0] / apply_ms,
               "chirality_ops": len(triples), "chirality_terms": len(chi), "chirality_expect_ms": chi_ms[0],
               "chirality_expect_in_applies": chi_ms[0] / apply_ms,
               "min_max": {"ecurrent_dedicated": ec_ded[1:], "ecurrent_strings": ec_str[1:], "bond_dedicated": bond_ded[1:],
                           "bond_strings": bond_str[1:], "hamiltonian_strings": h_str[1:], "chirality_expect": chi_ms[1:]}}
        print(json.dumps(rec), flush=True)
        del psi, out
        torch.cuda.empty_cache()
        m.ctx.release_scratch()


if __name__ == "__main__":
    main()
