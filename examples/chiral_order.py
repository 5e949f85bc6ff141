#!/usr/bin/env python3
"""Scalar chirality of a J1-J2 ring with a chiral three-spin term,

    H = J1 sum_i S_i . S_i+1 + J2 sum_i S_i . S_i+2 + J_chi sum_i S_i . (S_i+1 x S_i+2)          (sites mod L),

built from operator strings: the model holds the J1-J2 part, `operator_hamiltonian` adds the chiral term to it (no new kernel, no
work vector).  For J_chi = 0 and for J_chi != 0 it prints E0, the chirality per triangle <chi_i> = <S_i . (S_i+1 x S_i+2)> and the
chirality correlations <chi_1 chi_b> of the triangles that share no site with the first.  A real ground state (J_chi = 0) has no
chirality; the chiral term breaks time reversal and, once it is strong enough to bring the chiral level down (J_chi of about J1 at
L = 12), orders every triangle alike.  L = 12 by default, a few seconds
(python examples/chiral_order.py 16)."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import __graft_entry__ as g

sd = g.load_package()
L = int(sys.argv[1]) if len(sys.argv) > 1 else 12
J1, J2 = 1.0, 0.3
site = lambda i: (i - 1) % L + 1                  # noqa: E731
hop = [(i, site(i + 1), J1 / 2) for i in range(1, L + 1)] + [(i, site(i + 2), J2 / 2) for i in range(1, L + 1)]
zz = [(i, site(i + 1), J1) for i in range(1, L + 1)] + [(i, site(i + 2), J2) for i in range(1, L + 1)]
model = sd.build_model(L, nup=L // 2, hopping=hop, zz=zz, onsite_field=np.zeros(L))
triples = [(i, site(i + 1), site(i + 2)) for i in range(1, L + 1)]
far = [b for b in range(1, L) if not set(triples[0]) & set(triples[b])]

for Jchi in (0.0, 1.5):
    terms = []
    for t in triples:
        terms += sd.chirality_terms(*t, coeff=Jchi)
    terms = sd.operator_simplify(terms)
    assert sd.operator_is_hermitian(terms)
    t0 = time.time()
    E0, psi = sd.operator_groundstate(model, terms)
    t1 = time.time()
    chi = sd.scalar_chirality(psi, model, triples)
    corr = sd.chirality_correlations(psi, model, triples, pairs=[(0, b) for b in far])
    print("J_chi = %.1f: dimension %d, %d string terms, E0 = %.10f (%.2f s), chirality and correlations in %.3f s"
          % (Jchi, len(model), len(terms), E0, t1 - t0, time.time() - t1))
    print("   chirality per triangle: " + " ".join("%.6f" % x for x in chi))
    print("   <chi_1 chi_b>, b = %s: " % ",".join(str(b + 1) for b in far) + " ".join("%.6f" % corr[0, b] for b in far))
