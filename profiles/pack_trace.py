#!/usr/bin/env python3
"""Which clock do the eight XCD queues of the packed ComplexF64 launch follow?  (profiles/ablation_queue_clock.md)

Needs a library built with -DSD_PACK_TRACE=1 (bash profiles/build_variant.sh <name> -DSD_PACK_TRACE=1 [-DSD_ORBIT_...]), loaded
through SD_LIB_PATH: in that build lane 0 of wave 0 of every block of k_apply_tiled<.., PACK> stores the 100 MHz wall clock at
entry and after its last store, and the XCC id it ran on.  A plain run: no profiler, no counters.

  python profiles/pack_trace.py run OUTDIR [L ...]     (GPU) per size (default 28 32) one child process under its own time
                                                       limit: three warm applies, one traced apply -> OUTDIR/trace_L<L>.npz
  python profiles/pack_trace.py eval FILE.npz [quad_blocks cap_tenths]      (CPU only) -> one JSON line:
    (a) share of blocks i that ran on XCD i % 8 (and on the XCD most blocks of their residue ran on);
    (b) drift: at 400 instants of the launch, the queue position of the newest block started on each XCD, max - min over the
        XCDs, in blocks; and the same for the place in the orbit sequence (the orbit of that block's first tile, numbered as
        the planner numbers them), in orbits and converted to blocks of one queue;
    (c) per queue, windows of 1 000 blocks: least squares of the elapsed time (start of the window to start of the next) on the
        host-computable costs of its blocks -- rows, slots, requested bytes, out-of-orbit bytes (profiles/orbit_key.py,
        csrc/xcd_deal.hpp) -- through the origin, all queues together: relative rms residual for each cost alone and for every
        pair, with the coefficients (the ratio of a pair's coefficients is the mix to deal by).
"""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TICK_US = 0.01            # wall_clock64: 100 MHz


def child(L, out):
    import ctypes as C
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    _lib = sys.modules[pkg.__name__ + "._lib"]          # the package's ctypes binding and the library it loaded
    lib = _lib.lib()
    if not hasattr(lib, "sd_pack_trace_read"):
        raise SystemExit("pack_trace.py: %s is no trace build (-DSD_PACK_TRACE=1)" % _lib.LIB_PATH)
    m = pkg.XXZChain(L, nup=L // 2)
    a = torch.empty(m.N, dtype=torch.complex128, device="cuda")
    a.real.normal_()
    a.imag.normal_()
    b = torch.empty_like(a)
    for _ in range(4):                       # three warm applies and the traced one: every launch overwrites the records
        pkg.apply_H(b, a, m)
    torch.cuda.synchronize()
    fn = lib.sd_pack_trace_read
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    nb = fn(m.h, None, None, None)
    if nb <= 0:
        raise SystemExit("pack_trace.py: the plan of L=%d has no packed launch" % L)
    rec = np.zeros((nb, 3), dtype=np.uint64)
    slot = np.zeros((nb, 4), dtype=np.uint32)
    qn = np.zeros(8, dtype=np.int64)
    assert fn(m.h, rec.ctypes.data, slot.ctypes.data, qn.ctypes.data) == nb
    np.savez_compressed(out, rec=rec, slot_prefix=slot, q_blocks=qn, L=L, nup=L // 2, LS=12, lib=os.path.basename(_lib.LIB_PATH))
    dur = (int(rec[:, 1].max()) - int(rec[:, 0].min())) * TICK_US
    print("L=%d: %d blocks, launch %.1f us, records -> %s" % (L, nb, dur, out), flush=True)


def run(outdir, sizes):
    os.makedirs(outdir, exist_ok=True)
    for L in sizes:
        out = os.path.join(outdir, "trace_L%d.npz" % L)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "child", str(L), out], timeout=60 + (90 if L >= 32 else 30))
        except subprocess.TimeoutExpired:
            raise SystemExit("pack_trace.py: L=%d ran into its time limit; nothing more is started" % L)
        if r.returncode != 0:
            raise SystemExit("pack_trace.py: L=%d ended with status %d; nothing more is started" % (L, r.returncode))


def evaluate(path, quad_blocks=2, cap_tenths=78):
    import numpy as np
    sys.path.insert(0, HERE)
    from orbit_key import orbit_key, tile_costs
    z = np.load(path)
    rec, slot, qn = z["rec"].astype(np.int64), z["slot_prefix"], z["q_blocks"]
    L, nup, LS = int(z["L"]), int(z["nup"]), int(z["LS"])
    p, nb = L - LS, rec.shape[0]
    t0, t1, xcc = rec[:, 0] - rec[:, 0].min(), rec[:, 1] - rec[:, 0].min(), rec[:, 2]
    # queue and position of every block: block j of queue x follows block j of queue x - 1, queues that have run out are skipped
    queue, pos = np.empty(nb, dtype=np.int64), np.empty(nb, dtype=np.int64)
    i = 0
    for j in range(int(qn.max())):
        for x in range(8):
            if j < qn[x]:
                queue[i], pos[i] = x, j
                i += 1
    assert i == nb
    res = {"file": os.path.basename(path), "lib": str(z["lib"]), "L": L, "blocks": nb, "queue_blocks_max_minus_min": int(qn.max() - qn.min()),
           "launch_us": round(float(t1.max()) * TICK_US, 1), "block_life_us_median": round(float(np.median(t1 - t0)) * TICK_US, 2)}
    # (a)
    resid = np.arange(nb) % 8
    res["a_share_on_xcd_i_mod_8"] = round(float((xcc == resid).mean()), 4)
    perm = [int(np.bincount(xcc[resid == r], minlength=16).argmax()) for r in range(8)]
    res["a_most_common_xcd_of_residue"] = perm
    res["a_share_on_most_common_xcd"] = round(float((xcc == np.array(perm)[resid]).mean()), 4)
    # (b) by the XCD the block ran on: position (in its queue) of the newest block started
    T = np.linspace(0.0, float(t0.max()), 402)[1:-1]
    newest = []
    for x in sorted(set(xcc.tolist())):
        sel = np.where(xcc == x)[0]
        order = sel[np.argsort(t0[sel], kind="stable")]
        k = np.searchsorted(t0[order], T, side="right") - 1
        newest.append(np.where(k >= 0, pos[order][np.maximum(k, 0)], 0))
    newest = np.array(newest)
    drift = newest.max(axis=0) - newest.min(axis=0)
    mid = drift[20:-20]
    res["b_drift_blocks"] = {"mean": round(float(drift.mean()), 1), "median": float(np.median(drift)), "worst": int(drift.max()),
                             "mean_middle_90pc": round(float(mid.mean()), 1), "worst_middle_90pc": int(mid.max()),
                             "at_25_50_75_pc_of_the_launch": [int(drift[100]), int(drift[200]), int(drift[300])]}
    # (c) costs per block: a tile counts once, at the first slot of its team
    cache, rep_of = {}, {}
    cost = np.zeros((nb, 4))
    first_tile = np.zeros(nb, dtype=np.int64)
    for bi in range(nb):
        prev = 0xFFFFFFFF
        for P in slot[bi].tolist():
            if P != 0xFFFFFFFF and P != prev:
                c = cache.get(P)
                if c is None:
                    c = cache[P] = tile_costs(P, p, LS, nup, quad_blocks, cap_tenths)
                    rep_of[P] = orbit_key(P, p, quad_blocks, cap_tenths)[0]
                cost[bi] += c
                if prev == 0xFFFFFFFF:
                    first_tile[bi] = P
            prev = P
    # (b) again, in the orbit sequence: orbits numbered by first appearance among the tiles in ascending base row (site 1 most
    # significant, up first), as sd_build_plan hands them to xcd_queues
    tiles = np.array(sorted(cache), dtype=np.int64)
    key = np.zeros(len(tiles), dtype=np.int64)
    for k in range(1, p + 1):
        key |= (1 - ((tiles >> (k - 1)) & 1)) << (p - k)
    first_key = {}
    for P, kk in zip(tiles.tolist(), key.tolist()):
        r = rep_of[P]
        if r not in first_key or kk < first_key[r]:
            first_key[r] = kk
    rank = {r: n for n, r in enumerate(sorted(first_key, key=first_key.get))}
    seq = np.array([rank[rep_of[P]] for P in first_tile.tolist()], dtype=np.int64)
    newest = []
    for x in sorted(set(xcc.tolist())):
        sel = np.where(xcc == x)[0]
        order = sel[np.argsort(t0[sel], kind="stable")]
        k = np.searchsorted(t0[order], T, side="right") - 1
        newest.append(np.where(k >= 0, seq[order][np.maximum(k, 0)], 0))
    newest = np.array(newest)
    dseq = (newest.max(axis=0) - newest.min(axis=0))[20:-20]
    per_orbit = nb / len(rank)                    # blocks of one queue per orbit
    res["b_sequence_drift_middle_90pc"] = {"orbits": len(rank), "mean_orbits": round(float(dseq.mean()), 1), "worst_orbits": int(dseq.max()),
                                           "mean_as_blocks_of_a_queue": round(float(dseq.mean()) / 8 * per_orbit, 1),
                                           "worst_as_blocks_of_a_queue": round(float(dseq.max()) / 8 * per_orbit, 1)}
    names = ["rows", "slots", "req", "out"]
    X, y = [], []
    WIN = 1000
    for x in range(8):
        sel = np.where(queue == x)[0]                 # ascending block index = ascending position
        cs = np.vstack([np.zeros(4), np.cumsum(cost[sel], axis=0)])
        for w in range(0, len(sel) - WIN, WIN):
            X.append(cs[w + WIN] - cs[w])
            y.append((t0[sel[w + WIN]] - t0[sel[w]]) * TICK_US)
    X, y = np.array(X), np.array(y)
    res["c_windows"] = len(y)
    res["c_window_us_mean"] = round(float(y.mean()), 1)
    res["c_window_us_rel_spread"] = round(float(y.std() / y.mean()), 4)     # what a constant per block (the clock 'blocks') leaves
    fits = {}

    def fit(cols):
        A = X[:, cols]
        coef, *_ = np.linalg.lstsq(A, y, rcond=None)
        r = y - A @ coef
        return float(np.sqrt((r ** 2).mean()) / y.mean()), [float(c) for c in coef]

    for k, n in enumerate(names):
        rr, cf = fit([k])
        fits[n] = {"rel_rms": round(rr, 4), "us_per_unit": cf}
    best = None
    for k in range(4):
        for k2 in range(k + 1, 4):
            rr, cf = fit([k, k2])
            fits[names[k] + "+" + names[k2]] = {"rel_rms": round(rr, 4), "us_per_unit": cf}
            if best is None or rr < best[0]:
                best = (rr, names[k] + "+" + names[k2])
    res["c_fit"] = fits
    res["c_best_pair"] = best[1]
    print(json.dumps(res))
    return res


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "child":
        child(int(sys.argv[2]), sys.argv[3])
    elif len(sys.argv) >= 3 and sys.argv[1] == "run":
        run(sys.argv[2], [int(s) for s in sys.argv[3:]] or [28, 32])
    elif len(sys.argv) >= 3 and sys.argv[1] == "eval":
        evaluate(sys.argv[2], *[int(s) for s in sys.argv[3:5]])
    else:
        raise SystemExit(__doc__)
