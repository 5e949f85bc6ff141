#!/usr/bin/env python3
"""Headline benchmark: H|psi> matvecs/s for XXZChain(L=32, nup=16) (ComplexF64, N = 601 080 390)
on N MI355X GPUs of one node, the state sharded over the ranks for N > 1 (popcount-cell ownership by default,
SD_SHARD_MODE=range for contiguous basis-index ranges).

  python bench.py --gpus N --steps K --warmup W          (N > 1: starts its own N ranks, see self_launch)
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

A step = one pass of the hot path: out <- H psi on a random normalised psi resident in HBM (every step reads the same
psi and writes the same out, so the last step's output is H psi for any K; for N > 1 each step includes the RCCL halo
exchange).  Rank 0 prints ONE JSON line.

A plain run sets up, warms up, times the K steps and prints the line.  --full adds everything else the benchmark
measures or checks: the exactness self-checks before timing, the CPU baseline (unless --no-cpu) and, for N > 1, the
kernel-only timing behind `roofline` and the per-rank breakdown `per_rank_ms`.  --dump-outputs DIR writes a fixed, seeded
sample of the last step's output: DIR/Hpsi.npy (float64; [re, im] columns for c128) and DIR/rows.npy (their global basis
indices, as float64).
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X spec HBM3E peak (MI355X_MICROARCH.md)
HBM_COPY_GBS = 6290.0      # the guide's measured float4-copy ceiling: quoted beside the spec fraction
SEED = 20260821
DUMP_ROWS = 1 << 20        # --dump-outputs: sampled rows of a larger output (c128: 16 MB of values + 8 MB of indices)
# sources whose change invalidates a committed PMC traffic figure (profiles/collect_traffic.py stamps their hash)
TRAFFIC_SOURCES = ["spindynamics.jl_amd/csrc/kernels_apply.hip", "spindynamics.jl_amd/csrc/device_common.hpp",
                   "spindynamics.jl_amd/csrc/basis.cpp", "spindynamics.jl_amd/csrc/sd_internal.hpp"]


def kernel_source_hash():
    """Hash of what decides the apply kernel's memory traffic: the kernel and its device helpers, the plan / tile-order code, and
    the device-side structs of sd_internal.hpp (not the rest of that header: host-only fields do not change a kernel), with
    comments and white space removed."""
    import hashlib
    import re
    h = hashlib.sha256()
    for rel in TRAFFIC_SOURCES:
        with open(os.path.join(ROOT, rel), "rb") as f:
            data = f.read()
        text = data.decode()
        if rel.endswith("sd_internal.hpp"):
            parts = [re.search(r"struct %s \{.*?\n\};" % name, text, re.S) for name in ("sd_tile_rec", "sd_dev_model", "sd_epi_args")]
            text = "\n".join(m.group(0) if m else "" for m in parts)
        # comments and white space do not change a kernel: a note added to a source must not invalidate the measurement
        text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
        text = re.sub(r"//[^\n]*", "", text)
        h.update(" ".join(text.split()).encode())
    return h.hexdigest()[:16]


def self_launch(n):
    """`python bench.py --gpus N` without a launcher: this process -- which never touches a GPU and never imports torch --
    starts N ranks of this very script under torch.distributed.run on a free local port, passes their output through and
    exits with the launcher's status (non-zero when any rank failed)."""
    import socket
    import subprocess
    with socket.socket() as so:
        so.bind(("127.0.0.1", 0))
        port = so.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")    # dmabuf IPC: what RCCL needs on this image
    env.setdefault("OMP_NUM_THREADS", "1")
    sys.stderr.write("bench.py: starting %d ranks: %s\n" % (n, " ".join(cmd)))
    proc = subprocess.Popen(cmd, env=env, stdout=subprocess.PIPE, text=True, bufsize=1)
    for ln in proc.stdout:            # rank 0's JSON line goes to stdout; anything else a rank or its transport prints, to stderr
        out = sys.stdout if ln.lstrip().startswith("{") else sys.stderr
        out.write(ln)
        out.flush()
    raise SystemExit(proc.wait())


def host_cores():
    """Cores this process may really use: the scheduler affinity mask and the cgroup CPU quota, both reported."""
    aff = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = None
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            txt = open(path).read().split()
            if path.endswith("cpu.max"):
                if txt[0] != "max":
                    quota = float(txt[0]) / float(txt[1])
            else:
                q = float(txt[0])
                if q > 0:
                    quota = q / float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            break
        except Exception:
            continue
    use = aff if quota is None else max(1, min(aff, int(quota + 0.5)))
    return use, aff, quota


def cpu_baseline(L, nup, budget_s=20.0):
    """The C oracle (a port of the reference's algorithm: states[] + hash map, row-owner gather; Julia is absent on the
    box) timed on the host cores on a bounded sample: the same model family at L=28, scaled to
    L=32 rows.  Falls back to L=26 only when one L=28 apply alone would exceed the budget, and says so."""
    import numpy as np
    from oracle import oracle as O
    from math import comb
    Ls = int(os.environ.get("SD_BENCH_CPU_L", "28"))
    # threads = what this process is really allowed: min(affinity mask, cgroup CPU quota); SD_BENCH_CPU_THREADS overrides
    use, aff, quota = host_cores()
    ncores = int(os.environ.get("SD_BENCH_CPU_THREADS", str(use)))
    O.set_num_threads(ncores)
    note = ""
    while True:
        t0 = time.time()
        m = O.XXZChain(Ls, nup=Ls // 2)
        build_s = time.time() - t0
        rng = np.random.default_rng(1)
        psi = rng.standard_normal(m.N) + 1j * rng.standard_normal(m.N)
        t0 = time.time()
        O.apply_H(m, psi)  # warm
        first = time.time() - t0
        if first <= budget_s or Ls <= 26:
            break
        note = "; L=%d dropped: one apply took %.1f s > the %.0f s budget" % (Ls, first, budget_s)
        Ls = 26
    reps, t0 = 0, time.time()
    while True:
        O.apply_H(m, psi)
        reps += 1
        if time.time() - t0 > budget_s or reps >= 50:
            break
    dt = (time.time() - t0) / reps
    rows_per_s = m.N / dt
    n_full = comb(L, nup)
    return {
        "value": rows_per_s / n_full,
        "unit": "matvecs/s (L=32-equivalent, rows/s scaled by N)",
        "cores": O.num_threads(),
        "host_cpu_count": os.cpu_count(), "sched_affinity": aff, "cgroup_cpu_quota": quota,
        "kind": "port",
        "sample": f"oracle so_apply_H, XXZChain(L={Ls},nup={Ls // 2}) c128, N={m.N}, {reps} applies, "
                  f"{dt * 1e3:.1f} ms each ({rows_per_s / 1e6:.1f} Mrows/s) on {O.num_threads()} OpenMP threads (host has "
                  f"{os.cpu_count()} cores, affinity mask {aff}, cgroup quota {quota}); basis+hash build {build_s:.1f} s; extrapolated proportional to N (optimistic for the CPU: its "
                  f"hash map leaves cache at L=32){note}",
    }


def kernel_name(device_path, dtype):
    """The kernel the apply of this model runs (csrc/kernels_apply.hip, sd_launch_apply), from the plan the library built."""
    t = "<c128>" if dtype == "c128" else "<f64>"
    if device_path == "tiled":
        return "k_apply_tiled" + t + " (one launch per tile length class; all of them timed and counted together)"
    if device_path == "full-tiled":
        return "k_apply_fulltile" + t
    return "k_apply_generic" + t


def with_watchdog(fn, rank, on_timeout, status=3, limit_var="SD_BENCH_RCCL_TIMEOUT"):
    """Run fn() with a watchdog: a collective that never returns must not hang the run.  After `limit_var` seconds (default 120;
    SD_BENCH_RCCL_TIMEOUT for the library's sharded step, SD_BENCH_RELAY_TIMEOUT for the relay trial, SD_BENCH_EXIT_TIMEOUT, 60,
    for the closing barrier) on_timeout() is called (rank 0 prints the line it already has) and the process ends with `status`:
    3 for the library's own sharded step, so that the launcher and the driver see that this leg hung; 0 for the optional relay
    trial and the closing barrier, which leave a complete, verified direct-exchange measurement behind (the line says so)."""
    import threading
    limit = float(os.environ.get(limit_var, "60" if limit_var == "SD_BENCH_EXIT_TIMEOUT" else "120"))
    done = threading.Event()

    def watchdog():
        if not done.wait(limit):
            sys.stderr.write("rank %d: a communication leg did not finish within %.4g s (%s); giving up on it\n" % (rank, limit, limit_var))
            sys.stderr.flush()
            on_timeout()
            sys.stdout.flush()
            os._exit(status)      # the headline line is out; a hung library step must not read as a green run
    th = threading.Thread(target=watchdog, daemon=True)
    th.start()
    try:
        return fn()
    finally:
        done.set()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--L", type=int, default=int(os.environ.get("SD_BENCH_L", "32")))
    ap.add_argument("--dtype", default="c128", choices=["c128", "f64"])
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--full", action="store_true", help="also run the self-checks, the CPU baseline and the N > 1 breakdowns")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write a seeded sample of the last step's output as .npy files")
    args = ap.parse_args()

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args.gpus)        # does not return

    import torch
    import __graft_entry__ as g
    pkg = g.load_package()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        sys.stderr.write("bench.py: --gpus %d but WORLD_SIZE=%d: the launcher's world size is used\n" % (args.gpus, world))
    backend = os.environ.get("SD_BENCH_BACKEND", "nccl")   # "gloo": rehearsal of the N>1 control flow on a 1-GPU box
    if backend != "nccl":
        local_rank %= max(1, torch.cuda.device_count())
    elif local_rank >= torch.cuda.device_count():
        raise SystemExit("bench.py: rank %d needs GPU %d, but this node exposes %d GPU(s) -- one GPU per rank with RCCL "
                         "(SD_BENCH_BACKEND=gloo rehearses the N > 1 control flow with all ranks on one GPU)"
                         % (rank, local_rank, torch.cuda.device_count()))
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        import datetime
        tmo = datetime.timedelta(seconds=int(os.environ.get("SD_BENCH_DIST_TIMEOUT", "240")))   # a stuck exchange aborts, never hangs
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=tmo)
        else:
            dist.init_process_group(backend, timeout=tmo)

    L, nup = args.L, args.L // 2
    tdtype = torch.complex128 if args.dtype == "c128" else torch.float64
    esize = 16 if args.dtype == "c128" else 8
    model = pkg.XXZChain(L, nup=nup)
    op = pkg.ShardedOperator(model, rank, world)
    a = op.empty(tdtype, dev)
    b = op.empty(tdtype, dev)

    red_dev = dev if backend == "nccl" else "cpu"

    def all_ok(flag):
        """min over the ranks of a local 0/1 flag: every rank takes the same branch afterwards"""
        if dist is None:
            return bool(flag)
        t = torch.tensor([1.0 if flag else 0.0], device=red_dev)
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item() == 1.0)

    def selfcheck():
        """Exact, size-independent check of the path that is about to be timed (incl. the RCCL exchange): for the
        Heisenberg point of the open chain H|F> = (L-1)/4 |F> holds bit for bit for the uniform vector |F>
        (all partial sums are small dyadic rationals), on every row of every rank.  A rank whose check raises still
        takes part in the reduction, so no rank is left waiting in a collective while another runs the fallback."""
        ok = False
        try:
            a.fill_(1.0)
            b.zero_()
            op.apply(b, a)
            ok = bool((b == (L - 1) / 4).all())
        except Exception as e:             # noqa: BLE001 -- reported, then every rank runs the fallback together
            sys.stderr.write("rank %d: self-check raised %r\n" % (rank, e))
        return all_ok(ok)

    def selfcheck_vs_unsharded():
        """N > 1: the sharded apply of the counter-based random vector (keyed by the global index, identical for every
        sharding) against the unsharded apply of the same vector on this rank's own GPU, owned rows compared bit for
        bit.  Unlike the uniform state this sees a halo row that arrived in the wrong place."""
        ok = False
        try:
            ref_model = pkg.XXZChain(L, nup=nup)
            ref_op = pkg.ShardedOperator(ref_model, 0, 1)
            x = ref_op.fill_randn(ref_op.empty(tdtype, dev), SEED)
            y = torch.empty_like(x)
            ref_op.apply(y, x)
            lb, gb, ln = model.local_tiles()
            if len(ln):
                lens = torch.from_numpy(ln.astype("int64")).to(dev)
                starts = torch.from_numpy(gb - lb).to(dev)               # global row = local row + (gb - lb) of its tile
                order = torch.from_numpy(lb).to(dev).argsort()
                rows = torch.arange(op.n_local, device=dev) + torch.repeat_interleave(starts[order], lens[order])
                op.fill_randn(a, SEED)
                b.zero_()
                op.apply(b, a)
                ok = bool(torch.equal(a, x[rows])) and bool(torch.equal(b, y[rows]))
                del rows
            else:
                ok = True
            del x, y, ref_op, ref_model
            torch.cuda.empty_cache()
        except Exception as e:             # noqa: BLE001
            sys.stderr.write("rank %d: unsharded cross-check raised %r\n" % (rank, e))
        return all_ok(ok)

    def relay_selfcheck():
        """Relays on (SD_RELAY): the halo that arrives over the two-hop routes must equal, bit for bit, the halo of the
        direct exchange of the same vector; otherwise the routes are dropped on every rank."""
        routes = op.relay_plan()
        if routes is None:
            return "direct"
        ok = False
        try:
            op.fill_randn(a, SEED)
            h1 = op.exchange(a).clone()
            saved, op._routes = op._routes, False
            h2 = op.exchange(a).clone()
            op._routes = saved
            ok = bool(torch.equal(h1, h2))
        except Exception as e:             # noqa: BLE001
            sys.stderr.write("rank %d: relay self-check raised %r\n" % (rank, e))
        if all_ok(ok):
            return "two-hop relays (SD_RELAY), halo identical to the direct exchange"
        op._routes = False
        return "direct (relay routes FAILED their self-check and were dropped)"

    check = "uniform state exact eigenvector on all ranks"
    if os.environ.get("SD_DEBUG_SKIP", "0") not in ("", "0"):
        check = "SKIPPED: SD_DEBUG_SKIP timing ablation (results are wrong by construction)"
    elif not args.full:
        check = "not run (plain run; --full runs the self-checks)"
    else:
        good = selfcheck()
        if good and world > 1:
            good = selfcheck_vs_unsharded()
            check += "; owned rows of the random vector's sharded apply == unsharded apply, bit for bit"
        if not good:
            # fall back to the simplest distributed path before giving up: index ranges, no overlap, no relays
            if world > 1 and op.mode == "class":
                os.environ["SD_RELAY"] = "0"
                model = pkg.XXZChain(L, nup=nup)
                op = pkg.ShardedOperator(model, rank, world, mode="range")
                op.overlap = False
                a = op.empty(tdtype, dev)
                b = op.empty(tdtype, dev)
                check = "FELL BACK to index ranges without overlap (popcount-cell path failed its self-check)"
                if not (selfcheck() and selfcheck_vs_unsharded()):
                    raise SystemExit("sharded apply failed its exactness self-check on rank %d" % rank)
            else:
                raise SystemExit("apply failed its exactness self-check on rank %d" % rank)
    halo_routing = relay_selfcheck() if world > 1 else "none (one rank)"
    op.fill_randn(a, SEED)
    nrm = op.norm(a)
    a /= nrm
    b.zero_()

    def dump_outputs(out, path):
        """The last step's output at DUMP_ROWS global basis indices drawn with SEED (all rows when N is smaller), gathered
        on rank 0 from the ranks that own them and written as float64: Hpsi.npy ([re, im] columns for c128), rows.npy."""
        import numpy as np
        rows = np.arange(model.N, dtype=np.int64)
        if model.N > DUMP_ROWS:
            rows = np.unique(np.random.default_rng(SEED).integers(0, model.N, DUMP_ROWS))
        lb, gb, ln = model.local_tiles()            # local row lb+i <-> global row gb+i
        order = np.argsort(gb)
        lb, gb, ln = lb[order], gb[order], ln[order].astype(np.int64)
        t = np.searchsorted(gb, rows, side="right") - 1
        own = t >= 0
        own[own] = rows[own] < gb[t[own]] + ln[t[own]]
        local = lb[t[own]] + rows[own] - gb[t[own]]
        if len(local) and not (local.min() >= 0 and local.max() < out.numel()):
            raise SystemExit("bench.py: --dump-outputs: a local row outside this rank's vector")
        vals = out[torch.from_numpy(local).to(out.device)]
        vals = torch.view_as_real(vals) if vals.is_complex() else vals
        parts = [(np.flatnonzero(own), vals.cpu().numpy())]
        if dist is not None:
            mine, parts = parts[0], [None] * world
            dist.all_gather_object(parts, mine)
        if rank != 0:
            return
        got = np.full((len(rows),) + parts[0][1].shape[1:], np.nan)
        seen = np.zeros(len(rows), bool)
        for pos, v in parts:
            got[pos] = v
            seen[pos] = True
        if not seen.all():
            raise SystemExit("bench.py: --dump-outputs: %d sampled rows are owned by no rank" % (~seen).sum())
        os.makedirs(path, exist_ok=True)
        np.save(os.path.join(path, "Hpsi.npy"), got)
        np.save(os.path.join(path, "rows.npy"), rows.astype(np.float64))

    def sync():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(apply_fn, src, dst):
        """W untimed + K timed steps of apply_fn(dst, src) bracketed by barrier + synchronize; the MAX over the ranks of the
        wall time, the device time per step on the launch stream, the sorted per-step device times, and src / dst.  Every
        step reads the same src: a chain of applies would grow like |E0|^steps and overflow float64 after a few hundred."""
        for _ in range(args.warmup):
            apply_fn(dst, src)
        sync()
        ev0, ev1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]   # per-step device times (median / min)
        t0 = time.perf_counter()
        ev0.record()
        marks[0].record()
        for k in range(args.steps):
            apply_fn(dst, src)
            marks[k + 1].record()
        ev1.record()
        sync()
        t1 = time.perf_counter()
        step_ms = sorted(marks[k].elapsed_time(marks[k + 1]) for k in range(args.steps))
        elapsed = t1 - t0
        if dist is not None:
            t = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            elapsed = float(t.item())
        return elapsed, ev0.elapsed_time(ev1) / args.steps, step_ms, src, dst

    # the Python-issued path (pack kernel, torch.distributed batch_isend_irecv, interior / boundary launches): always measured
    elapsed, ev_ms, step_ms, src, dst = timed(lambda d, s_: op.apply(d, s_), a, b)
    path_used = "python: torch.distributed point-to-point issued per step" if world > 1 else "single rank"

    # kernel-only timing (no exchange) for the roofline of the dominant kernel: HIP events around K launches (N > 1: --full)
    kern_ms = ev_ms if world == 1 else None
    if world > 1 and args.full:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(args.steps):
            op.apply(dst, src, exchange=False)
        e1.record()
        torch.cuda.synchronize()
        kern_ms = e0.elapsed_time(e1) / args.steps

    # ---- N > 1: where a step's time goes on every rank (--full) ----
    per_rank = None
    if world > 1 and args.full:
        prof = [op.apply_profiled(dst, src) for _ in range(3)][-1]
        prof["rank"] = rank
        prof["rows_owned"], prof["rows_imported"] = op.n_local, op.n_halo
        prof["bytes_sent_per_peer"] = {str(peer): cnt * esize for (peer, _off, cnt, _g) in op.send_slabs}
        prof["bytes_recv_per_peer"] = {str(peer): cnt * esize for (peer, _off, cnt, _g) in op.recv_slabs}
        prof["kernel_only"] = kern_ms
        per_rank = [None] * world
        dist.all_gather_object(per_rank, prof)

    def build_line(elapsed, step_ms, path_used, library_path):
        N = model.N
        ms_per_step = elapsed / args.steps * 1e3
        alg_bytes = op.n_local * 2 * esize               # read psi[idx] once + write out[idx] once
        achieved = alg_bytes / (kern_ms * 1e-3) / 1e9 if kern_ms is not None else None   # GB/s on this rank's GPU
        # HBM-side bytes per apply from the PMC counters (2*FETCH_SIZE + WRITE_SIZE, gfx950 correction): collected by
        # profiles/run_profile.sh in separate rocprofv3 passes and committed with the hash of the kernel sources it was
        # measured on.  A figure measured on other sources is not reported.
        traffic, traffic_source = None, "no PMC figure for this workload (profiles/traffic_latest.json)"
        valu_insts = None
        tp = os.path.join(ROOT, "profiles", "traffic_latest.json")
        if os.path.exists(tp):
            try:
                tj = json.load(open(tp))
                if tj.get("L") == L and tj.get("dtype") == args.dtype and world == 1:
                    if tj.get("source_hash") == kernel_source_hash():
                        traffic = tj.get("hbm_bytes_per_launch")
                        valu_insts = tj.get("SQ_INSTS_VALU_per_launch")
                        traffic_source = "profiles/traffic_latest.json, measured on these kernel sources (hash %s)" % tj.get("source_hash")
                    else:
                        traffic_source = "profiles/traffic_latest.json is stale (kernel sources changed since it was measured): null"
            except Exception:
                traffic = None
        return {
            "metric": "H|psi> matvecs/s, XXZ L=%d Sz=0" % L,
            "value": args.steps / elapsed,
            "unit": "matvecs/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "ms_per_step_median": step_ms[len(step_ms) // 2], "ms_per_step_min": step_ms[0],   # rank 0, device time per step
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": args.dtype,
            "data": "synthetic: counter-based N(0,1) psi keyed by (seed=%d, global index), normalised" % SEED,
            "config": {"workload": "XXZChain(L=%d, nup=%d) open, Jxy=Jz=1, hz=0: out <- H psi, %s, N=%d, per-row summation in the "
                                   "reference's order (bit-identical to the CPU oracle); %s shards, %d rank(s), halo exchange per step"
                                   % (L, nup, "ComplexF64" if args.dtype == "c128" else "Float64", N,
                                      "popcount-cell" if op.mode == "class" else "basis-index-range", world),
                       "rows_per_rank": op.n_local, "halo_rows_rank0": op.n_halo, "shard_mode": op.mode,
                       "device_path": model.device_path,
                       "halo_routing": halo_routing, "per_rank_ms": per_rank,
                       # which path the headline was timed on, and the other one beside it (N > 1): the library's own sharded step
                       # (sd_apply_sharded on its RCCL communicator -- what every sharded recursion runs) or the Python-issued one
                       "path": path_used, "library_path": library_path},
            "selfcheck": check,
            "achieved_hbm_GBs_per_gpu": achieved,
            "roofline": None if kern_ms is None else {"bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                         "frac": achieved / HBM_PEAK_GBS, "frac_of_copy_ceiling": achieved / HBM_COPY_GBS,
                         "traffic": traffic, "traffic_source": traffic_source,
                         # the verdict on the 0.60 target in numbers: how many times the algorithmic bytes
                         # cross the fabric side of the L2s, at what rate (the chip sustains 7.4-7.9 TB/s there for gathers past
                         # L2, MI355X_MICROARCH.md), and the time the VALU instruction stream alone would take (SQ_INSTS_VALU
                         # wave-instructions x 4 cycles on 1024 SIMDs at 2.4 GHz) -- a second ceiling under the byte one
                         "traffic_ratio": (traffic / alg_bytes) if traffic else None,
                         "fabric_GBs": (traffic / (kern_ms * 1e-3) / 1e9) if traffic else None,
                         "valu_wave_insts": valu_insts,
                         "valu_lane_ops_per_row": (valu_insts * 64.0 / op.n_local) if valu_insts else None,
                         "valu_issue_floor_ms": (valu_insts * 4.0 / (1024 * 2.4e9) * 1e3) if valu_insts else None,
                         "target_frac": 0.60, "target_met": bool(achieved / HBM_PEAK_GBS >= 0.60),
                         "kernel": kernel_name(model.device_path, args.dtype),
                         "kernel_ms": kern_ms, "algorithmic_bytes_per_launch": alg_bytes},
        }

    line = build_line(elapsed, step_ms, path_used, None) if rank == 0 else None
    if world > 1:
        # ---- the library's own sharded step: sd_apply_sharded on the communicator ShardedOperator.comm() settles on (RCCL itself
        # under an NCCL process group, after its self-test on every rank; torch.distributed callbacks otherwise).  Checked bit for
        # bit against the Python-issued step before it is timed; when it passes, IT is the headline (it is what every sharded
        # recursion runs) and the Python-issued figure is reported beside it.
        def on_timeout():
            if rank == 0:
                line["config"]["library_path"] = {"status": "timeout: the library's communication path did not return (SD_BENCH_RCCL_TIMEOUT)",
                                                  "python_path_ms_per_step": line["ms_per_step"]}
                print(json.dumps(line), flush=True)

        def library_leg():
            info = {}
            try:
                op.comm(dev)
                info["communicator"] = op.comm_kind
                if op.comm_note:
                    info["note"] = op.comm_note
                ref = torch.empty_like(dst)
                op.apply(ref, src)
                op.apply_lib(dst, src)
                torch.cuda.synchronize()
                same = bool(torch.equal(ref, dst))
                del ref
                if not all_ok(same):
                    info["status"] = "ran, but its result differs from the Python-issued step: not timed"
                    return info, None
                el, _ev, st, _s, _d = timed(lambda d, s_: op.apply_lib(d, s_), src, dst)
                info["status"] = "ok: bit-identical to the Python-issued step"
                info["ms_per_step"] = el / args.steps * 1e3
                return info, (el, st)
            except Exception as e:     # noqa: BLE001 -- a failed leg is reported, the Python-issued headline stays
                info["status"] = "failed: %r" % (e,)
                all_ok(False)
                return info, None
        info, res = with_watchdog(library_leg, rank, on_timeout)
        info["python_path_ms_per_step"] = elapsed / args.steps * 1e3
        head_path = path_used
        if res is not None:
            head_path = "library: sd_apply_sharded on the %s communicator" % (
                "library's RCCL" if info.get("communicator") == "rccl" else "torch.distributed callback")
        head_el = res[0] if res is not None else elapsed
        if rank == 0:
            if res is not None:
                line = build_line(res[0], res[1], head_path, info)
            else:
                line["config"]["library_path"] = info

        # ---- two-hop relays, tried AFTER the direct exchange has been measured (SD_RELAY unset; SD_BENCH_RELAY_TRIAL=0 skips, =2
        # forces routes even where none pays: rehearsals).  xGMI is point to point and the busiest pair of this exchange carries
        # 2-3x the mean: with 8 ranks the routes cut the busiest link from 0.285 to 0.171 GB.  The routed
        # exchange has never met real links, so it must earn the headline: same halo and same H psi to the bit, and faster than the
        # direct step on this very run; otherwise the direct figure stands.  A routed exchange that hangs ends the run from
        # its watchdog with the direct line printed and `relay_trial` saying so.
        trial_mode = os.environ.get("SD_BENCH_RELAY_TRIAL", "1")
        if world >= 3 and op.mode == "class" and "SD_RELAY" not in os.environ and trial_mode != "0":
            apply_head = (lambda d, s_: op.apply_lib(d, s_)) if res is not None else (lambda d, s_: op.apply(d, s_))

            def trial_timeout():
                if rank == 0:
                    line["config"]["relay_trial"] = {"status": "timeout: the routed exchange did not return; the headline is the direct "
                                                               "exchange measured before it"}
                    print(json.dumps(line), flush=True)

            def relay_trial():
                tinfo = {}
                try:
                    op._routes = None
                    routes = op.relay_plan(relay=trial_mode)
                    if routes is None:
                        tinfo["status"] = "no route brings the busiest link below 0.9 of the busiest direct message: direct exchange kept"
                        return tinfo, None
                    op._routes = False
                    h_direct = op.exchange(src).clone()
                    ref = torch.empty_like(dst)
                    apply_head(ref, src)
                    op.set_relay(routes)
                    h_routed = op.exchange(src)
                    apply_head(dst, src)
                    torch.cuda.synchronize()
                    same = bool(torch.equal(h_direct, h_routed)) and bool(torch.equal(ref, dst))
                    del ref, h_direct
                    if not all_ok(same):
                        op.set_relay(None)
                        tinfo["status"] = "routed halo or H psi differs from the direct exchange: routes dropped"
                        return tinfo, None
                    el, _ev, st, _s, _d = timed(apply_head, src, dst)
                    tinfo["ms_per_step"] = el / args.steps * 1e3
                    tinfo["direct_ms_per_step"] = head_el / args.steps * 1e3
                    if el < head_el:
                        tinfo["status"] = "ok: halo and H psi bit-identical to the direct exchange, and faster: headline"
                        return tinfo, (el, st)
                    op.set_relay(None)
                    tinfo["status"] = "ok (bit-identical) but not faster than the direct exchange: direct headline kept"
                    return tinfo, None
                except Exception as e:     # noqa: BLE001 -- the direct headline stays
                    tinfo["status"] = "failed: %r" % (e,)
                    all_ok(False)
                    return tinfo, None
            tinfo, tres = with_watchdog(relay_trial, rank, trial_timeout, status=0, limit_var="SD_BENCH_RELAY_TIMEOUT")
            if tres is not None:
                halo_routing = "two-hop relays (tried after the direct exchange: bit-identical halo, faster)"
            if rank == 0:
                if tres is not None:
                    line = build_line(tres[0], tres[1], head_path + ", halo over pipelined two-hop relays", info)
                line["config"]["relay_trial"] = tinfo
    if args.dump_outputs:
        dump_outputs(dst, args.dump_outputs)
    if rank == 0:
        if world == 1 and args.full and not args.no_cpu:
            try:
                line["cpu_baseline"] = cpu_baseline(L, nup)
            except Exception as e:  # the baseline is a report, never a reason to lose the GPU number
                line["cpu_baseline"] = {"value": None, "unit": "matvecs/s", "cores": 0, "kind": "port",
                                        "sample": "failed: %r" % (e,)}
        print(json.dumps(line), flush=True)
    if dist is not None:
        # the line is out; a rank that left an optional leg through its watchdog must not keep the others in this barrier
        with_watchdog(lambda: (dist.barrier(), dist.destroy_process_group()), rank, lambda: None, status=0, limit_var="SD_BENCH_EXIT_TIMEOUT")


if __name__ == "__main__":
    main()
