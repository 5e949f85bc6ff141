"""bench.py as the driver runs it: a plain run times exactly --steps steps and leaves the self-checks and the CPU baseline
to --full; --dump-outputs writes a seeded sample of the last step's output, which must be H psi of the benchmark's own
psi (the CPU oracle's, at the sampled rows) for one rank and for two."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(args, **env_extra):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "SD_RELAY")}
    env.update(env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, cwd=ROOT, capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def check_dump(pkg, O, L, path):
    """The dumped rows against the oracle's H psi, psi = bench.py's counter-based vector normalised as bench.py does."""
    import torch
    import bench
    rows = np.load(os.path.join(path, "rows.npy"))
    got = np.load(os.path.join(path, "Hpsi.npy"))
    assert rows.dtype == np.float64 and got.dtype == np.float64
    assert os.path.getsize(os.path.join(path, "rows.npy")) + os.path.getsize(os.path.join(path, "Hpsi.npy")) <= 64 << 20
    model = pkg.XXZChain(L, nup=L // 2)
    op = pkg.ShardedOperator(model, 0, 1)
    x = op.fill_randn(op.empty(torch.complex128, "cuda"), bench.SEED)
    x /= op.norm(x)
    psi = np.empty(model.N, np.complex128)
    psi[model.local_rows()] = x.cpu().numpy()
    want = O.apply_H(O.XXZChain(L, nup=L // 2), psi)
    idx = rows.astype(np.int64)
    assert np.array_equal(idx, rows) and (np.diff(idx) > 0).all() and idx[0] >= 0 and idx[-1] < model.N
    if model.N > bench.DUMP_ROWS:
        assert 0.5 * bench.DUMP_ROWS < len(idx) <= bench.DUMP_ROWS       # a sample, drawn with bench.SEED
    else:
        assert len(idx) == model.N
    assert got.shape == (len(idx), 2)
    err = np.abs(got[:, 0] + 1j * got[:, 1] - want[idx]).max()
    assert err <= 1e-14, err
    return rows, got


def test_plain_run_times_the_steps_and_dumps_H_psi(pkg, O, tmp_path):
    line = run_bench(["--gpus", "1", "--L", "24", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)])
    assert line["metric"] == "H|psi> matvecs/s, XXZ L=24 Sz=0" and line["unit"] == "matvecs/s" and line["higher_is_better"] is True
    assert line["dtype"] == "c128" and line["steps"] == 3 and line["warmup"] == 1
    assert line["ms_per_step"] > 0 and abs(line["value"] - 1e3 / line["ms_per_step"]) <= 1e-9 * line["value"]
    assert line["selfcheck"].startswith("not run") and "cpu_baseline" not in line
    assert line["roofline"]["kernel_ms"] > 0
    check_dump(pkg, O, 24, str(tmp_path))


def test_full_run_adds_the_self_check_and_the_cpu_baseline():
    line = run_bench(["--gpus", "1", "--L", "20", "--steps", "3", "--warmup", "1", "--full"], SD_BENCH_CPU_L="20")
    assert line["selfcheck"] == "uniform state exact eigenvector on all ranks"
    assert line["cpu_baseline"]["value"] > 0 and "L=20" in line["cpu_baseline"]["sample"]


def test_two_rank_dump_matches_the_one_rank_dump(pkg, O, tmp_path):
    """Two gloo ranks on this GPU: rank 0 gathers the sampled rows from the rank that owns each; the same rows as one rank and
    the same values to rounding (the norm that scales psi sums the ranks' partial sums), and the oracle's."""
    one, two = tmp_path / "one", tmp_path / "two"
    run_bench(["--gpus", "1", "--L", "24", "--steps", "2", "--warmup", "0", "--dump-outputs", str(one)])
    line = run_bench(["--gpus", "2", "--L", "24", "--steps", "2", "--warmup", "0", "--dump-outputs", str(two)],
                     SD_BENCH_BACKEND="gloo")
    assert line["n_gpus"] == 2 and line["config"]["per_rank_ms"] is None and line["roofline"] is None   # --full only
    rows1, got1 = check_dump(pkg, O, 24, str(one))
    rows2, got2 = check_dump(pkg, O, 24, str(two))
    assert np.array_equal(rows1, rows2) and np.abs(got1 - got2).max() <= 1e-15
