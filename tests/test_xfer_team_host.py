"""The copy team of the staged host <-> device transfers (csrc/xfer_team.hpp), on the host: tests/xfer_team_host.cpp includes the
header and is compiled with the host compiler, as the library's xfer.cpp includes it.

bounds: sd_xfer_team::slice_bounds for n = 1..64 members over every byte count 0..2^17, every 4096 n j + r with j in {1, 16, 256,
257} and r = 0..n, 2^20 -+ 8 and 2^25 + 8: the n slices ascend, are disjoint, lie in [0, bytes], cover [0, bytes) and meet at
multiples of 4096.  The slice length was once (bytes / n) rounded up to a page; whenever bytes / n was itself a multiple of 4096
the last bytes % n bytes then belonged to no member -- 10 767 of the 8 397 440 cells here, all of that class and no other.

copy n: one team of n = 1..16 threads over a list of copies in sequence (the team and its generation counter reused, lengths up
and down, copies below the 1 MiB threshold -- the caller's own memcpy -- in between): 0, 1, 8, 2^20 - 8, 2^20, 2^20 + 8, the
smallest 4096 n j + r >= 2^20 for every r in 1..n-1, 3 MiB + 12 345, 8 MiB, 16 MiB + 8; source and destination 0, 1 and 8 bytes
past a page boundary.  The source is a hash of the offset, the destination holds its complement between two guards of 4096 bytes;
after each copy every byte is the source's, the guards and the source are intact.

The same program under ThreadSanitizer, and under AddressSanitizer with UndefinedBehaviorSanitizer, on n = 2, 7, 16 and the
lengths around 2^20 (the `reduced` list): stand-alone binaries, nothing preloaded.  A sanitizer build is skipped only where a
one-line program does not link with its flag."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BASE = ["g++", "-std=c++17", "-pthread", "-Wall", "-Wextra", "-Werror"]
SANITIZERS = {"tsan": "-fsanitize=thread", "asan_ubsan": "-fsanitize=address,undefined"}


def build(outdir, name, extra):
    out = os.path.join(str(outdir), name)
    cmd = BASE + extra + ["-I", os.path.join(ROOT, "spindynamics.jl_amd", "csrc"), os.path.join(ROOT, "tests", "xfer_team_host.cpp"),
                          "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return out


def run(exe, *args):
    """-> number of cells; any FAIL line, a sanitizer report (stderr) or a non-zero exit status is an assertion failure"""
    env = dict(os.environ, TSAN_OPTIONS="halt_on_error=0 exitcode=66", ASAN_OPTIONS="detect_leaks=1",
               UBSAN_OPTIONS="print_stacktrace=1 halt_on_error=0 exitcode=66")
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=300, env=env)
    lines = r.stdout.splitlines()
    fails = [ln for ln in lines if ln.startswith("FAIL")]
    assert not fails, "%d failing cells, the first:\n%s" % (len(fails), "\n".join(fails[:8]))
    assert r.returncode == 0 and r.stderr == "", "exit status %d\n%s" % (r.returncode, r.stderr[-4000:])
    assert lines and lines[-1].startswith("ok "), r.stdout[-400:]
    return int(lines[-1].split()[1])


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return build(tmp_path_factory.mktemp("xfer_team"), "xfer_team_host", ["-O2"])


@pytest.fixture(scope="module", params=list(SANITIZERS))
def sanitized(request, tmp_path_factory):
    flag = SANITIZERS[request.param]
    d = tmp_path_factory.mktemp("xfer_team_" + request.param)
    one = os.path.join(str(d), "one.cpp")
    with open(one, "w") as f:
        f.write("int main() { return 0; }\n")
    r = subprocess.run(["g++", flag, one, "-o", os.path.join(str(d), "one")], capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the host compiler does not link with %s: %s" % (flag, r.stderr.strip()[-200:]))
    return build(d, "xfer_team_host_" + request.param, ["-O1", "-g", "-fno-omit-frame-pointer", flag])


def test_slices_tile_every_length(exe):
    # 64 * (2^17 + 1 + the 4096 n j + r + 3) cells: sum over n of 4 (n + 1) = 8576
    assert run(exe, "bounds") == 64 * ((1 << 17) + 1 + 3) + 8576


@pytest.mark.parametrize("n", range(1, 17))
def test_team_copies_every_byte(exe, n):
    # 10 fixed entries, the class of n - 1 lengths twice and an 8 after every fourth, each at 3 x 3 offsets
    assert run(exe, "copy", str(n)) == 9 * (10 + 2 * (n - 1) + (n + 1) // 4)


@pytest.mark.parametrize("n", [2, 7, 16])
def test_team_under_sanitizers(sanitized, n):
    assert run(sanitized, "copy", str(n), "reduced") == 9 * (6 + 2 * (n - 1) + (n + 1) // 4)
