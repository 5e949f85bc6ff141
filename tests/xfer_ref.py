"""What tests/test_gpu_host_transfers.py needs beside the GPU: the constants of csrc/xfer.cpp and csrc/xfer_team.hpp read from the
sources, the byte pattern, host buffers between guards at a chosen distance from a page boundary, the list of cells, and the build
of tests/xfer_shim.cpp.  A transfer has no arithmetic: the yardstick is the source bytes themselves, compared under ==."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "spindynamics.jl_amd", "csrc")
MiB = 1 << 20
PAGE = 4096
HOST_GUARD = 4096                   # guard bytes on each side of a host buffer
DEV_GUARD = 256                     # guard bytes on each side of a device buffer
GUARD_BYTE = 0xA5
MAX_BYTES = 27 * MiB                # the largest transfer of the file
THREADS = (1, 2, 3, 7, 12, 16)
CHUNKS_MB = (1, 2, 3)


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def constants():
    """-> dict: NBUF (slots of the pinned ring), TEAM_MIN (bytes from which a copy is shared by the team), MIN_MB and CHUNK_MB (the
    defaults of SD_XFER_MIN_MB and SD_XFER_CHUNK_MB), MAX_THREADS (the default team's cap)"""
    x, t = _read("xfer.cpp"), _read("xfer_team.hpp")
    return {
        "NBUF": int(re.search(r"constexpr int NBUF = (\d+);", x).group(1)),
        "TEAM_MIN": 1 << int(re.search(r"nthreads == 1 \|\| b < \(\(size_t\)1 << (\d+)\)", t).group(1)),
        "MIN_MB": int(re.search(r'env_mb\("SD_XFER_MIN_MB", (\d+)\)', x).group(1)),
        "CHUNK_MB": int(re.search(r'env_mb\("SD_XFER_CHUNK_MB", (\d+)\)', x).group(1)),
        "MAX_THREADS": int(re.search(r"std::min\((\d+), allowed_cores\(\)\)", x).group(1)),
    }


def team_lifetime_facts():
    """What the tests rely on when they change SD_XFER_THREADS, read off csrc/xfer.cpp: the variable is read in ensure_ring alone,
    and only where the context has no team; ensure_ring returns early while the chunk size stands, and otherwise releases ring and
    team together (sd_xfer_release deletes the team).  So a new thread count takes effect with a new chunk size or after
    release_scratch(), and not before.  -> dict of booleans, all of which must hold"""
    x = _read("xfer.cpp")
    ring = x[x.index("int ensure_ring("):x.index("int plain(")]
    release = x[x.index("void sd_xfer_release("):]
    return {
        "threads are read in ensure_ring alone": x.count('getenv("SD_XFER_THREADS")') == ring.count('getenv("SD_XFER_THREADS")') > 0,
        "and only without a team": ring.index("if (!ctx->xfer_team)") < ring.index('getenv("SD_XFER_THREADS")'),
        "the ring is kept while the chunk size stands": re.search(
            r"if \(ctx->xfer_chunk == chunk && ctx->xfer_buf\[0\]\) return SD_OK;\s*sd_xfer_release\(ctx\);", ring) is not None,
        "release frees the team with the ring": "delete ctx->xfer_team;" in release and "hipHostFree(ctx->xfer_buf[k])" in release,
    }


def pattern():
    """MAX_BYTES + 64 KiB position-dependent bytes, read-only: a slice copied from or to a shifted offset, or twice, differs"""
    p = np.random.default_rng(20211).integers(0, 256, MAX_BYTES + (1 << 16), dtype=np.uint8)
    p.setflags(write=False)
    return p


class HostArena:
    """front guard | data | back guard inside one allocation; the data start `off` bytes past a page boundary"""

    def __init__(self, cap=MAX_BYTES):
        self.raw = np.empty(cap + 2 * HOST_GUARD + 3 * PAGE, dtype=np.uint8)
        self.base = (-self.raw.ctypes.data) % PAGE

    def place(self, nbytes, off):
        s = self.base + HOST_GUARD + off
        assert (self.raw.ctypes.data + s) % PAGE == off and s + nbytes + HOST_GUARD <= len(self.raw)
        front, data, back = self.raw[s - HOST_GUARD:s], self.raw[s:s + nbytes], self.raw[s + nbytes:s + nbytes + HOST_GUARD]
        front[:] = GUARD_BYTE
        back[:] = GUARD_BYTE
        return data, (front, back)


def mismatch(got, want):
    """None when equal, else a sentence with the number of differing bytes and the first of them"""
    if got.shape == want.shape and np.array_equal(got, want):
        return None
    if got.shape != want.shape:
        return "shape %s, expected %s" % (got.shape, want.shape)
    idx = np.flatnonzero(got != want)
    return "%d bytes wrong, first at %d of %d" % (len(idx), idx[0], len(got))


def guards_intact(guards):
    return all(bool((g == GUARD_BYTE).all()) for g in guards)


# ---- the cells ----
def class_length(n, r, at_least):
    """the smallest 4096 n j + r >= at_least with j >= 1: the lengths whose last r bytes a slice length of (bytes / n) rounded up to
    a page left to nobody"""
    step = PAGE * n
    j = max(1, -(-(at_least - r) // step))
    return step * j + r


def counts(NBUF):
    """name -> number of chunks, in terms of the ring: a device-to-host copy runs NBUF - 1 chunks ahead, chunk NBUF is the first to
    use a slot a second time"""
    return {"one": 1, "two": 2, "lookahead": NBUF - 1, "ring": NBUF, "reuse": NBUF + 1, "tworings": 2 * NBUF, "tworings+1": 2 * NBUF + 1}


def tail_length(kind, chunk, n, consts, r=8):
    """length of the last chunk, or None where the kind does not exist at this chunk size / thread count"""
    T = consts["TEAM_MIN"]
    if kind == "8":
        return 8
    if kind == "alone":                         # below the team's threshold: the caller's own memcpy
        return T - 8
    if kind == "full":
        return chunk
    if kind == "ragged":                        # shared by the team, no whole number of pages
        return T + 8 if T + 8 < chunk else None
    if kind == "class":
        t = class_length(n, r, T)
        return t if 0 < r < n and t < chunk else None
    raise ValueError(kind)


def assert_edge(cell, consts):
    """every cell first asserts the edge it is there to cross"""
    chunk, n, nbytes, tail = cell["chunk_mb"] * MiB, cell["threads"], cell["bytes"], cell["tail"]
    T, NBUF = consts["TEAM_MIN"], consts["NBUF"]
    assert 1 <= n <= consts["MAX_THREADS"] == 16
    assert 0 < nbytes <= MAX_BYTES == 27 * MiB
    nchunks = -(-nbytes // chunk)
    if cell["count"] is not None:
        assert nchunks == counts(NBUF)[cell["count"]] and nbytes == (nchunks - 1) * chunk + tail
    kind = cell["kind"]
    if kind == "8":
        assert tail == 8 < T
    elif kind == "alone":
        assert tail == T - 8 < chunk
    elif kind == "full":
        assert tail == chunk and nbytes % chunk == 0 and chunk >= T
    elif kind == "ragged":
        assert T <= tail < chunk and tail % PAGE != 0
    elif kind == "class":
        assert T <= tail < chunk and (tail // n) % PAGE == 0 and tail % n == cell["r"] != 0
    elif kind == "odd":
        assert nbytes % 8 != 0
    else:
        raise ValueError(kind)
    staged = cell["mode"] == "staged" or (cell["mode"] == "auto" and nbytes >= cell["min_mb"] * MiB)
    assert cell["staged"] == staged


def cells(consts):
    """the list of cells of the grid: dicts with mode, dir, chunk_mb, threads, count (name in counts(), or None), kind, tail, r,
    bytes, off (host bytes past a page boundary), min_mb, staged, id"""
    NBUF = consts["NBUF"]
    cnt = counts(NBUF)
    assert sorted(cnt.values()) == [1, 2, 3, 4, 5, 8, 9]
    out = []
    rot = [0]

    def add(mode, chunk_mb, n, count, kind, tail, r=0, nbytes=None):
        chunk = chunk_mb * MiB
        if nbytes is None:
            nbytes = (cnt[count] - 1) * chunk + tail
        for d in ("h2d", "d2h"):
            rot[0] += 1
            c = dict(mode=mode, dir=d, chunk_mb=chunk_mb, threads=n, count=count, kind=kind, tail=tail, r=r, bytes=nbytes,
                     off=8 * (rot[0] // 2 % 2), min_mb=1)
            c["staged"] = mode == "staged" or (mode == "auto" and nbytes >= MiB)
            c["id"] = "%s-%s-c%d-t%d-%s-%s%s-%d" % (mode, d, chunk_mb, n, count or "x", kind, ("+%d" % r) if kind == "class" else "", nbytes)
            out.append(c)

    # A. staged: every chunk size x every count x every tail kind; the thread count rotates (7 counts against 6 thread counts:
    #    every thread count meets every count and every tail kind)
    i = 0
    for chunk_mb in CHUNKS_MB:
        for kind in ("8", "alone", "full", "ragged"):
            for count in cnt:
                n = THREADS[i % len(THREADS)]
                tail = tail_length(kind, chunk_mb * MiB, n, consts)
                if tail is None:
                    continue
                add("staged", chunk_mb, n, count, kind, tail)
                i += 1
    # B. the tails 4096 n j + r of the cell's own n: r = 8 where n >= 9 (Float64 vectors, byte tables), r = 4 (int tables), r = 1
    for n in THREADS:
        for r in (1, 4, 8):
            for mode, chunk_mb, count in (("staged", 2, "one"), ("staged", 2, "reuse"), ("staged", 3, "two"), ("auto", 3, "lookahead")):
                tail = tail_length("class", chunk_mb * MiB, n, consts, r)
                if tail is not None:
                    add(mode, chunk_mb, n, count, "class", tail, r)
    # C. plain, register, auto: every chunk size x every count, tail kind and thread count rotating
    for mode in ("plain", "register", "auto"):
        i = 0
        for chunk_mb in CHUNKS_MB:
            for count in cnt:
                n = THREADS[(i + 2) % len(THREADS)]
                kinds = [k for k in ("8", "alone", "full", "ragged", "class") if tail_length(k, chunk_mb * MiB, n, consts) is not None]
                kind = kinds[i % len(kinds)]
                add(mode, chunk_mb, n, count, kind, tail_length(kind, chunk_mb * MiB, n, consts), 8 if kind == "class" else 0)
                i += 1
    # D. byte counts that are multiples of 4 and not of 8 (the tables are int lists), and odd ones
    odd = (1, 4, 12, 4097, MiB + 1, MiB + 4, 3 * MiB + 12345, 5 * MiB + 12, 5 * MiB - 4, 9 * MiB - 1)
    for mode, n in (("staged", 3), ("staged", 16), ("register", 7), ("plain", 1), ("auto", 12)):
        for nbytes in odd:
            add(mode, 1, n, None, "odd", None, nbytes=nbytes)
    assert len({c["id"] for c in out}) == len(out)
    return out


# ---- the shim ----
_vp, _i, _sz = C.c_void_p, C.c_int, C.c_size_t
SHIM_PROTOTYPES = {
    "xf_addr_of_sd_device_count": (_vp, []),
    "xf_h2d": (_i, [_vp, _vp, _vp, _sz]),
    "xf_d2h": (_i, [_vp, _vp, _vp, _sz]),
    "xf_release": (None, [_vp]),
}


def build_shim(pkg, outdir):
    """tests/xfer_shim.cpp compiled with the host compiler and linked against the library the package has loaded -> the ctypes
    handle.  A compile or link failure is an assertion failure; so is a shim bound to another instance of the library."""
    pkg.lib()                                                              # libspindyn.so is loaded first
    lib_path = os.path.abspath(pkg._lib.LIB_PATH)
    libdir, out = os.path.dirname(lib_path), os.path.join(str(outdir), "libxfer_shim.so")
    cmd = ["g++", "-std=c++17", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror", os.path.join(ROOT, "tests", "xfer_shim.cpp"),
           "-o", out, "-L", libdir, "-l:" + os.path.basename(lib_path), "-Wl,-rpath," + libdir, "-Wl,--no-undefined"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    shim = C.CDLL(out)
    for name, (res, args) in SHIM_PROTOTYPES.items():
        fn = getattr(shim, name)
        fn.restype, fn.argtypes = res, args
    seen_by_package = C.cast(pkg.lib().sd_device_count, C.c_void_p).value
    assert shim.xf_addr_of_sd_device_count() == seen_by_package, "the shim is bound to another instance of libspindyn.so"
    return shim
