"""sd_xfer_h2d / sd_xfer_d2h (csrc/xfer.cpp) at arbitrary byte counts, through tests/xfer_shim.cpp: every host-pointer entry of the C
ABI moves its vectors and tables through these two functions.  Every comparison is on bytes under ==; nothing has a tolerance.

Buffers.  Host: numpy uint8 between two guards of 4096 bytes of 0xA5, the data 0 or 8 bytes past a page boundary.  Device: a torch
uint8 tensor between two guards of 256 bytes.  The source is a position-dependent pattern (tests/xfer_ref.py), the destination
holds the pattern's complement, so a byte that nobody copied is a wrong byte.  The device side is written and read back with
torch's own copies, which do not pass through xfer.cpp.  After each transfer: the destination equals the source, the guards on
both sides are intact, the source is unchanged.

Constants.  NBUF, the team's 1 MiB threshold and the 16 / 32 MiB defaults are read from the sources; every cell first asserts the
edge it is there to cross (xfer_ref.assert_edge).

The grid (xfer_ref.cells), both directions, SD_XFER_MIN_MB = 1, chunk sizes 1, 2, 3 MiB, 1, 2, 3, 7, 12, 16 threads, at most 27 MiB:
  A  staged: every chunk size x 1, 2, 3 (= NBUF - 1, the look-ahead of a device-to-host copy), 4, 5 (the first reuse of a ring
     slot), 8, 9 chunks x last chunk of 8 bytes, 1 MiB - 8 (the caller's own memcpy), one whole chunk, 1 MiB + 8 (at 2 and 3 MiB);
  B  last chunks 4096 n j + r >= 1 MiB of the cell's own thread count n, r = 8 (n >= 9), 4 and 1: the lengths whose last r bytes
     no member of the team copied while the slice length was (bytes / n) rounded up to a page;
  C  plain, register and auto over every chunk size x every count;
  D  byte counts that are multiples of 4 and not of 8, and odd ones.
Each cell releases the context's scratch first: SD_XFER_THREADS is read when the ring is built, and the team lives and dies with
the ring (test_thread_count_is_read_when_the_ring_is_built asserts that off the source).

Sequences on one context without a release: h2d then d2h three times (the ring's events reused across calls), sizes down and up, a
new chunk size and thread count between calls (ring and team rebuilt), auto below SD_XFER_MIN_MB between two staged calls.

Stream order: the context on a torch side stream; a fill of the device buffer queued on that stream behind other work and
sd_xfer_d2h called at once must deliver the fill (xfer.cpp: the DMA is queued on the producer's stream); the reverse, h2d and then a
torch read on that stream.

The public API: apply_H on host arrays against sd_apply_dev on the same bits at L = 22, nup = 11, Float64 and ComplexF64, 1, 3 and
16 threads, chunks of 1 and 3 MiB.

Measured on one MI355X: 460 grid cells, 487 tests, 4.8 s for the file (1.7 s of it the module's set-up: shim, pattern, arenas); the
slowest cell 0.10 s (the first one, which warms the runtime up), 0.05 s after it (staged d2h, 1 MiB chunks, 12 threads, 5 chunks)."""
import numpy as np
import pytest

import xfer_ref as XR

pytestmark = pytest.mark.gpu

MiB = XR.MiB
CONSTS = XR.constants()
CELLS = XR.cells(CONSTS)


class Env:
    """one context of its own, the shim, the pattern on both sides, the arenas"""

    def __init__(self, pkg, tmpdir):
        import torch
        self.torch, self.pkg = torch, pkg
        self.shim = XR.build_shim(pkg, tmpdir)
        self.ctx = pkg._lib.Context(0)
        self.dev = torch.device("cuda", 0)
        self.pat = XR.pattern()
        self.dpat = torch.as_tensor(np.array(self.pat), device=self.dev)
        self.darena = torch.empty(XR.MAX_BYTES + 2 * XR.DEV_GUARD, dtype=torch.uint8, device=self.dev)
        self.hsrc, self.hdst = XR.HostArena(), XR.HostArena()

    def device_place(self, nbytes, fill):
        """guard | body | guard at the head of the device arena; body = fill (a device tensor of nbytes) -> body, whole"""
        G = XR.DEV_GUARD
        whole = self.darena[:nbytes + 2 * G]
        whole[:G] = XR.GUARD_BYTE
        whole[G + nbytes:] = XR.GUARD_BYTE
        body = whole[G:G + nbytes]
        body.copy_(fill)
        return body, whole

    def setenv(self, mp, mode, chunk_mb, threads, min_mb=1):
        mp.setenv("SD_XFER", mode)
        mp.setenv("SD_XFER_CHUNK_MB", str(chunk_mb))
        mp.setenv("SD_XFER_THREADS", str(threads))
        mp.setenv("SD_XFER_MIN_MB", str(min_mb))

    def h2d(self, nbytes, off, shift, what):
        torch, G = self.torch, XR.DEV_GUARD
        want = self.pat[shift:shift + nbytes]
        src, hguards = self.hsrc.place(nbytes, off)
        src[:] = want
        body, whole = self.device_place(nbytes, ~self.dpat[shift:shift + nbytes])
        torch.cuda.synchronize()
        rc = self.shim.xf_h2d(self.ctx.h, body.data_ptr(), src.ctypes.data, nbytes)
        assert rc == 0, (what, rc, self.pkg.lib().sd_last_error(self.ctx.h))
        got = whole.cpu().numpy()
        bad = XR.mismatch(got[G:G + nbytes], want)
        assert bad is None, "%s: device destination: %s" % (what, bad)
        assert XR.guards_intact((got[:G], got[G + nbytes:])), "%s: device guard overwritten" % what
        assert XR.mismatch(src, want) is None and XR.guards_intact(hguards), "%s: host source or its guards changed" % what

    def d2h(self, nbytes, off, shift, what):
        torch, G = self.torch, XR.DEV_GUARD
        want = self.pat[shift:shift + nbytes]
        dst, hguards = self.hdst.place(nbytes, off)
        np.invert(want, out=dst)
        body, whole = self.device_place(nbytes, self.dpat[shift:shift + nbytes])
        torch.cuda.synchronize()
        rc = self.shim.xf_d2h(self.ctx.h, dst.ctypes.data, body.data_ptr(), nbytes)
        assert rc == 0, (what, rc, self.pkg.lib().sd_last_error(self.ctx.h))
        bad = XR.mismatch(dst, want)
        assert bad is None, "%s: host destination: %s" % (what, bad)
        assert XR.guards_intact(hguards), "%s: host guard overwritten" % what
        after = whole.cpu().numpy()
        assert XR.mismatch(after[G:G + nbytes], want) is None and XR.guards_intact((after[:G], after[G + nbytes:])), \
            "%s: device source or its guards changed" % what

    def move(self, direction, nbytes, off, shift, what):
        (self.h2d if direction == "h2d" else self.d2h)(nbytes, off, shift, what)


@pytest.fixture(scope="module")
def env(pkg, tmp_path_factory):
    e = Env(pkg, tmp_path_factory.mktemp("xfer_shim"))
    yield e
    e.ctx.close()


def test_constants_are_the_ones_the_grid_was_laid_out_for():
    assert CONSTS == {"NBUF": 4, "TEAM_MIN": MiB, "MIN_MB": 16, "CHUNK_MB": 32, "MAX_THREADS": 16}
    assert max(c["bytes"] for c in CELLS) == 27 * MiB and max(c["threads"] for c in CELLS) == 16
    for mode in ("plain", "staged", "register", "auto"):
        for d in ("h2d", "d2h"):
            mine = [c for c in CELLS if c["mode"] == mode and c["dir"] == d]
            assert {c["chunk_mb"] for c in mine} == set(XR.CHUNKS_MB) and {c["threads"] for c in mine} >= {1, 7, 12, 16}
            assert {c["count"] for c in mine if c["count"]} == set(XR.counts(CONSTS["NBUF"]))
    staged = [c for c in CELLS if c["mode"] == "staged"]
    assert {c["threads"] for c in staged} == set(XR.THREADS)
    assert {(c["kind"], c["chunk_mb"]) for c in staged} >= {(k, m) for k in ("8", "alone", "full") for m in XR.CHUNKS_MB} | {
        ("ragged", 2), ("ragged", 3), ("class", 2), ("class", 3)}
    assert {(c["threads"], c["r"]) for c in CELLS if c["kind"] == "class"} >= {(12, 8), (16, 8), (12, 4), (7, 4), (2, 1), (3, 1), (16, 1)}


def test_thread_count_is_read_when_the_ring_is_built():
    facts = XR.team_lifetime_facts()
    assert all(facts.values()), facts


@pytest.mark.parametrize("cell", CELLS, ids=[c["id"] for c in CELLS])
def test_grid(env, monkeypatch, cell):
    XR.assert_edge(cell, CONSTS)
    env.ctx.release_scratch()                         # the next staged call builds ring and team anew, with this cell's thread count
    env.setenv(monkeypatch, cell["mode"], cell["chunk_mb"], cell["threads"], cell["min_mb"])
    env.move(cell["dir"], cell["bytes"], cell["off"], 1 + cell["bytes"] % 4099, cell["id"])


def test_zero_bytes_touch_nothing(env, monkeypatch):
    for mode in ("plain", "staged", "register", "auto"):
        env.setenv(monkeypatch, mode, 1, 3)
        env.move("h2d", 0, 0, 0, mode)
        env.move("d2h", 0, 8, 0, mode)


def test_there_and_back_three_times_on_one_ring(env, monkeypatch):
    """5 chunks + 8 bytes through a ring of NBUF = 4, in and out, three times: every call after the first finds the events of the
    ring recorded by the call before it"""
    env.ctx.release_scratch()
    env.setenv(monkeypatch, "staged", 1, 7)
    nbytes = (CONSTS["NBUF"] + 1) * MiB + 8
    assert -(-nbytes // MiB) == CONSTS["NBUF"] + 2
    for k in range(3):
        env.h2d(nbytes, 8 * (k % 2), 17 + k, "h2d #%d" % k)
        env.d2h(nbytes, 8 * (k % 2), 4001 + k, "d2h #%d" % k)


@pytest.mark.parametrize("direction", ["h2d", "d2h"])
def test_sizes_down_and_up_on_one_ring(env, monkeypatch, direction):
    env.ctx.release_scratch()
    env.setenv(monkeypatch, "staged", 2, 12)
    sizes = [18 * MiB, 10 * MiB + 8, 6 * MiB, XR.class_length(12, 8, MiB), MiB - 8, 8, 1, MiB + 4, 4 * MiB, 8 * MiB + MiB + 8, 16 * MiB]
    assert [-(-s // (2 * MiB)) for s in sizes] == [9, 6, 3, 1, 1, 1, 1, 1, 2, 5, 8]
    for k, s in enumerate(sizes):
        env.move(direction, s, 8 * (k % 2), 3 * k + 1, "%s of %d bytes (#%d)" % (direction, s, k))


def test_new_chunk_size_rebuilds_ring_and_team(env, monkeypatch):
    """no release between the calls: a new SD_XFER_CHUNK_MB alone makes ensure_ring drop ring and team, and the new team has the
    thread count of its own call -- the last chunk is 4096 n j + 8 of that n"""
    env.ctx.release_scratch()
    for k, (chunk_mb, n) in enumerate([(2, 16), (3, 12), (2, 9), (3, 16), (2, 1), (3, 13)]):
        assert n <= CONSTS["MAX_THREADS"]
        env.setenv(monkeypatch, "staged", chunk_mb, n)
        tail = XR.class_length(n, 8, MiB) if n >= 9 else MiB + 8
        assert MiB <= tail < chunk_mb * MiB
        nbytes = (CONSTS["NBUF"] + 1) * chunk_mb * MiB + tail
        env.h2d(nbytes, 0, k + 1, "h2d chunk %d MiB, %d threads" % (chunk_mb, n))
        env.d2h(nbytes, 8, k + 2, "d2h chunk %d MiB, %d threads" % (chunk_mb, n))
    env.shim.xf_release(env.ctx.h)                    # the shim's own release: the next call starts from nothing
    env.setenv(monkeypatch, "staged", 3, 2)
    env.d2h(7 * MiB + 1, 0, 5, "d2h after xf_release")


@pytest.mark.parametrize("direction", ["h2d", "d2h"])
def test_auto_below_the_minimum_between_two_staged_calls(env, monkeypatch, direction):
    env.ctx.release_scratch()
    big, small = 9 * MiB + 8, 3 * MiB + 4
    env.setenv(monkeypatch, "auto", 2, 3, min_mb=4)
    assert small < 4 * MiB <= big
    env.move(direction, big, 0, 1, "staged, first")
    env.move(direction, small, 8, 2, "plain, between")   # the ring stays as it is
    env.move(direction, big, 0, 3, "staged, second")


@pytest.mark.parametrize("mode", ["staged", "plain", "register"])
def test_d2h_is_ordered_behind_the_producer_on_the_stream(env, monkeypatch, mode):
    """the context on a torch side stream: work is queued on that stream, the fill of the device buffer behind it, and sd_xfer_d2h is
    called at once -- the host must receive the fill, not what the buffer held before"""
    torch = env.torch
    nbytes, shift, G = 6 * MiB + 8, 77, XR.DEV_GUARD
    want = env.pat[shift:shift + nbytes]
    env.ctx.release_scratch()
    env.setenv(monkeypatch, mode, 1, 3)
    dst, hguards = env.hdst.place(nbytes, 8)
    np.invert(want, out=dst)
    body, whole = env.device_place(nbytes, ~env.dpat[shift:shift + nbytes])       # before the fill: the complement
    ballast = torch.zeros(64 * MiB, dtype=torch.uint8, device=env.dev)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=env.dev)
    env.ctx.set_stream(side.cuda_stream)
    try:
        with torch.cuda.stream(side):
            for _ in range(24):
                ballast.add_(1)                                                   # the fill waits behind these
            body.copy_(env.dpat[shift:shift + nbytes])
        rc = env.shim.xf_d2h(env.ctx.h, dst.ctypes.data, body.data_ptr(), nbytes)
    finally:
        env.ctx.set_stream(None)
    assert rc == 0
    bad = XR.mismatch(dst, want)
    assert bad is None, "the copy overtook its producer: %s" % bad
    assert XR.guards_intact(hguards)
    side.synchronize()
    assert int(ballast[0]) == 24 and int(ballast[-1]) == 24


@pytest.mark.parametrize("mode", ["staged", "plain", "register"])
def test_h2d_then_a_read_on_the_same_stream(env, monkeypatch, mode):
    torch = env.torch
    nbytes, shift = 6 * MiB + 8, 91
    want = env.pat[shift:shift + nbytes]
    env.ctx.release_scratch()
    env.setenv(monkeypatch, mode, 1, 3)
    src, hguards = env.hsrc.place(nbytes, 8)
    src[:] = want
    body, whole = env.device_place(nbytes, ~env.dpat[shift:shift + nbytes])
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=env.dev)
    env.ctx.set_stream(side.cuda_stream)
    try:
        with torch.cuda.stream(side):
            rc = env.shim.xf_h2d(env.ctx.h, body.data_ptr(), src.ctypes.data, nbytes)
            seen = whole.clone()                                                  # a consumer on the same stream
        side.synchronize()
    finally:
        env.ctx.set_stream(None)
    assert rc == 0
    got = seen.cpu().numpy()
    G = XR.DEV_GUARD
    bad = XR.mismatch(got[G:G + nbytes], want)
    assert bad is None, bad
    assert XR.guards_intact((got[:G], got[G + nbytes:])) and XR.guards_intact(hguards) and XR.mismatch(src, want) is None


# ---- the public API: apply_H on host arrays against sd_apply_dev on the same bits ----
@pytest.fixture(scope="module")
def flagship_sector(pkg):
    """L = 22, nup = 11: the model, psi and sd_apply_dev's H psi for both element types, computed once"""
    import torch
    m = pkg.XXZChain(22, nup=11)
    rng = np.random.default_rng(5)
    re, im = rng.standard_normal(m.N), rng.standard_normal(m.N)
    out = {}
    for name, psi in (("f64", re), ("c128", re + 1j * im)):
        tp = torch.as_tensor(psi, device=torch.device("cuda", m.ctx.device))
        th = torch.empty_like(tp)
        pkg.apply_H(th, tp, m)
        psi.setflags(write=False)
        want = th.cpu().numpy()
        want.setflags(write=False)
        out[name] = (psi, want)
    return m, out


@pytest.mark.parametrize("chunk_mb", [1, 3])
@pytest.mark.parametrize("threads", [1, 3, 16])
@pytest.mark.parametrize("name", ["f64", "c128"])
def test_apply_H_on_host_arrays_is_the_device_apply(pkg, flagship_sector, monkeypatch, name, threads, chunk_mb):
    m, vectors = flagship_sector
    psi, want = vectors[name]
    assert psi.nbytes > chunk_mb * MiB >= CONSTS["TEAM_MIN"]                      # staged, more than one chunk, the team at work
    m.ctx.release_scratch()
    for k, v in (("SD_XFER", "staged"), ("SD_XFER_MIN_MB", "1"), ("SD_XFER_CHUNK_MB", str(chunk_mb)), ("SD_XFER_THREADS", str(threads))):
        monkeypatch.setenv(k, v)
    keep = psi.copy()
    out = np.empty_like(psi)
    pkg.apply_H(out, psi, m)
    assert np.array_equal(out.view(np.uint8), want.view(np.uint8))
    pkg.apply_H(out, psi, m)                                                      # the same ring, reused pages
    assert np.array_equal(out.view(np.uint8), want.view(np.uint8)) and np.array_equal(psi, keep)
    m.ctx.release_scratch()
