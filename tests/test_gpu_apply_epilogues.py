"""Every fused apply epilogue on every launch form of sd_launch_apply (csrc/kernels_apply.hip), element by element against the numpy
restatement of tests/epilogue_ref.py (proven on the CPU by tests/test_epilogue_ref_host.py) fed with the ORACLE's H psi.

Entry points (public C ABI, unsharded model, halo = NULL, part = 0):
  sd_apply_sharded_dev        epilogue 0 PLAIN, 1 RESCALE, 3 RECUR (Float64 and ComplexF64), 2 CHEB (ComplexF64; Float64 is refused)
  sd_apply_sharded_cheb2_dev  CHEB2 (ComplexF64)
  sd_kpm_step_sharded_dev     first = 1 RESCALE_DOT, first = 0 KPM (ComplexF64), each with a phi vector and with phi = NULL
  lanczos_tridiag / lanczos_extremal   DOT (and PLAIN / DOT with negate): the only public route to them
Not reachable through the public ABI, and so not here: the Float64 sum epilogues (DOT, RESCALE_DOT, KPM) and Float64 CHEB / CHEB2.

Cells (23).  XXZ with Jxy = 0.9, Jz = 0.7, hz = 0.3; "-pow2": Jxy = Jz = 1 (hop amplitude 0.5: the multiply-add accumulation).
  C, C-pow2                 L=16 nup=8 open, default plan: one class launch; Float64 takes the 8-rows-per-thread form
  P-20-10, P-20-7, P-18-9-b10, P-18-9-b11, each also -pow2
                            SD_LEN_CLASSES=2, open chain: ComplexF64 takes the packed launch, Float64 the split class launches
  W-16-8, W-20-7, each also -split (SD_LEN_CLASSES=2: classes split, no packing)
                            periodic chain: wrap bond, second LDS image
  G-open, G-periodic, G-open-rows (SD_GEN_PLAN=0)
                            J1-J2 lists on L=16 nup=8: the general-bond plan, and its per-row form
  B13                       L=16 nup=8, SD_SUFFIX_BITS=13: binomial partners, the large workgroups
  S                         L=18 nup=5, SD_SHORT_TILES=1, SD_SUFFIX_BITS=10: k_apply_short<.,16> and <.,1>
  F                         L=12 full basis: k_apply_fulltile, 4 tiles of 1024 rows
  R-20-3, R-22-19           L=20 nup=3 open, L=22 nup=19 periodic: k_apply_generic
  X                         L=23 nup=11 open, SD_SUFFIX_BITS=8: 32 071 tiles (> 16 384 partial pairs: k_reduce_pairs_stage) and
                            1 352 078 rows (> 4096 * 256: k_epilogue_only wraps)
Tests: 23 vector cells + 23 sum cells + 23 DOT cells + the Float64 refusal + 2 user-operator evolutions + the user-operator moments
= 73.

What this file cannot see.  Nothing exported tells WHICH launch ran: `device_path` is "tiled" for the class launches, the packed
launch and the short-tile kernels alike.  Each cell asserts what the launcher's choice rests on (path, tile lengths, tile and row
counts); that the P cells take the packed launch rests on the eligibility rule of sd_build_plan / sd_upload_model (unsharded,
packed partner tables i.e. at most 12 suffix bits, chain bonds only -- no wrap bond, no general-bond plan --, classes split,
which SD_LEN_CLASSES=2 forces, and ComplexF64), the limit tests/test_gpu_apply_packed.py states for itself.  Tile indices in the
messages and probe choices are those of Model.local_tiles(); the kernels visit the tiles in their own (XCD) order.

All vectors are seeded random, psi normalised on the host; a, b, c, c0 have no power-of-two value, so every rounding happens.
out and psi_t carry 32 NaN guard elements on each side and are NaN-filled before every call.  Exact means exact: real and
imaginary parts as separate IEEE doubles under ==."""
import ctypes as C
import gc
import math

import numpy as np
import pytest

import epilogue_ref as ER

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 32
A, B, C1, C0 = 4.3, -0.7, 0.3 - 0.2j, -0.11 + 0.23j
# constants of the launchers (csrc/kernels_apply.hip)
PAIRS_ONE_STAGE = 16384            # sd_reduce_pairs: more partial pairs than this go through k_reduce_pairs_stage first
EPI_ONLY_BLOCKS = 4096             # sd_launch_epilogue_only: at most 4096 blocks of 256 rows
GENERIC_BLOCK = 256                # k_apply_generic / k_epilogue_only: rows per block
FULL_TILE = 1024                   # k_apply_fulltile: 2^10 rows per tile (full_ls = 10)
SLOT_ROWS = 256                    # packed launch: rows per wave slot, four slots per workgroup
SHORT_ROWS = 16                    # k_apply_short: tiles of at most 16 rows


def j1j2(L, periodic, J1=1.0, J2=0.4):
    hop, zz = [], []
    for d, J in ((1, J1), (2, J2)):                            # the chain bonds first, in order: they keep their own form
        for i in range(1, L + 1):
            j = i + d
            if j > L:
                if not periodic:
                    continue
                j -= L
            hop.append((i, j, 0.5 * J))
            zz.append((i, j, J))
    return hop, zz, np.full(L, 0.1)


def spec(L, nup, bc="open", pow2=False, env=(), path="tiled", lists=None):
    return dict(L=L, nup=nup, bc=bc, pow2=pow2, env=dict(env), path=path, lists=lists)


SPECS = {"C": spec(16, 8), "C-pow2": spec(16, 8, pow2=True)}
for _L, _nup, _bits in ((20, 10, None), (20, 7, None), (18, 9, "10"), (18, 9, "11")):      # the shapes of test_gpu_apply_packed.py
    for _p2 in (False, True):
        _env = {"SD_LEN_CLASSES": "2"} if _bits is None else {"SD_LEN_CLASSES": "2", "SD_SUFFIX_BITS": _bits}
        SPECS[f"P-{_L}-{_nup}" + (f"-b{_bits}" if _bits else "") + ("-pow2" if _p2 else "")] = spec(_L, _nup, pow2=_p2, env=_env)
for _L, _nup in ((16, 8), (20, 7)):
    SPECS[f"W-{_L}-{_nup}"] = spec(_L, _nup, bc="periodic")
    SPECS[f"W-{_L}-{_nup}-split"] = spec(_L, _nup, bc="periodic", env={"SD_LEN_CLASSES": "2"})
SPECS.update({
    "G-open": spec(16, 8, lists="open"),
    "G-periodic": spec(16, 8, lists="periodic"),
    "G-open-rows": spec(16, 8, lists="open", env={"SD_GEN_PLAN": "0"}),
    "B13": spec(16, 8, env={"SD_SUFFIX_BITS": "13"}),
    "S": spec(18, 5, env={"SD_SHORT_TILES": "1", "SD_SUFFIX_BITS": "10"}),
    "F": spec(12, None, path="full-tiled"),
    "R-20-3": spec(20, 3, path="generic"),
    "R-22-19": spec(22, 19, bc="periodic", path="generic"),
    "X": spec(23, 11, env={"SD_SUFFIX_BITS": "8"}),
})
CELLS = list(SPECS)
assert len(CELLS) == 23
PLAN_ENV = ("SD_LEN_CLASSES", "SD_SUFFIX_BITS", "SD_SHORT_TILES", "SD_GEN_PLAN")

_refs = {}


def reference(O, sp):
    """the oracle's H psi for the model of a spec (the plan's environment does not enter): psi normalised, H psi for the complex
    and for a real vector; computed once per model and never modified"""
    key = (sp["L"], sp["nup"], sp["bc"], sp["pow2"], sp["lists"])
    if key not in _refs:
        L, nup = sp["L"], sp["nup"]
        if sp["lists"] is not None:
            hop, zz, field = j1j2(L, sp["lists"] == "periodic")
            r = O.build_model(L, nup=nup, hopping=hop, onsite_field=field, zz=zz)
        else:
            J = (1.0, 1.0) if sp["pow2"] else (0.9, 0.7)
            r = O.XXZChain(L, Jxy=J[0], Jz=J[1], hz=0.3, nup=nup, boundary=sp["bc"])
        rng = np.random.default_rng(1000 * L + (nup or 0))
        v = {}
        for k in ("psi", "prev", "phi", "psi_t"):
            v[k + "_c"] = rng.standard_normal(r.N) + 1j * rng.standard_normal(r.N)
            v[k + "_r"] = rng.standard_normal(r.N)
        v["psi_c"] /= np.linalg.norm(v["psi_c"])
        v["psi_r"] /= np.linalg.norm(v["psi_r"])
        v["h_c"] = O.apply_H(r, v["psi_c"])
        v["h_r"] = O.apply_H(r, v["psi_r"])
        assert v["h_c"].dtype == np.complex128 and v["h_r"].dtype == np.float64
        for x in v.values():
            x.setflags(write=False)
        _refs[key] = v
    return _refs[key]


class Cell:
    """the library's model of one cell, what makes it the form it claims to be, and the reference vectors on the device"""

    def __init__(self, pkg, O, name):
        import torch
        self.name, sp = name, SPECS[name]
        self.L, self.nup = sp["L"], sp["nup"]
        with pytest.MonkeyPatch.context() as mp:              # the plan reads its environment when the model is built
            for k in PLAN_ENV:
                mp.delenv(k, raising=False)
            for k, x in sp["env"].items():
                mp.setenv(k, x)
            if sp["lists"] is not None:
                hop, zz, field = j1j2(self.L, sp["lists"] == "periodic")
                self.m = pkg.build_model(self.L, nup=self.nup, hopping=hop, zz=zz, onsite_field=field)
            else:
                J = (1.0, 1.0) if sp["pow2"] else (0.9, 0.7)
                self.m = pkg.XXZChain(self.L, Jxy=J[0], Jz=J[1], hz=0.3, nup=self.nup, boundary=sp["bc"])
        m = self.m
        self.N = m.N
        assert m.device_path == sp["path"], (name, m.device_path)
        self.tiles = None
        if sp["path"] == "tiled":
            lb, gb, ln = m.local_tiles()
            assert np.array_equal(lb, gb) and int(ln.sum()) == m.N    # one device holds the whole sector
            self.tiles = (gb, ln)
        self.assert_form()
        self.ref = reference(O, sp)
        assert len(self.ref["psi_c"]) == m.N
        self.dev = torch.device("cuda", m.ctx.device)
        self.d = {k: torch.from_numpy(np.array(x)).to(self.dev) for k, x in self.ref.items() if not k.startswith("h_")}

    def assert_form(self):
        """what the launcher's choice rests on, from the plan itself"""
        name, m = self.name, self.m
        kind = name.split("-")[0]
        if self.tiles is not None:
            ln = self.tiles[1]
        if kind == "C":
            assert ln.max() == math.comb(12, 6) and len(ln) < 32768          # 12 suffix bits; classes split from 32768 tiles on only
        elif kind == "P":
            # packed launch: open chain (no wrap bond, no general bond), <= 12 suffix bits, every tile within four slots
            assert all(j == i + 1 for i, j, _ in m.hopping_list) and ln.max() <= 4 * SLOT_ROWS
            assert ln.max() <= math.comb(12, 6) and (ln > SHORT_ROWS).any()
        elif kind == "W":
            assert (self.L, 1) in [(i, j) for i, j, _ in m.hopping_list] and ln.max() <= math.comb(12, 6)
        elif kind == "G":
            assert any(abs(i - j) not in (1,) for i, j, _ in m.hopping_list) and ln.max() <= math.comb(12, 6)
        elif kind == "B13":
            assert ln.max() == math.comb(13, 6)                              # 13 suffix bits: no packed partner table
        elif kind == "S":
            assert (ln == 1).any() and ((ln >= 2) & (ln <= SHORT_ROWS)).any() and (ln > SHORT_ROWS).any()
        elif kind == "F":
            assert m.N == 4 * FULL_TILE
        elif kind == "R":
            assert m.N > GENERIC_BLOCK                                       # more than one block
        elif kind == "X":
            assert len(ln) > PAIRS_ONE_STAGE and m.N > EPI_ONLY_BLOCKS * GENERIC_BLOCK
            assert len(ln) == 32071 and m.N == 1352078

    def tile_of(self, rows):
        if self.tiles is None:
            return None
        order = np.argsort(self.tiles[0])
        return order[np.searchsorted(self.tiles[0][order], np.asarray(rows), side="right") - 1].tolist()

    def probe_rows(self):
        """rows whose sums a misfiled partial pair or a short reduction would lose: see the module docstring's cells"""
        N, kind = self.N, self.name.split("-")[0]
        rows = [0, N - 1]
        if self.tiles is None:
            blk = FULL_TILE if kind == "F" else GENERIC_BLOCK
            last = (N - 1) // blk * blk                                      # first row of the last block
            assert last > 0
            rows += [blk - 1, blk, last - 1, last, last + (N - 1 - last) // 2]
            return sorted(set(rows))
        gb, ln = self.tiles
        nt = len(gb)

        def of(t, offsets):
            return [int(gb[t]) + o for o in offsets if 0 <= o < int(ln[t])]
        for t in (0, nt - 1, nt // 2):
            rows += of(t, (0, int(ln[t]) - 1))
        if kind == "P":
            slots = (ln + SLOT_ROWS - 1) // SLOT_ROWS
            present = sorted(set(slots.tolist()))
            if self.name.startswith(("P-20-10", "P-20-7")):
                assert present == [1, 2, 4]
            for k in present:
                ts = np.nonzero(slots == k)[0]
                for t in (ts[0], ts[len(ts) // 2], ts[-1]):
                    # in multi-slot tiles a row of each later wave of the team: in-tile offsets >= 256
                    later = of(t, tuple(SLOT_ROWS * s + 3 for s in range(1, k)))
                    assert len(later) == k - 1
                    rows += of(t, (0, 70, int(ln[t]) - 1)) + later
        elif kind == "S":
            ones, multi = np.nonzero(ln == 1)[0], np.nonzero((ln >= 2) & (ln <= SHORT_ROWS))[0]
            for ts in (ones, multi):
                for t in (ts[0], ts[len(ts) // 2], ts[-1]):
                    rows += of(t, (0, 1, int(ln[t]) - 1))
        elif kind == "X":
            for t in (PAIRS_ONE_STAGE - 1, PAIRS_ONE_STAGE, PAIRS_ONE_STAGE + 1, 20000, 25001, nt - 2):
                rows += of(t, (0, int(ln[t]) // 2))
            assert max(self.tile_of(rows)) > PAIRS_ONE_STAGE
        else:
            long = np.nonzero(ln > 64)[0]                                    # a row of a later wave of the workgroup
            rows += of(long[len(long) // 2], (64, int(ln[long[len(long) // 2]]) - 1))
        return sorted(set(rows))


class Cells:
    def __init__(self, pkg, O):
        self.pkg, self.O, self.store = pkg, O, {}

    def get(self, name):
        if name not in self.store:
            if len(self.store) > 3:                            # tests run cell by cell: keep a few, not all 23
                self.store.clear()
                gc.collect()
            self.store[name] = Cell(self.pkg, self.O, name)
        return self.store[name]


@pytest.fixture(scope="module")
def cells(pkg, O):
    import torch
    st = Cells(pkg, O)
    yield st
    st.store.clear()
    _refs.clear()
    gc.collect()
    torch.cuda.empty_cache()


# ---- buffers the caller owns: NaN-filled, 32 guard elements on each side ----
class Guarded:
    def __init__(self, N, cplx, dev):
        import torch
        self.N = N
        self.buf = torch.empty(N + 2 * GUARD, dtype=torch.complex128 if cplx else torch.float64, device=dev)
        self.inner = self.buf[GUARD:GUARD + N]
        assert self.inner.data_ptr() % 16 == 0
        self.fill_nan()

    def raw(self):
        import torch
        return torch.view_as_real(self.buf) if self.buf.is_complex() else self.buf

    def fill_nan(self):
        self.raw().fill_(NAN)

    def load(self, x):
        self.fill_nan()
        self.inner.copy_(x)

    def guards_are_nan(self):
        import torch
        raw = self.raw()
        return bool(torch.isnan(raw[:GUARD]).all()) and bool(torch.isnan(raw[GUARD + self.N:]).all())

    def host(self):
        return self.inner.cpu().numpy()


def bits_equal(a, b):
    """real and imaginary parts as separate doubles under =="""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if np.iscomplexobj(a):
        return bool(np.all(a.real == b.real) and np.all(a.imag == b.imag))
    return bool(np.all(a == b))


def differing(cell, what, got, want):
    """form, epilogue, dtype and stream, and which rows differ: count, the first rows and their tiles"""
    bad = (got.real != want.real) | (got.imag != want.imag) if np.iscomplexobj(got) else got != want
    first = np.nonzero(bad)[0][:8].tolist()
    return (f"{cell.name} {what}: {int(bad.sum())} of {cell.N} rows differ; first rows {first}, tiles {cell.tile_of(first)}, "
            f"got {got[first[:2]].tolist()} want {want[first[:2]].tolist()}")


def ptr(x):
    return None if x is None else x.data_ptr()


def bind(cell):
    import torch
    cell.m.ctx.set_stream(torch.cuda.current_stream().cuda_stream)


def call_apply(pkg, cell, cplx, epi_code, out, psi, prev=None, psi_t=None):
    import torch
    m = cell.m
    bind(cell)
    pkg.check(pkg.lib().sd_apply_sharded_dev(m.ctx.h, m.h, pkg._lib.SD_C128 if cplx else pkg._lib.SD_F64, ptr(out), ptr(psi), None,
                                             cell.N, epi_code, A, B, C1.real, C1.imag, ptr(prev), ptr(psi_t), 0), m.ctx.h)
    torch.cuda.synchronize()


def call_cheb2(pkg, cell, out, psi, prev, psi_t):
    import torch
    m = cell.m
    bind(cell)
    pkg.check(pkg.lib().sd_apply_sharded_cheb2_dev(m.ctx.h, m.h, ptr(out), ptr(psi), None, cell.N, A, B, C0.real, C0.imag, C1.real,
                                                   C1.imag, ptr(prev), ptr(psi_t), 0), m.ctx.h)
    torch.cuda.synchronize()


def call_kpm(pkg, cell, out, psi, prev, phi, first):
    """-> the two sums (sd_kpm_step_sharded_dev reads them back: the call is synchronous)"""
    m = cell.m
    bind(cell)
    s = (C.c_double * 2)(NAN, NAN)
    pkg.check(pkg.lib().sd_kpm_step_sharded_dev(m.ctx.h, m.h, ptr(out), ptr(psi), None, ptr(prev), ptr(phi), cell.N, A, B, int(first), s),
              m.ctx.h)
    return float(s[0]), float(s[1])


def inputs_unchanged(cell, sfx, names):
    return [k for k in names if not bits_equal(cell.d[k + sfx].cpu().numpy(), cell.ref[k + sfx])]


# ---- 1. the vector epilogues: out and psi_t bit for bit, inputs untouched, guards intact ----
@pytest.mark.parametrize("name", CELLS)
def test_vector_epilogues_equal_the_reference_bit_for_bit(pkg, cells, name):
    cell = cells.get(name)
    for cplx in (True, False):
        sfx = "_c" if cplx else "_r"
        dt = "c128" if cplx else "f64"
        d, ref = cell.d, cell.ref
        out, acc = Guarded(cell.N, cplx, cell.dev), Guarded(cell.N, cplx, cell.dev)
        cases = [(ER.PLAIN, lambda: call_apply(pkg, cell, cplx, 0, out.inner, d["psi" + sfx])),
                 (ER.RESCALE, lambda: call_apply(pkg, cell, cplx, 1, out.inner, d["psi" + sfx])),
                 (ER.RECUR, lambda: call_apply(pkg, cell, cplx, 3, out.inner, d["psi" + sfx], prev=d["prev" + sfx]))]
        if cplx:
            cases += [(ER.CHEB, lambda: call_apply(pkg, cell, cplx, 2, out.inner, d["psi_c"], prev=d["prev_c"], psi_t=acc.inner)),
                      (ER.CHEB2, lambda: call_cheb2(pkg, cell, out.inner, d["psi_c"], d["prev_c"], acc.inner))]
        for epi, run in cases:
            out.fill_nan()
            acc.load(d["psi_t" + sfx])
            run()
            want, want_t, _, _ = ER.epilogue(epi, ref["h" + sfx], ref["psi" + sfx], a=A, b=B, c=C1, c0=C0, prev=ref["prev" + sfx],
                                             psi_t=ref["psi_t" + sfx])
            got = out.host()
            assert bits_equal(got, want), differing(cell, f"{epi} {dt} out", got, want)
            got_t = acc.host()
            if want_t is None:
                want_t = ref["psi_t" + sfx]                    # not an argument of this epilogue: as loaded
            assert bits_equal(got_t, want_t), differing(cell, f"{epi} {dt} psi_t", got_t, want_t)
            assert out.guards_are_nan() and acc.guards_are_nan(), (name, epi, dt, "guard elements written")
            assert inputs_unchanged(cell, sfx, ("psi", "prev", "phi")) == [], (name, epi, dt)
        assert float(np.abs(want).max()) > 1e-3                # a real comparison, not zeros against zeros


def test_chebyshev_epilogue_on_float64_is_still_refused(pkg, cells):
    cell = cells.get("C")
    out, acc = Guarded(cell.N, False, cell.dev), Guarded(cell.N, False, cell.dev)
    with pytest.raises(pkg.ArgumentError):
        call_apply(pkg, cell, False, 2, out.inner, cell.d["psi_r"], prev=cell.d["prev_r"], psi_t=acc.inner)
    assert bool(np.isnan(out.host()).all()) and bool(np.isnan(acc.host()).all())       # and nothing was launched


# ---- 2. the sum epilogues: out bit for bit, the sums within the summation bound, probes exact ----
def sum_bound(N, terms):
    """worst case of ANY order of N - 1 double additions of these terms: N 2^-53 sum |term_i| (the terms themselves are
    bit-equal to the kernel's, so the order of the additions is all that differs)"""
    return N * 2.0 ** -53 * math.fsum(np.abs(terms).tolist())


@pytest.mark.parametrize("name", CELLS)
def test_sum_epilogues_bound_probes_and_streams(pkg, cells, name):
    import torch
    cell = cells.get(name)
    d, ref = cell.d, cell.ref
    out = Guarded(cell.N, True, cell.dev)
    wants = {}
    for epi, first in ((ER.RESCALE_DOT, 1), (ER.KPM, 0)):
        prev = None if first else d["prev_c"]
        for with_phi in (True, False):
            what = f"{epi} c128 phi={'vector' if with_phi else 'NULL'}"
            want, _, t0, t1 = ER.epilogue(epi, ref["h_c"], ref["psi_c"], a=A, b=B, prev=ref["prev_c"], phi=ref["phi_c"] if with_phi else None)
            wants[epi] = want
            out.fill_nan()
            got = call_kpm(pkg, cell, out.inner, d["psi_c"], prev, d["phi_c"] if with_phi else None, first)
            o = out.host()
            assert bits_equal(o, want), differing(cell, what + " out", o, want)
            assert out.guards_are_nan() and inputs_unchanged(cell, "_c", ("psi", "prev", "phi")) == [], (name, what)
            for k, terms in enumerate((t0, t1)):
                exact, bar = math.fsum(terms.tolist()), sum_bound(cell.N, terms)
                print(f"{name} {what} sum {k}: |got - fsum| = {abs(got[k] - exact):.2e} (bound {bar:.2e}, |sum| {abs(exact):.2e})")
                assert abs(got[k] - exact) <= bar, (name, what, k, got[k], exact, bar)
            out.fill_nan()
            again = call_kpm(pkg, cell, out.inner, d["psi_c"], prev, d["phi_c"] if with_phi else None, first)
            assert got[0].hex() == again[0].hex() and got[1].hex() == again[1].hex(), (name, what)      # same call twice: equal bits
    # probes: phi = e_r picks Re out[r], phi = i e_r picks Im out[r]; every other term of the sum is an exact zero
    rows = cell.probe_rows()
    tiles = cell.tile_of(rows)
    phi = torch.zeros(cell.N, dtype=torch.complex128, device=cell.dev)
    for epi, first in ((ER.RESCALE_DOT, 1), (ER.KPM, 0)):
        prev = None if first else d["prev_c"]
        for i, r in enumerate(rows):
            for unit, part in ((1.0 + 0.0j, "real"), (1.0j, "imag")):
                phi[r] = unit
                got = call_kpm(pkg, cell, out.inner, d["psi_c"], prev, phi, first)
                want = float(getattr(wants[epi][r], part))
                assert got[0] == want, f"{name} {epi} c128 probe {part} row {r} tile {tiles[i] if tiles else None}: got {got[0]!r} want {want!r}"
            phi[r] = 0.0


# ---- 3. DOT, through the Lanczos drivers ----
@pytest.mark.parametrize("name", CELLS)
def test_dot_epilogue_through_the_lanczos_drivers(pkg, cells, name):
    cell = cells.get(name)
    m, ref = cell.m, cell.ref
    _, _, t0, _ = ER.epilogue(ER.DOT, ref["h_c"], ref["psi_c"])
    want = math.fsum(t0.tolist())                              # <psi|H psi> of the oracle's H psi, |psi| = 1
    al, be, nv = pkg.lanczos_tridiag(pkg.apply_H, m, ref["psi_c"], lanc_m=2)
    print(f"{name} alpha_1 - <psi|H psi> = {al[0] - want:.2e}")
    assert len(al) == 2 and abs(nv - 1.0) <= 1e-12
    assert abs(al[0] - want) <= 1e-9, (name, al[0], want)      # the bar of test_packed_sum_epilogue_vs_oracle
    if name.split("-")[0] in ("C", "P"):
        lo, hi = pkg.lanczos_extremal(pkg.apply_H, m, lanc_m=40, psi0=ref["psi_c"], negate=False)
        nlo, nhi = pkg.lanczos_extremal(pkg.apply_H, m, lanc_m=40, psi0=ref["psi_c"], negate=True)
        assert lo < hi and abs(nlo + hi) <= 1e-10 and abs(nhi + lo) <= 1e-10, (name, lo, hi, nlo, nhi)


# ---- 4. k_epilogue_only past its 4096-block cap: a user operator that is the library's own apply ----
def _own_apply(pkg, calls):
    def op(out, psi, model):
        calls.append(len(psi))
        pkg.apply_H(out, psi, model)
    return op


@pytest.mark.parametrize("cheb_n", [4, 5])
def test_epilogue_only_kernel_equals_the_fused_epilogues_in_a_chebyshev_evolution(pkg, cells, cheb_n):
    """RESCALE, RECUR, CHEB2 and (odd number of terms) CHEB through k_epilogue_only on 1 352 078 rows: the vector epilogues have no
    summation order, so the evolution equals the built-in operator's bit for bit."""
    import torch
    cell = cells.get("X")
    assert cell.N > EPI_ONLY_BLOCKS * GENERIC_BLOCK
    Eb = (-cell.L / 2, cell.L / 2)
    calls = []
    want = pkg.chebyshev_time_evolve(cell.d["psi_c"], 0.3, pkg.apply_H, cell.m, cheb_n=cheb_n, Ebounds=Eb)
    got = pkg.chebyshev_time_evolve(cell.d["psi_c"], 0.3, _own_apply(pkg, calls), cell.m, cheb_n=cheb_n, Ebounds=Eb)
    assert calls and set(calls) == {cell.N}                    # the user operator ran, on whole vectors
    g, w = got.cpu().numpy(), want.cpu().numpy()
    assert bits_equal(g, w), differing(cell, f"chebyshev evolution, {cheb_n} terms, user operator", g, w)
    assert bool(torch.isfinite(torch.view_as_real(got)).all()) and float(got.abs().max()) > 1e-4


def test_epilogue_only_kernel_sums_in_a_moment_recursion(pkg, cells):
    """RESCALE_DOT and KPM through k_epilogue_only (4096 partial pairs, rows past 4096 * 256) against the fused form (32 071 pairs,
    two-stage reduction): the moments of a normalised vector within 1e-13, the bar test_user_operator_at_recursion_level uses for
    the same comparison at L = 12 (the two runs differ in the order of their sums only)."""
    cell = cells.get("X")
    a, b = pkg.rescaling_from_bounds(-cell.L / 2, cell.L / 2)
    calls = []
    mu = pkg.compute_chebyshev_moments(_own_apply(pkg, calls), cell.ref["psi_c"], 6, a, b, cell.m)
    mu2 = pkg.compute_chebyshev_moments(pkg.apply_H, cell.ref["psi_c"], 6, a, b, cell.m)
    print(f"X moments, user operator against built-in: {np.abs(mu - mu2).max():.2e}")
    assert calls and np.isfinite(mu).all() and abs(mu[0] - 1.0) <= 1e-13
    assert np.abs(mu - mu2).max() <= 1e-13
