"""GPU tests of the fixed-order composite backward (splat_composite_backward_det, include/splat.h): against the float64
restatement within the atomic path's bounds; its cross-tile addition order restated on the CPU and compared bit for bit; the
prior content added once; the same bits on every run and on every ctx; its edges, its refusals and its stores' bounds.

Clouds, lists and upstream gradients are built as tests/test_gpu_ellipsoid_grad.py builds them: the NumPy oracle's lists, random
upstreams that are zero on rim and near pixels."""
import ctypes as C
import functools

import numpy as np
import pytest

import splat_renderer_amd as sr
from splat_renderer_amd import _lib
from tests import ellipsoid_depth_grad_ref as DR
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER
from tests import test_gpu_ellipsoid_grad as TG

pytestmark = pytest.mark.gpu

CASES = TG.CASES
REC_COLS = TG.REC_COLS
rel_l2 = TG.rel_l2
TILE = 16


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def tiles_of(w, h):
    return -(-w // TILE), -(-h // TILE)


@functools.lru_cache(maxsize=None)
def scene(n, w, h, seed, spread, scale):
    """One case's cloud, projection, oracle lists, decisions and upstreams: computed once, shared, never written to."""
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale)
    u = TG.camera_u(w, h)
    _, proj, _ = ER.project(u, pos, scl, rot)
    rec, counts, offsets, idx = TG.lists(u, pos, scl, rot, w, h)
    z = np.ascontiguousarray(proj[:, 4])
    dec = GR.decisions(rec, col, idx, counts, offsets, w, h)
    ref = ER.composite(rec, col, z, idx, counts, offsets, w, h)
    g = GR.upstream(w, h, dec["rim"], dec["near"], seed)
    gd = DR.upstream_depth(ref["alpha"], dec["rim"], dec["near"], seed)
    out = dict(rec=rec, col=col, proj=proj, z=z, counts=counts, offsets=offsets, idx=idx, dec=dec, g=g, gd=gd, n=n, w=w, h=h)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


class Det:
    """The inputs of one scene on the device, for any number of splat_composite_backward_det calls."""

    def __init__(self, device, s, proj=None, guard=0):
        d = self.d = device
        self.n, self.w, self.h = s["n"], s["w"], s["h"]
        idx = s["idx"]
        self.pairs = int(idx.size)
        assert self.pairs == int(s["counts"].sum())
        ntx, nty = tiles_of(self.w, self.h)
        self.tiles = ntx * nty
        arrays = (s["rec"], s["col"], s["proj"] if proj is None else proj, idx if idx.size else np.zeros(1, np.uint32), s["counts"],
                  s["offsets"], s["z"])
        self.bufs = [d.createBufferFrom(np.ascontiguousarray(a) if a.size else np.zeros(4, np.float32)) for a in arrays]
        self.g = d.createBuffer(self.w * self.h * 16)
        self.gd = d.createBuffer(self.w * self.h * 4)
        self.out = [d.createBuffer(max(self.n, 1) * 32), d.createBuffer(max(self.n, 1) * 16), d.createBuffer(max(self.n, 1) * 4)]
        self.guard = guard
        self.ws_bytes = {dep: int(d.lib.splat_composite_backward_det_workspace_bytes(self.pairs, self.tiles, self.n, dep)) for dep in (0, 1)}
        self.ws = d.createBuffer(self.ws_bytes[1] + 2 * guard + 16)

    def run(self, g, gd=None, prior=None, c=None, ws_ptr="own", ws_bytes=None, proj_ptr="own", pairs=None):
        """One call: (rc, grad_records (n, 8), grad_color_opacity (n, 4), grad_depth (n,)).  gd None: the colour-only variant
        (grad_depth then returns its prior).  prior: the three outputs' content before the call (default zeros)."""
        d, n = self.d, self.n
        depth = gd is not None
        self.g.write(np.ascontiguousarray(g, np.float32))
        if depth:
            self.gd.write(np.ascontiguousarray(gd, np.float32))
        for o, shape, p in zip(self.out, ((n, 8), (n, 4), (n,)), prior or (None, None, None)):
            if p is None:
                o.zero()
            elif n:
                o.write(np.ascontiguousarray(p, np.float32).reshape(shape))
        b = self.bufs
        rc = d.lib.splat_composite_backward_det(
            d.ctx, C.byref(c or TG.cfg()), b[1].ptr, 1, b[0].ptr, b[2].ptr if proj_ptr == "own" else proj_ptr, b[3].ptr, b[4].ptr, b[5].ptr,
            self.pairs if pairs is None else pairs, self.w, self.h, self.g.ptr, n, self.out[0].ptr, self.out[1].ptr,
            b[6].ptr if depth else None, 1 if depth else 0, self.gd.ptr if depth else None, self.out[2].ptr if depth else None,
            self.ws.ptr + self.guard if ws_ptr == "own" else ws_ptr, self.ws_bytes[int(depth)] if ws_bytes is None else ws_bytes)
        return (rc, self.out[0].read(np.float32, n * 8).reshape(n, 8), self.out[1].read(np.float32, n * 4).reshape(n, 4),
                self.out[2].read(np.float32, n))

    def destroy(self):
        for b in self.bufs + self.out + [self.g, self.gd, self.ws]:
            b.destroy()


def columns(grec, gcol, gz=None):
    cols = [(f"rec[{k}]", grec[:, k]) for k in REC_COLS] + [(f"col[{k}]", gcol[:, k]) for k in range(4)]
    return cols + ([("z", gz)] if gz is not None else [])


# ---- 1. against float64 ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [False, True], ids=["colour", "depth"])
@pytest.mark.parametrize("n,w,h,seed,spread,scale", CASES)
def test_against_float64(device, n, w, h, seed, spread, scale, depth):
    s = scene(n, w, h, seed, spread, scale)
    run = Det(device, s)
    rc, grec, gcol, gz = run.run(s["g"], s["gd"] if depth else None)
    run.destroy()
    assert rc == 0
    if depth:
        assert (s["gd"] != 0).any()
        want = DR.composite_depth_grads(s["rec"], s["col"], s["z"], s["dec"]["steps"], w, h, s["g"], s["gd"])
    else:
        want = GR.composite_grads(s["rec"], s["col"], s["dec"]["steps"], w, h, s["g"]) + (None,)
    assert np.isfinite(grec).all() and np.isfinite(gcol).all() and np.isfinite(gz).all()
    figures = []
    for (name, got), (_, ref) in zip(columns(grec, gcol, gz if depth else None), columns(*want)):
        figures.append((name, rel_l2(got, ref), np.abs(got - ref).max(), np.abs(ref).max()))
        print(f"n={n} {'depth' if depth else 'colour'} {name}: relative L2 {figures[-1][1]:.3g}, max |diff| {figures[-1][2]:.3g} of "
              f"max |ref| {figures[-1][3]:.3g}")
    for name, l2, mx, top in figures:
        assert l2 <= 1e-4, f"{name}: relative L2 {l2:.3g}"
        assert mx <= 2e-3 * top + 1e-30, f"{name}: max {mx:.3g}"
    reached = np.zeros(n, bool)
    for _pix, sp, _stop in s["dec"]["steps"]:
        reached[sp] = True
    assert (grec[~reached] == 0).all() and (gcol[~reached] == 0).all() and (gz[~reached] == 0).all()
    assert (grec[:, [4, 6, 7]] == 0).all()
    if not depth:
        assert (gz == 0).all()


# ---- 2. the cross-tile order ------------------------------------------------------------------------------------------------
ORDER_SCENE = (600, 100, 70, 7, 0.5, 0.2)
# two more, for the gather's other path (a rectangle of more than 64 tiles in more than one row is summed by a whole wave, the
# lanes taking rows): splats that cover most of a 10 x 9 tile screen, and splats that cover more than 64 tile rows of a 2 x 69
# tile screen (a lane then takes a second row)
WIDE_SCENE = (60, 160, 144, 8, 0.5, 0.6)
TALL_SCENE = (40, 32, 1100, 9, 0.5, 0.6)
ORDER_SCENES = {"issue": ORDER_SCENE, "wide": WIDE_SCENE, "tall": TALL_SCENE}


@functools.lru_cache(maxsize=None)
def check_order_scene(which):
    """The order test cannot go vacuous.  "issue": at least 100 splats have consumed pairs in >= 4 tiles over >= 2 tile rows and
    >= 2 tile columns.  "wide" / "tall": at least 20 such splats (>= 2 rows) whose tile rectangle holds more than 64 tiles / rows."""
    s = scene(*ORDER_SCENES[which])
    w, h = s["w"], s["h"]
    ntx, nty = tiles_of(w, h)
    used = set()
    for pix, sp, _stop in s["dec"]["steps"]:
        t = (pix // w // TILE) * ntx + (pix % w) // TILE
        used.update(zip(sp.tolist(), t.tolist()))
    per = {}
    for sp, t in used:
        per.setdefault(sp, []).append(t)
    b = s["proj"][:, :4].astype(np.float64)  # the binner's tile rectangle (finite bounds here)
    with np.errstate(invalid="ignore"):
        cols = np.minimum(np.floor(np.minimum(b[:, 2], w) / TILE), ntx - 1) - np.floor(np.maximum(b[:, 0], 0) / TILE) + 1
        rows = np.minimum(np.floor(np.minimum(b[:, 3], h) / TILE), nty - 1) - np.floor(np.maximum(b[:, 1], 0) / TILE) + 1
    many = [sp for sp, ts in per.items() if len(ts) >= 4 and len({t // ntx for t in ts}) >= 2 and (ntx == 2 or len({t % ntx for t in ts}) >= 2)]
    print(f"order scene {which}: {s['idx'].size} pairs, longest list {int(s['counts'].max())}, {len(per)} splats reached, {len(many)} over >= 4 tiles")
    if which == "issue":
        assert (ntx, nty) == (7, 5) and int(s["counts"].max()) > 4 * 64 and len(many) >= 100
    elif which == "wide":
        assert sum(1 for sp in many if rows[sp] > 1 and cols[sp] * rows[sp] > 64) >= 20
    else:
        assert sum(1 for sp in many if rows[sp] > 64) >= 20


@pytest.mark.parametrize("which", list(ORDER_SCENES))
@pytest.mark.parametrize("depth", [False, True], ids=["colour", "depth"])
def test_cross_tile_order_is_the_contracts(device, depth, which):
    check_order_scene(which)
    s = scene(*ORDER_SCENES[which])
    n, w, h = s["n"], s["w"], s["h"]
    ntx, nty = tiles_of(w, h)
    run = Det(device, s)
    rc, *full = run.run(s["g"], s["gd"] if depth else None)
    assert rc == 0
    one = np.float32(0)
    total = [np.zeros((n, 8), np.float32), np.zeros((n, 4), np.float32), np.zeros(n, np.float32)]
    for ty in range(nty):
        row = [np.zeros_like(t) for t in total]
        for tx in range(ntx):  # the upstream zeroed outside one tile: the run returns that tile's P(i, t, k) exactly
            g, gd = np.zeros_like(s["g"]), np.zeros_like(s["gd"])
            sl = (slice(ty * TILE, (ty + 1) * TILE), slice(tx * TILE, (tx + 1) * TILE))
            g[sl], gd[sl] = s["g"][sl], s["gd"][sl]
            rc, *part = run.run(g, gd if depth else None)
            assert rc == 0
            row = [(r + p).astype(np.float32) for r, p in zip(row, part)]   # a row's tiles left to right, from +0
        total = [(t + r).astype(np.float32) for t, r in zip(total, row)]     # the rows top to bottom, from +0
    run.destroy()
    want = [(one + t).astype(np.float32) for t in total]                      # the zero prior + total
    assert np.abs(full[0]).max() > 0 and (not depth or np.abs(full[2]).max() > 0)
    for name, got, exp in zip(("records", "colour", "depth"), full, want):
        diff = bits(got) != bits(exp)
        assert not diff.any(), f"{name}: {int(diff.sum())} words differ from the contract's order"


# ---- 3. prior content --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [False, True], ids=["colour", "depth"])
def test_prior_is_added_once(device, depth):
    s = scene(*CASES[0])
    n = s["n"]
    run = Det(device, s)
    gd = s["gd"] if depth else None
    rc, *total = run.run(s["g"], gd)
    assert rc == 0
    rng = np.random.default_rng(17)
    prior = [rng.uniform(-3, 3, (n, 8)).astype(np.float32), rng.uniform(-3, 3, (n, 4)).astype(np.float32),
             rng.uniform(-3, 3, n).astype(np.float32)]
    rc, *got = run.run(s["g"], gd, prior=prior)
    run.destroy()
    assert rc == 0
    reached = (total[1] != 0).any(axis=1)
    assert reached.sum() > n // 10
    for k, (name, t, p, o) in enumerate(zip(("records", "colour", "depth"), total, prior, got)):
        want = (p + t).astype(np.float32)
        if k == 0:
            want[:, [4, 6, 7]] = p[:, [4, 6, 7]]  # the columns nobody writes
        if k == 2 and not depth:
            want = p                              # (not an argument of the colour-only call)
        assert np.array_equal(bits(o), bits(want)), f"{name}: prior + total differs"


# ---- 4. repeatable -----------------------------------------------------------------------------------------------------------
def test_same_bits_on_every_run_and_ctx(device):
    s = scene(*CASES[4])
    assert s["n"] == 40000
    run = Det(device, s)
    first = run.run(s["g"], s["gd"])
    assert first[0] == 0
    for _ in range(2):
        again = run.run(s["g"], s["gd"])
        assert again[0] == 0 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(again[1:], first[1:]))
    run.destroy()
    other = sr.Device(0)
    try:
        run2 = Det(other, s)
        fourth = run2.run(s["g"], s["gd"])
        run2.destroy()
    finally:
        other.destroy()
    assert fourth[0] == 0 and all(np.array_equal(bits(a), bits(b)) for a, b in zip(fourth[1:], first[1:])), "a second ctx gave other bits"
    # the atomic path: within 1e-4 of the same float64 reference, so within 2e-4 of this one
    from tests import test_gpu_ellipsoid_depth_grad as TD
    atomic = [TD.composite_backward_depth(device, s["rec"], s["col"], s["z"], s["counts"], s["offsets"], s["idx"], s["w"], s["h"], s["g"],
                                          s["gd"]) for _ in range(2)]
    assert atomic[0][0] == 0 and atomic[1][0] == 0
    differed = any(not np.array_equal(bits(a), bits(b)) for a, b in zip(atomic[0][1:], atomic[1][1:]))
    print(f"the atomic path's two runs {'differed' if differed else 'did not differ'} in their bits")
    for (name, got), (_, ref) in zip(columns(*first[1:]), columns(*atomic[0][1:])):
        e = rel_l2(got, ref)
        print(f"deterministic vs atomic {name}: relative L2 {e:.3g}")
        assert e <= 2e-4, f"{name}: relative L2 {e:.3g} to the atomic path"


# ---- 5. edges and errors -----------------------------------------------------------------------------------------------------
def _tiny(n, w, h, seed=1, culled=False, empty=False):
    pos, scl, rot, col = ER.make_cloud(max(n, 1), seed, 0.0 if n <= 1 else 0.5, 0.05, degenerate=False)
    pos, scl, rot, col = pos[:n], scl[:n], rot[:n], col[:n]
    u = TG.camera_u(w, h)
    ntx, nty = tiles_of(w, h)
    if n and not culled:
        _, proj, _ = ER.project(u, pos, scl, rot)
        rec, counts, offsets, idx = TG.lists(u, pos, scl, rot, w, h)
    else:
        rec, proj = np.zeros((n, 8), np.float32), np.zeros((n, 8), np.float32)
        counts, offsets, idx = np.zeros(ntx * nty, np.uint32), np.zeros(ntx * nty + 1, np.uint32), np.zeros(0, np.uint32)
    if empty:  # every list empty although the splats are on screen
        counts, offsets, idx = np.zeros(ntx * nty, np.uint32), np.zeros(ntx * nty + 1, np.uint32), np.zeros(0, np.uint32)
    rng = np.random.default_rng(seed)
    return dict(rec=rec, col=col, proj=proj, z=np.ascontiguousarray(proj[:, 4]), counts=counts, offsets=offsets, idx=idx, n=n, w=w, h=h,
                g=rng.uniform(-1, 1, (h, w, 4)).astype(np.float32), gd=rng.uniform(-1, 1, (h, w)).astype(np.float32))


@pytest.mark.parametrize("depth", [False, True], ids=["colour", "depth"])
def test_edges(device, depth):
    for name, s in (("n = 1", _tiny(1, 64, 48)), ("n = 0", _tiny(0, 64, 48)), ("empty lists", _tiny(50, 64, 48, empty=True)),
                    ("all culled", _tiny(50, 64, 48, culled=True)), ("one partial tile", _tiny(20, 5, 3))):
        n = s["n"]
        run = Det(device, s)
        gd = s["gd"] if depth else None
        rc, grec, gcol, gz = run.run(s["g"], gd)
        assert rc == 0, name
        prior = [np.full((n, 8), 2.0, np.float32), np.full((n, 4), -1.0, np.float32), np.full(n, 5.0, np.float32)]
        rc2, prec, pcol, pz = run.run(s["g"], gd, prior=prior)
        run.destroy()
        assert rc2 == 0, name
        assert np.isfinite(grec).all() and np.isfinite(gcol).all() and np.isfinite(gz).all(), name
        if name in ("n = 1", "one partial tile"):
            assert s["idx"].size > 0 and (gcol != 0).any(), name
            touched = (gcol != 0).any(axis=1)
        else:
            assert (grec == 0).all() and (gcol == 0).all() and (gz == 0).all(), name
            touched = np.zeros(n, bool)
        # untouched splats, and the columns nobody writes, keep their prior bits
        assert np.array_equal(prec[~touched], prior[0][~touched]) and np.array_equal(pcol[~touched], prior[1][~touched]), name
        assert np.array_equal(pz[~touched], prior[2][~touched]) and np.array_equal(prec[:, [4, 6, 7]], prior[0][:, [4, 6, 7]]), name


def test_refusals_launch_nothing(device):
    s = scene(*CASES[2])
    n = s["n"]
    run = Det(device, s)
    prior = [np.full((n, 8), 2.0, np.float32), np.full((n, 4), -1.0, np.float32), np.full(n, 5.0, np.float32)]
    need = run.ws_bytes[1]
    own = run.ws.ptr + run.guard
    bad_calls = [("NULL workspace", dict(ws_ptr=None)), ("misaligned workspace", dict(ws_ptr=own + 4)),
                 ("a workspace one byte short", dict(ws_bytes=need - 1)), ("NULL projected", dict(proj_ptr=None)),
                 ("2^32 pairs", dict(pairs=1 << 32, ws_bytes=1 << 40))]
    bad_calls += [(str(bad), dict(c=TG.cfg(**bad))) for bad in (dict(tile_size=8), dict(mode=_lib.MODE_REFERENCE_LITERAL), dict(early_out=0),
                                                                 dict(tile_row0=1), dict(tile_row1=2), dict(footprint=_lib.FOOTPRINT_DISC),
                                                                 dict(record_format=_lib.RECORDS_LIT32))]
    for name, kw in bad_calls:
        for gd in (None, s["gd"]):
            if name == "a workspace one byte short" and gd is None:
                kw = dict(ws_bytes=run.ws_bytes[0] - 1)
            rc, grec, gcol, gz = run.run(s["g"], gd, prior=prior, **kw)
            assert rc == -1, name
            assert np.array_equal(grec, prior[0]) and np.array_equal(gcol, prior[1]) and np.array_equal(gz, prior[2]), name
    # the exact size is enough
    rc, _, gcol, _ = run.run(s["g"], s["gd"], ws_bytes=need)
    run.destroy()
    assert rc == 0 and (gcol != 0).any()
    ntx, nty = tiles_of(s["w"], s["h"])
    for dep, nv in ((0, 9), (1, 10)):
        assert run.ws_bytes[dep] == 16 * ntx * nty + 16 * ((n + 3) // 4) + 4 * nv * s["idx"].size
        assert run.ws_bytes[dep] <= 40 * s["idx"].size + 16 * ntx * nty + 4 * n + 12


def test_foreign_lists_stay_inside_the_workspace(device):
    """Lists binned from another projection (here: the true one, while `projected` says every rectangle is a tile smaller on
    both axes, or nowhere, or two tiles larger all round): no error, gradients unspecified, and not one byte stored outside the
    workspace, which is checked through a patterned guard on either side of it."""
    s = scene(*ORDER_SCENE)
    proj = s["proj"].copy()
    wide = (proj[:, 2] - proj[:, 0] > TILE) & (proj[:, 3] - proj[:, 1] > TILE)
    assert wide.sum() > 100
    proj[wide, 2] -= TILE
    proj[wide, 3] -= TILE
    guard = 1 << 16
    grown = s["proj"].copy()  # (their tile counts add up to more than the lists' pairs: slots past the last are dropped)
    grown[:, :2] -= 2 * TILE
    grown[:, 2:4] += 2 * TILE
    for shrunk in (proj, np.zeros_like(proj), grown):
        run = Det(device, s, proj=shrunk, guard=guard)
        pattern = np.full(run.ws.size // 4, 0xA5C3F00D, np.uint32)
        for dep in (False, True):
            run.ws.write(pattern)
            rc, grec, gcol, gz = run.run(s["g"], s["gd"] if dep else None)
            assert rc == 0
            after = run.ws.read(np.uint32)
            used = run.ws_bytes[int(dep)] // 4
            assert (after[:guard // 4] == 0xA5C3F00D).all(), "stored below the workspace"
            assert (after[guard // 4 + used:] == 0xA5C3F00D).all(), "stored past the workspace"
        run.destroy()
