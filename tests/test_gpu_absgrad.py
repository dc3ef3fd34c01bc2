"""GPU tests of AbsGS's absolute screen-space gradient at the C ABI (include/splat.h: splat_composite_backward_abs,
splat_composite_backward_det_abs, splat_density_accumulate_abs).

Per-splat bound.  On tests/composite_grad_terms_ref.py's four scenes, under both forward update orders and through the four new
paths (atomic, atomic with depth, fixed-order, fixed-order with depth), for every reached splat s and k in {0, 1}
    |got_abs - m[s, k]| <= 4 c_abs m[s, k]
m = the float64 sum of |term| (terms64), c_abs = the largest |abs32 - m| / m of the binary32 restatement of the kernel's formulas
with np.abs on the per-pair terms (tests/absgrad_ref.py; never the kernel).  The 4 is test_gpu_grad_per_splat.MARGIN, for its
reasons: the kernel's addition order, v_exp_f32's 1 ulp against NumPy's half ulp, contraction.  Unreached splats are exact zeros.
A kernel that returned |signed sum| would miss this by five orders of magnitude (tests/test_absgrad_cpu.py prints the ratios).

Measured on one MI355X ("Absolute screen-space gradient"), the kernel's worst err / m against c_abs, both in units of
2^-24; the atomic and the fixed-order entry points agree to the digit shown except on veil, px, depth (atomic 12.5, fixed 13.6):
             quadrant colour   quadrant depth    px colour         px depth
    hazy       9.1 /  27.2      19.0 /  33.6      9.1 /  27.2      17.3 /  27.1
    veil      15.7 /  18.5      14.2 /  24.6     14.7 /  18.5      13.6 /  21.2
    needle    17.2 /  31.8      18.0 /  31.7     17.4 /  29.9      18.0 /  31.7
    classic  109.5 /  62.8     174.7 /  95.0    109.5 /  62.8      34.9 /  95.0
The largest ratio is 1.84 (classic, quadrant, depth: the splat and the figure of the signed sums' table, a splat of few pairs).
The signed outputs: the fixed-order entry point gives splat_composite_backward_det's bits, the atomic one stays inside the
existing per-splat bound.  The same bits on every run and every ctx; a prior is added once; edges and refusals; the density
statistic against the header's rule and, on a plane that copies columns 0 and 1, splat_density_accumulate's bits.
"""
import ctypes as C

import numpy as np
import pytest

import splat_renderer_amd as sr
from tests import absgrad_ref as AR
from tests import composite_grad_terms_ref as CT
from tests import density_ref as DR
from tests import test_gpu_ellipsoid_grad as TG
from tests import test_gpu_grad_decisions as TDEC
from tests import test_gpu_grad_deterministic as TDET
from tests import test_gpu_grad_per_splat as TPS

pytestmark = pytest.mark.gpu

bits = TDET.bits
ENTRIES = ("atomic", "atomic_depth", "det", "det_depth")
MARGIN = TPS.MARGIN


class Abs:
    """One scene's inputs on the device, for any number of calls of the four composite backwards that take them: the two _abs
    entry points and, for comparison, splat_composite_backward_det."""

    def __init__(self, device, s):
        d = self.d = device
        self.n, self.w, self.h = s["n"], s["w"], s["h"]
        idx = s["idx"]
        self.pairs = int(idx.size)
        ntx, nty = TDET.tiles_of(self.w, self.h)
        self.tiles = ntx * nty
        arrays = (s["rec"], s["col"], s["proj"], idx if idx.size else np.zeros(1, np.uint32), s["counts"], s["offsets"], s["z"])
        self.bufs = [d.createBufferFrom(np.ascontiguousarray(a) if a.size else np.zeros(4, np.float32)) for a in arrays]
        self.g = d.createBuffer(self.w * self.h * 16)
        self.gd = d.createBuffer(self.w * self.h * 4)
        n1 = max(self.n, 1)
        self.out = [d.createBuffer(n1 * 32), d.createBuffer(n1 * 16), d.createBuffer(n1 * 4), d.createBuffer(n1 * 8 + 16)]
        self.shapes = ((self.n, 8), (self.n, 4), (self.n,), (self.n, 2))
        self.ws_bytes = {dep: int(d.lib.splat_composite_backward_det_abs_workspace_bytes(self.pairs, self.tiles, self.n, dep)) for dep in (0, 1)}
        self.plain_ws_bytes = {dep: int(d.lib.splat_composite_backward_det_workspace_bytes(self.pairs, self.tiles, self.n, dep)) for dep in (0, 1)}
        self.ws = d.createBuffer(self.ws_bytes[1] + 32)

    def run(self, entry, g, gd=None, prior=None, c=None, abs_ptr="own", ws_ptr="own", ws_bytes=None):
        """One call: (rc, grad_records (n, 8), grad_color_opacity (n, 4), grad_depth (n,), grad_center_abs (n, 2)).  entry:
        "atomic" / "det" (the _abs entry points) or "det_plain" (splat_composite_backward_det: grad_center_abs then returns its
        prior).  gd None: the colour-only variant.  prior: the four outputs' content before the call (default zeros)."""
        d, n = self.d, self.n
        depth = gd is not None
        self.g.write(np.ascontiguousarray(g, np.float32))
        if depth:
            self.gd.write(np.ascontiguousarray(gd, np.float32))
        for o, shape, p in zip(self.out, self.shapes, prior or (None,) * 4):
            if p is None:
                o.zero()
            elif n:
                o.write(np.ascontiguousarray(p, np.float32).reshape(shape))
        b = self.bufs
        gabs = self.out[3].ptr if abs_ptr == "own" else abs_ptr
        tail = (b[6].ptr if depth else None, 1 if depth else 0, self.gd.ptr if depth else None, self.out[2].ptr if depth else None)
        cfg = C.byref(c or TG.cfg())
        if entry == "atomic":
            rc = d.lib.splat_composite_backward_abs(d.ctx, cfg, b[1].ptr, 1, b[0].ptr, b[3].ptr, b[4].ptr, b[5].ptr, self.w, self.h, self.g.ptr, n,
                                                    self.out[0].ptr, self.out[1].ptr, *tail, gabs)
        else:
            plain = entry == "det_plain"
            need = (self.plain_ws_bytes if plain else self.ws_bytes)[int(depth)]
            args = (d.ctx, cfg, b[1].ptr, 1, b[0].ptr, b[2].ptr, b[3].ptr, b[4].ptr, b[5].ptr, self.pairs, self.w, self.h, self.g.ptr, n,
                    self.out[0].ptr, self.out[1].ptr, *tail, self.ws.ptr if ws_ptr == "own" else ws_ptr, need if ws_bytes is None else ws_bytes)
            rc = d.lib.splat_composite_backward_det(*args) if plain else d.lib.splat_composite_backward_det_abs(*args, gabs)
        return (rc, *(o.read(np.float32, int(np.prod(shape))).reshape(shape) for o, shape in zip(self.out, self.shapes)))

    def destroy(self):
        for b in self.bufs + self.out + [self.g, self.gd, self.ws]:
            b.destroy()


_results = {}


def run_entry(device, name, order, entry):
    """(rc, grec, gcol, gz, gabs) of one new path on a scene with the forward update order forced; once per session."""
    key = (name, order, entry)
    if key not in _results:
        s = CT.scene(name)
        TDEC.with_kernel(device, TPS.KERNEL[order])
        try:
            run = Abs(device, s)
            _results[key] = run.run(entry.split("_")[0], s["g"], s["gd"] if entry.endswith("depth") else None)
            run.destroy()
        finally:
            TDEC.with_kernel(device, -1)
    return _results[key]


# ---- 1. the per-splat bound --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("order", CT.ORDERS)
@pytest.mark.parametrize("name", CT.SCENES)
def test_absolute_sums_per_splat(device, name, order, entry):
    s = CT.scene(name)
    depth = entry.endswith("depth")
    ref = AR.restated_abs(name, order, depth)
    m = AR.want_abs(name, depth)
    rc, grec, gcol, gz, gabs = run_entry(device, name, order, entry)
    assert rc == 0
    assert gabs.shape == m.shape and np.isfinite(gabs).all() and (gabs >= 0).all()
    q = CT.ratios(gabs, m, m)
    worst = np.unravel_index(np.argmax(q), q.shape)
    print(f"{name} {order} {entry}: kernel worst err / m = {q.max() * 2 ** 24:.1f} x 2^-24 (splat {worst[0]}, {CT.NAMES[worst[1]]}) against "
          f"c_abs = {ref['c'] * 2 ** 24:.1f} x 2^-24: ratio {q.max() / ref['c']:.2f}")
    assert (gabs[~s["reached"]] == 0).all()
    assert (gabs[s["reached"]] > 0).any()
    bad = q > MARGIN * ref["c"]
    assert not bad.any(), (f"{int(bad.sum())} (splat, number) sums beyond {MARGIN:g} c_abs m; the worst at splat {worst[0]}, {CT.NAMES[worst[1]]}: "
                           f"err / m = {q.max() * 2 ** 24:.1f} x 2^-24 = {q.max() / ref['c']:.2f} c_abs")


# ---- 2. the signed outputs are what they were --------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [False, True], ids=["colour", "depth"])
@pytest.mark.parametrize("name", ["hazy", "classic"])
def test_fixed_order_signed_outputs_are_the_det_entry_points_bits(device, name, depth):
    s = CT.scene(name)
    run = Abs(device, s)
    gd = s["gd"] if depth else None
    plain = run.run("det_plain", s["g"], gd)
    both = run.run("det", s["g"], gd)
    run.destroy()
    assert plain[0] == 0 and both[0] == 0
    assert np.abs(plain[1]).max() > 0 and np.abs(plain[2]).max() > 0 and (not depth or np.abs(plain[3]).max() > 0)
    for what, a, b in zip(("grad_records", "grad_color_opacity", "grad_depth"), both[1:4], plain[1:4]):
        diff = bits(a) != bits(b)
        assert not diff.any(), f"{what}: {int(diff.sum())} words differ from splat_composite_backward_det's"
    assert (plain[4] == 0).all() and (both[4] > 0).any()


@pytest.mark.parametrize("depth", [False, True], ids=["colour", "depth"])
@pytest.mark.parametrize("order", CT.ORDERS)
@pytest.mark.parametrize("name", ["hazy", "classic"])
def test_atomic_signed_outputs_stay_inside_the_per_splat_bound(device, name, order, depth):
    s = CT.scene(name)
    ref = CT.restated(name, order, depth)
    want, m = (s["want_depth"], s["m_depth"]) if depth else (s["want"], s["m"])
    rc, grec, gcol, gz, _ = run_entry(device, name, order, "atomic_depth" if depth else "atomic")
    assert rc == 0
    got = np.concatenate([grec[:, CT.REC_COLS], gcol] + ([gz[:, None]] if depth else []), axis=1)
    q = CT.ratios(got, want, m)
    print(f"{name} {order} {'depth' if depth else 'colour'}: signed worst err / m = {q.max() / ref['c']:.2f} c_scene")
    assert (got[~s["reached"]] == 0).all() and (grec[:, [4, 6, 7]] == 0).all()
    assert (q <= TPS.MARGIN * ref["c"]).all()


@pytest.mark.parametrize("which", ["wide", "tall"])
def test_gather_of_large_rectangles(device, which):
    """k_det_gather's other path (a rectangle of more than 64 tiles in more than one row is summed by a whole wave): the signed
    outputs are still splat_composite_backward_det's bits, and the absolute sums are the atomic path's up to the order of the
    additions.  Both add the same non-negative binary32 per-tile sums P(i, t, k), one tile after another: each result is within
    T 2^-24 (relative) of their exact sum, T the number of tiles, so the two lie within T 2^-23 of each other."""
    TDET.check_order_scene(which)
    s = TDET.scene(*TDET.ORDER_SCENES[which])
    run = Abs(device, s)
    plain = run.run("det_plain", s["g"], s["gd"])
    det = run.run("det", s["g"], s["gd"])
    atomic = run.run("atomic", s["g"], s["gd"])
    run.destroy()
    assert plain[0] == 0 and det[0] == 0 and atomic[0] == 0
    for a, b in zip(det[1:4], plain[1:4]):
        assert np.array_equal(bits(a), bits(b))
    d, a = det[4].astype(np.float64), atomic[4].astype(np.float64)
    assert (d > 0).sum() > s["n"] and np.array_equal(d > 0, a > 0)
    rel = np.abs(d - a) / np.where(a > 0, a, 1.0)
    print(f"{which}: |fixed-order - atomic| / atomic at most {rel.max() * 2 ** 24:.1f} x 2^-24 over {run.tiles} tiles")
    assert (rel <= run.tiles * 2.0 ** -23).all()
    assert (d * (1 + run.tiles * 2.0 ** -22) >= np.abs(det[1][:, :2])).all()  # (a signed sum's error is relative to the absolute one)


# ---- 3. determinism and accumulation -----------------------------------------------------------------------------------------
def test_same_bytes_on_every_run_and_ctx_and_a_prior_is_added_once(device):
    s = CT.scene("classic")
    n = s["n"]
    run = Abs(device, s)
    first = run.run("det", s["g"], s["gd"])
    again = run.run("det", s["g"], s["gd"])
    rng = np.random.default_rng(23)
    prior = [rng.uniform(-3, 3, shape).astype(np.float32) for shape in run.shapes]
    third = run.run("det", s["g"], s["gd"], prior=prior)
    atomic = run.run("atomic", s["g"], s["gd"], prior=prior)
    run.destroy()
    other = sr.Device(0)
    try:
        run2 = Abs(other, s)
        fourth = run2.run("det", s["g"], s["gd"])
        run2.destroy()
    finally:
        other.destroy()
    assert first[0] == 0 and again[0] == 0 and third[0] == 0 and fourth[0] == 0 and atomic[0] == 0
    assert (first[4][s["reached"]] > 0).any()
    for a, b, c in zip(first[1:], again[1:], fourth[1:]):
        assert np.array_equal(bits(a), bits(b)), "a second run gave other bits"
        assert np.array_equal(bits(a), bits(c)), "a second ctx gave other bits"
    # prior + total in one add; the columns nobody writes keep the prior; splats no pixel consumed keep their bits on both paths
    for k, (t, p, o) in enumerate(zip(first[1:], prior, third[1:])):
        want = (p + t).astype(np.float32)
        if k == 0:
            want[:, [4, 6, 7]] = p[:, [4, 6, 7]]
        assert np.array_equal(bits(o), bits(want)), f"output {k}: prior + total differs"
    assert (first[1][:, [4, 6, 7]] == 0).all()
    unreached = ~s["reached"]
    assert unreached.any()
    for p, o in zip(prior, atomic[1:]):
        assert np.array_equal(bits(o[unreached]), bits(p[unreached]))
    m = AR.want_abs("classic", True)
    c = AR.restated_abs("classic", "quadrant", True)["c"]
    err = np.abs(atomic[4].astype(np.float64) - prior[3] - m)
    assert (err <= MARGIN * c * m + 2.0 ** -23 * (np.abs(prior[3]) + m)).all()  # (and one rounding of the add into the prior)


# ---- 4. edges and refusals ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry", ["atomic", "det"])
@pytest.mark.parametrize("depth", [False, True], ids=["colour", "depth"])
def test_edges(device, entry, depth):
    cases = (("n = 1", TDET._tiny(1, 64, 48)), ("n = 0", TDET._tiny(0, 64, 48)), ("empty lists", TDET._tiny(50, 64, 48, empty=True)),
             ("all culled", TDET._tiny(50, 64, 48, culled=True)), ("17 x 1", TDET._tiny(20, 17, 1)), ("1 x 17", TDET._tiny(20, 1, 17)))
    for name, s in cases:
        n = s["n"]
        run = Abs(device, s)
        gd = s["gd"] if depth else None
        rc, grec, gcol, gz, gabs = run.run(entry, s["g"], gd)
        assert rc == 0, name
        prior = [np.full((n, 8), 2.0, np.float32), np.full((n, 4), -1.0, np.float32), np.full(n, 5.0, np.float32), np.full((n, 2), 3.0, np.float32)]
        rc2, prec, pcol, pz, pabs = run.run(entry, s["g"], gd, prior=prior)
        run.destroy()
        assert rc2 == 0, name
        assert all(np.isfinite(a).all() for a in (grec, gcol, gz, gabs)), name
        if name in ("n = 1", "17 x 1", "1 x 17"):
            assert s["idx"].size > 0 and (gcol != 0).any() and (gabs > 0).any(), name
            touched = (gcol != 0).any(axis=1)
            assert (gabs[touched] >= np.abs(grec[touched][:, :2]) * (1 - 2.0 ** -20)).all(), name
        else:
            assert (grec == 0).all() and (gcol == 0).all() and (gz == 0).all() and (gabs == 0).all(), name
            touched = np.zeros(n, bool)
        assert (gabs[~touched] == 0).all(), name
        for got, p in zip((prec, pcol, pz, pabs), prior):
            assert np.array_equal(got[~touched], p[~touched]), name
        assert np.array_equal(prec[:, [4, 6, 7]], prior[0][:, [4, 6, 7]]), name


def test_refusals_launch_nothing(device):
    s = TDET._tiny(50, 64, 48)
    n = s["n"]
    run = Abs(device, s)
    prior = [np.full((n, 8), 2.0, np.float32), np.full((n, 4), -1.0, np.float32), np.full(n, 5.0, np.float32), np.full((n, 2), 3.0, np.float32)]
    own = run.out[3].ptr
    for entry in ("atomic", "det"):
        bad_calls = [("NULL grad_center_abs", dict(abs_ptr=None)), ("misaligned grad_center_abs", dict(abs_ptr=own + 4)),
                     ("tile_size 8", dict(c=TG.cfg(tile_size=8))), ("early_out 0", dict(c=TG.cfg(early_out=0)))]
        if entry == "det":
            bad_calls += [("NULL workspace", dict(ws_ptr=None)), ("misaligned workspace", dict(ws_ptr=run.ws.ptr + 4)),
                          ("a workspace one byte short", None), ("the plain entry point's workspace", "plain")]
        for name, kw in bad_calls:
            for dep, gd in enumerate((None, s["gd"])):
                if kw is None:
                    kw_ = dict(ws_bytes=run.ws_bytes[dep] - 1)
                elif kw == "plain":
                    kw_ = dict(ws_bytes=run.plain_ws_bytes[dep])
                else:
                    kw_ = kw
                rc, *outs = run.run(entry, s["g"], gd, prior=prior, **kw_)
                assert rc == -1, (entry, name)
                for got, p in zip(outs, prior):
                    assert np.array_equal(got, p), (entry, name)
    rc, _, gcol, _, gabs = run.run("det", s["g"], s["gd"], ws_bytes=run.ws_bytes[1])  # the exact size is enough
    run.destroy()
    assert rc == 0 and (gcol != 0).any() and (gabs > 0).any()
    assert s["idx"].size > 0 and run.ws_bytes[0] - run.plain_ws_bytes[0] == 8 * s["idx"].size == run.ws_bytes[1] - run.plain_ws_bytes[1]


# ---- 5. the density statistic -------------------------------------------------------------------------------------------------
def _density_case(n, seed):
    """n records over a 64 x 48 screen: inside it, outside it, straddling an edge, culled (all zeros); a gradient plane."""
    w, h = 64, 48
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 8), np.float32)
    kind = np.arange(n) % 4 if n > 1 else np.array([2])
    rec[:, 2] = rng.uniform(0.05, 0.5, n)
    rec[:, 3] = rng.uniform(-0.2, 0.2, n)
    rec[:, 5] = rng.uniform(0.05, 0.5, n)
    hx = np.sqrt(rec[:, 3] ** 2 + rec[:, 5] ** 2) / (rec[:, 2] * rec[:, 5])
    rec[:, 0] = np.where(kind == 0, rng.uniform(0, w, n), np.where(kind == 1, w + hx + rng.uniform(1, 50, n), -0.5 * hx))
    rec[:, 1] = rng.uniform(0, h, n)
    rec[kind == 3] = 0
    gabs = (rng.uniform(0, 1, (n, 2)) * np.exp(rng.normal(-6, 2, (n, 1)))).astype(np.float32)
    return rec, gabs, kind, w, h


@pytest.mark.parametrize("n", [1, 255, 257])
def test_density_statistic_against_the_rule(device, n):
    lib, ctx = device.lib, device.ctx
    rec, gabs, kind, w, h = _density_case(n, n)
    grec = np.zeros((n, 8), np.float32)
    grec[:, :2] = gabs
    grec[:, 2:] = 7.0  # (columns the statistic does not read)
    drec, dabs, dgrec = (device.createBufferFrom(a) for a in (rec, gabs, grec))
    prior = [np.full(n, 0.5, np.float32), np.full(n, 2.0, np.float32), np.full(n, 1.5, np.float32)]
    results = []
    for fn, plane in ((lib.splat_density_accumulate_abs, dabs), (lib.splat_density_accumulate, dgrec)):
        stats = [device.createBufferFrom(p) for p in prior]
        vis = device.createBufferFrom(np.full(n + 3, 7, np.uint8))
        rc = fn(ctx, drec.ptr, plane.ptr, n, w, h, stats[0].ptr, stats[1].ptr, stats[2].ptr, vis.ptr)
        assert rc == 0
        results.append([b.read(np.float32, n) for b in stats] + [vis.read(np.uint8, n + 3)])
        for b in stats + [vis]:
            b.destroy()
    got, same = results
    mask, *ref = DR.accumulate(rec, grec, w, h, *prior)
    if n > 1:
        assert mask[kind == 0].all() and not mask[kind == 1].any() and mask[kind == 2].all() and not mask[kind == 3].any()
    assert np.array_equal(got[3][:n], mask) and (got[3][n:] == 7).all(), "the visibility mask differs"
    assert np.array_equal(got[1], ref[1]), "denom differs"
    for k, key in ((0, "grad_accum"), (2, "max_radius")):
        e = float((np.abs(got[k] - ref[k]) / ref[k]).max())
        print(f"n = {n}: {key} relative {e:.3g}")
        assert e <= 1e-6, f"{key} relative {e:.3g}"
        assert np.array_equal(bits(got[k][mask == 0]), bits(prior[k][mask == 0]))
    # a plane that copies columns 0 and 1: splat_density_accumulate's bits
    for a, b in zip(got, same):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
    # refusals: a NULL or misaligned plane
    stats = [device.createBufferFrom(p) for p in prior]
    vis = device.createBufferFrom(np.full(n + 3, 7, np.uint8))
    for ptr in (None, dabs.ptr + 4):
        assert lib.splat_density_accumulate_abs(ctx, drec.ptr, ptr, n, w, h, stats[0].ptr, stats[1].ptr, stats[2].ptr, vis.ptr) == -1
    assert all(np.array_equal(b.read(np.float32, n), p) for b, p in zip(stats, prior)) and (vis.read(np.uint8, n) == 7).all()
    for b in stats + [vis, drec, dabs, dgrec]:
        b.destroy()
