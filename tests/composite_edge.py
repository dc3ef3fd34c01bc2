"""Adversarial record sets for the composite (ComputeShaderRenderer.ts:97-198), and a float64 evaluation of it.

Every scene is a set of 8-float ProjectedSplat records {min x, min y, max x, max y, depth, screen radius, index, 0} with a
colour and a normal per record, on a screen of w x h pixels.  Records the projector could have made are CONSISTENT:
formed from {centre x, y, radius, depth} as oracle.c:form_record forms them (bounds = c -/+ 1.5 r, one f32 rounding per
operation), so they can also be given to the composite as 16-byte COMPACT and 32-byte LIT32 records.  Family d's records
are not: their boxes are free (what the staged API accepts in a PROJECTED buffer).  Record i has depth 1 + i / 1024, so
the oracle's depth sort keeps the records in the order they were built.

Families (ISSUE: "Hold every composite kernel to the oracle at pixel, tile and list edges"):
  a  box edges: min or max of a box, on either axis, bisected in f32 onto a pixel centre x + 0.5, one ulp either side of
     it and +-0.5 px from it — at the first and last pixel of a tile, pixel 0, the screen's last (partial-tile) pixel and
     beyond the screen; on a screen of ordinary size and on one 4100 px wide (ulp(x) = 2^-11 there);
  b  radius and non-finite values: r at the 0.5 cull, one ulp either side, r << 0.5 over pixel centres, r so large that
     one record covers the screen, NaN / +-inf in a bound, the radius or the centre, negative r; opacity 0, 1, 2, -1
     (the reference never reads it); colours above 1 and below 0; zero and NaN normals;
  c  list lengths: one tile per length (1, 31, 32, 33, 63-65, 95-97, 255-257, 4097) — the 32-entry chunks of
     k_composite_px and the 256-entry batches of k_composite / k_composite_tile — and tiles whose centre pixel's
     1 - T reaches 0.99 (float32, the oracle's arithmetic) exactly at list entry 30, 31, 32, 254, 255 or 256, or just not;
  d  free boxes (PROJECTED only): half-widths 3 r, 10 r, 100 r and 0.5 r, r in [0.5, 4]; centres off the screen with
     boxes that cover it.

Used by tests/test_composite_edges_cpu.py (the oracle against composite_f64) and tests/test_gpu_composite_edges.py
(the kernels).  Nothing here is part of the product or of the oracle.
"""
import numpy as np

from oracle import oracle as O

F = np.float32
PAD = F(1.5)  # SplatProjector.ts:119 / oracle.c:152


def nextup(x):
    return np.nextafter(F(x), F(np.inf))


def nextdown(x):
    return np.nextafter(F(x), F(-np.inf))


class Scene:
    """Records built in list (depth) order.  cen: {cx, cy, r} per record (NaN rows for free boxes)."""

    def __init__(self, name, w, h, seed=0):
        self.name, self.w, self.h = name, w, h
        self.rng = np.random.default_rng(seed)
        self.bounds, self.rad, self.cen, self.col, self.nrm, self.tag = [], [], [], [], [], []
        self.free = False

    def _extras(self, n, col=None, nrm=None):
        if col is None:
            col = np.ones((n, 4), F)
            col[:, :3] = self.rng.uniform(0.1, 1.0, (n, 3))
        if nrm is None:
            v = self.rng.standard_normal((n, 3))
            nrm = np.ones((n, 4), F)
            nrm[:, :3] = v / np.linalg.norm(v, axis=1, keepdims=True)
        self.col.append(np.asarray(col, F).reshape(n, 4))
        self.nrm.append(np.asarray(nrm, F).reshape(n, 4))

    def add(self, cx, cy, r, tag, col=None, nrm=None):
        """Consistent records: bounds formed from the centre and radius exactly as the projector does."""
        cx, cy, r = np.broadcast_arrays(np.asarray(cx, F), np.asarray(cy, F), np.asarray(r, F))
        n = cx.size
        cx, cy, r = cx.ravel().astype(F), cy.ravel().astype(F), r.ravel().astype(F)
        with np.errstate(invalid="ignore", over="ignore"):
            p = r * PAD
            self.bounds.append(np.stack([cx - p, cy - p, cx + p, cy + p], axis=1).astype(F))
        self.rad.append(r)
        self.cen.append(np.stack([cx, cy, r], axis=1))
        self.tag += [tag] * n
        self._extras(n, col, nrm)

    def add_free(self, bounds, r, tag, col=None, nrm=None):
        """Free boxes: any bounds, any radius (PROJECTED records only)."""
        b = np.asarray(bounds, F).reshape(-1, 4)
        n = b.shape[0]
        self.free = True
        self.bounds.append(b)
        self.rad.append(np.broadcast_to(np.asarray(r, F), (n,)).astype(F))
        self.cen.append(np.full((n, 3), np.nan, F))
        self.tag += [tag] * n
        self._extras(n, col, nrm)

    def arrays(self):
        """(records (n, 8), compact (n, 4) or None, colours (n, 4), normals (n, 4), tags)."""
        b = np.concatenate(self.bounds)
        n = b.shape[0]
        rec = np.zeros((n, 8), F)
        rec[:, :4] = b
        rec[:, 4] = 1.0 + np.arange(n, dtype=np.float64) / 1024.0
        rec[:, 5] = np.concatenate(self.rad)
        rec[:, 6] = np.arange(n, dtype=np.uint32).view(F)
        cen = np.concatenate(self.cen)
        compact = None
        if not self.free:
            compact = np.zeros((n, 4), F)
            compact[:, :3] = cen
            compact[:, 3] = rec[:, 4]
            # the records the composite rebuilds from the compact ones must be these (oracle.c:form_record)
            assert np.array_equal(O.expand_compact(compact).view(np.uint32), rec.view(np.uint32))
        return rec, compact, np.concatenate(self.col), np.concatenate(self.nrm), np.array(self.tag)


def lit32(compact, col, nrm):
    """LIT32 records {cx, cy, r, depth | lit rgb, opacity}: the reference's shading (ComputeShaderRenderer.ts:143-145)
    in one f32 operation per operator, max() dropping a NaN as oracle.c and lit_color (shade.h) do."""
    k = F(0.577350269189625764)
    with np.errstate(invalid="ignore", over="ignore"):
        ndl = (nrm[:, 0] * k + nrm[:, 1] * k) + nrm[:, 2] * k
        kd = F(0.85) + F(0.15) * np.fmax(ndl, F(0))
        out = np.empty((compact.shape[0], 8), F)
        out[:, :4] = compact
        out[:, 4:7] = col[:, :3] * kd[:, None]
    out[:, 7] = col[:, 3]
    return out


def lists(rec, w, h, tile):
    """The oracle's tile lists of the records in depth order: (counts, offsets, indices)."""
    keys, pay = O.extract_keys(rec)
    _, order = O.sort_pairs(keys, pay)
    return O.bin_sorted(rec, order, w, h, tile)


# ---- family a: box edges -------------------------------------------------------------------------------------------

def bisect_f32(f, lo, hi, target):
    """Adjacent f32 brackets (a, b) of the rising f's crossing of target: f(a) < target <= f(b), vectorised."""
    lo, hi = np.asarray(lo, F).copy(), np.asarray(hi, F).copy()
    for _ in range(200):
        mid = ((lo.astype(np.float64) + hi.astype(np.float64)) * 0.5).astype(F)
        live = (mid != lo) & (mid != hi)
        if not live.any():
            break
        below = f(mid) < target
        lo = np.where(live & below, mid, lo)
        hi = np.where(live & ~below, mid, hi)
    return lo, hi


def edge_targets(col):
    """A pixel centre, one ulp either side of it, and +-0.5 px from it."""
    c = F(col) + F(0.5)
    return np.array([c, nextup(c), nextdown(c), c + F(0.5), c - F(0.5)], F)


def centres_for_edge(target, r, side):
    """Centres c (both f32 brackets) whose box edge c - 1.5 r (side 0) or c + 1.5 r (side 1) meets target."""
    target = np.asarray(target, F)
    r = np.broadcast_to(np.asarray(r, F), target.shape).astype(F)
    p = r * PAD
    sgn = F(1.0) if side == 0 else F(-1.0)
    f = (lambda c: c - p) if side == 0 else (lambda c: c + p)
    guess = target + sgn * p
    a, b = bisect_f32(f, guess - F(4.0), guess + F(4.0), target)
    return np.concatenate([a, b]), np.concatenate([r, r])


def edge_columns(w, tiles=(16,)):
    """Pixel columns where a box edge is interesting: pixel 0, the first and last column of tiles (for every tile size
    asked for), the screen's last pixel, and beyond the screen on both sides."""
    cols = {0, -1, -3, w - 1, w, w + 2}
    for t in tiles:
        for k in (1, 2, (w // t) - 1, w // t):
            for c in (k * t - 1, k * t):
                if 0 <= c < w:
                    cols.add(c)
    return sorted(cols)


def family_a(w, h, tiles=(16, 8, 10, 24, 32, 64), seed=1, radii=(0.5, 0.75, 1.3, 3.7, 11.0), name="a"):
    """Box edges on pixel centres.  Each record has one box edge (min x, max x, min y or max y) aimed at a target; the
    other axis is either aimed too (both axes) or placed at random inside the screen (one axis only)."""
    sc = Scene(name, w, h, seed)
    rng = sc.rng
    for axis in (0, 1):
        size, other = (w, h) if axis == 0 else (h, w)
        for col in edge_columns(size, tiles):
            for side in (0, 1):
                for r in radii:
                    c, rr = centres_for_edge(edge_targets(col), r, side)
                    o = rng.uniform(-0.3 * r, other + 0.3 * r, c.shape[0]).astype(F)
                    cx, cy = (c, o) if axis == 0 else (o, c)
                    sc.add(cx, cy, rr, f"edge{'xy'[axis]}{side}")
    # both axes on edges at once: corners of tiles and of the screen
    for side in (0, 1):
        for r in (0.5, 2.1):
            xs = np.array([0, 15, 16, w - 1], F)
            ys = np.array([0, 15, 16, h - 1], F)
            cx, rx = centres_for_edge(np.concatenate([edge_targets(x) for x in xs]), r, side)
            cy, _ = centres_for_edge(np.concatenate([edge_targets(y) for y in ys]), r, side)
            sc.add(cx, cy, rx, "corner")
    return sc


# ---- family b: radius and non-finite values ------------------------------------------------------------------------

def family_b(w=70, h=52, seed=2):
    sc = Scene("b", w, h, seed)
    rng = sc.rng
    half = F(0.5)
    # the :127-129 cull: r at 0.5 and one ulp either side, centred on and between pixel centres
    for r in (half, nextdown(half), nextup(half), F(0.4999), F(0.5001)):
        for cx, cy in ((10.5, 10.5), (11.0, 10.5), (20.25, 30.75), (0.5, 0.5), (w - 0.5, h - 0.5)):
            sc.add(cx, cy, r, "r_cull")
    # r far below 0.5 over pixel centres: the box still holds a pixel centre, the splat is culled
    sc.add([30.5, 31.5, 32.5], [5.5, 5.5, 5.5], [0.1, 1e-6, 0.0], "r_tiny")
    sc.add([33.5], [5.5], [-0.0], "r_tiny")
    # negative radii: the box is inverted (min > max), the binner drops them
    sc.add([40.5, 41.5], [6.5, 6.5], [-1.0, -np.inf], "r_negative")
    # opacity 0, 1, above 1, negative (the reference never reads it); colours above 1 and below 0; zero / NaN normals
    for i, op in enumerate((0.0, 1.0, 2.0, -1.0)):
        c = np.array([[1.7, -0.4, 0.6, op]], F)
        sc.add([12.5 + 9 * i], [25.3], [2.5], "opacity", col=c)
    for i, nv in enumerate(([0.0, 0.0, 0.0], [np.nan, 0.0, 1.0], [np.nan] * 3, [1.0, 1.0, 1.0], [-1.0, -1.0, -1.0])):
        n = np.array([nv + [1.0]], F)
        c = np.array([[3.0, -2.0, 0.25, 1.0]], F)
        sc.add([8.5 + 11 * i], [40.0], [3.0], "normal", col=c, nrm=n)
    # NaN / inf in the centre: bounds NaN (dropped by the binner) or +-inf
    sc.add([np.nan, 20.0, np.inf, -np.inf], [20.0, np.nan, 20.0, 20.0], [2.0, 2.0, 2.0, 2.0], "c_nonfinite")
    # a few ordinary splats in between, so that later records have something to cover
    sc.add(rng.uniform(0, w, 24), rng.uniform(0, h, 24), rng.uniform(0.5, 3.0, 24), "plain")
    # records that cover the whole screen: r = 1e6, 2^24, then a NaN radius and r = inf (NaN centre): last in depth order,
    # so that they can only darken what is already there — nearest-on-top they come last, the literal blend ends with them
    sc.add([w / 2, -1e5], [h / 2, h / 2], [1e6, 2.0 ** 24], "r_huge")
    sc.add([w * 0.3], [h * 0.7], [np.inf], "r_inf")
    return sc


def family_b_free(w=70, h=52, seed=3):
    """NaN / inf in a bound, and NaN radius with finite bounds (PROJECTED only)."""
    sc = Scene("b_free", w, h, seed)
    rng = sc.rng
    inf, nan = np.inf, np.nan
    sc.add_free([[-inf, 10.0, 20.7, 20.0], [30.0, -inf, 40.0, 30.0], [44.2, 3.0, inf, 12.0], [5.0, 44.0, 12.0, inf]], 3.0, "b_inf")
    sc.add_free([[nan, 10.0, 20.7, 20.0], [30.0, 10.0, nan, 20.0], [nan, nan, nan, nan]], 3.0, "b_nan")
    lo = rng.uniform(0, 1, (16, 2)) * [w, h]
    sc.add_free(np.c_[lo, lo + rng.uniform(2, 20, (16, 2))], rng.uniform(0.5, 3, 16), "plain")
    sc.add_free([[50.0, 30.0, 60.0, 40.0]], np.nan, "r_nan")
    sc.add_free([[-inf, -inf, inf, inf]], 2.0, "b_all_inf")
    return sc


# ---- family c: list lengths and the stop ---------------------------------------------------------------------------

LENGTHS = (1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 255, 256, 257, 4097)


def family_c(seed=4):
    """One 16 x 16 tile per list length; every record's box lies inside its tile (r in [0.5, 3.5], centre at least
    1.5 r + 0.5 from the tile's edges), so each tile's list is exactly its records."""
    ntx = 4
    nty = -(-len(LENGTHS) // ntx)
    sc = Scene("c", ntx * 16, nty * 16 - 5, seed)  # (the last row of tiles is partial)
    rng = sc.rng
    for t, n in enumerate(LENGTHS):
        x0, y0 = (t % ntx) * 16, (t // ntx) * 16
        r = rng.uniform(0.5, 3.5, n).astype(F)
        m = r * 1.5 + 0.5
        ymax = min(16.0, sc.h - y0)
        sc.add(x0 + rng.uniform(m, 16 - m), y0 + rng.uniform(np.minimum(m, ymax / 2), np.maximum(ymax - m, ymax / 2)), r, f"len{n}")
    return sc


STOP_AT = (30, 31, 32, 254, 255, 256)  # list positions (0-based) of the entry at which the pixel's 1 - T reaches 0.99


def _centre_pixel_stop(recs, w, h, px, py, mode):
    """List position after which pixel (px, py) stops, by the oracle, for records laid one tile's list."""
    n = recs.shape[0]
    rec = np.zeros((n, 8), F)
    rec[:, :4] = recs[:, :4]
    rec[:, 5] = recs[:, 5]
    rec[:, 6] = np.arange(n, dtype=np.uint32).view(F)
    col = np.ones((n, 4), F)
    nrm = np.zeros((n, 4), F)
    idx = np.arange(n, dtype=np.uint32)
    out = O.composite(mode, True, col, nrm, rec, idx, np.array([n], np.uint32), np.zeros(1, np.uint32), w, h, tile=w,
                      want_u8=False, want_stops=True)
    return int(out[3][py, px])


def family_c_stop(mode=O.MODE_FRONT_TO_BACK, seed=5):
    """Tiles whose centre pixel (8, 8) reaches the stop exactly at entry m (m in STOP_AT), and, on the next tile, with the
    same records but the m-th moved one f32 step further from the pixel: there 1 - T stays just below 0.99 at entry m.
    Entries before m are one record, repeated, diagonally at a distance that leaves 1 - T a little short of 0.99; entries after m
    (40 of them) cover the pixel too.  Bisected through the oracle itself (its expf, its operation order)."""
    ntx = 4
    ntiles = 2 * len(STOP_AT)
    sc = Scene(f"c_stop{mode}", ntx * 16, -(-ntiles // ntx) * 16, seed)
    r = F(2.5)
    p = r * PAD
    for t, m in enumerate(STOP_AT):
        # g per repeated entry such that 1 - T after m entries is ~0.98; its centre offset d along x: g = exp(-2 (d / r)^2)
        g = 1.0 - 0.02 ** (1.0 / m)
        d = F(r * np.sqrt(-np.log(g) / 2.0) / np.sqrt(2.0))  # (along the diagonal: every box stays inside the tile)
        for variant in (0, 1):
            tt = 2 * t + variant
            x0, y0 = (tt % ntx) * 16, (tt // ntx) * 16
            cx0, cy0 = F(x0 + 8.5), F(y0 + 8.5)
            def stop_with(dm):
                # the tile's records as the scene will hold them, then moved to a one-tile screen at the origin (x0, y0 are
                # multiples of 16 and every value here is below 2^7: the shift is exact, every f32 operation the same)
                cx = np.concatenate([np.full(m, cx0 + d, F), [cx0 - dm]]).astype(F)
                cy = np.concatenate([np.full(m, cy0 + d, F), [cy0]]).astype(F)
                rows = np.zeros((m + 2, 6), F)
                rows[:m + 1, :4] = np.stack([cx - p, cy - p, cx + p, cy + p], axis=1)
                rows[:m + 1, :4] -= np.array([x0, y0, x0, y0], F)
                rows[m + 1, :4] = [100.0, 100.0, 101.0, 101.0]  # (one entry more, off the pixel: a pixel that does not stop visits it)
                rows[:, 5] = r
                return _centre_pixel_stop(rows, 16, 16, 8, 8, mode)

            # the m-th entry's offset dm: at 0 it stops the pixel (g = 1), at 1.5 r - 0.01 it does not; bisect in f32
            lo, hi = F(0.0), F(p - F(0.01))
            if stop_with(lo) != m + 1 or stop_with(hi) == m + 1:
                continue
            for _ in range(100):
                mid = F((float(lo) + float(hi)) * 0.5)
                if mid in (lo, hi):
                    break
                if stop_with(mid) == m + 1:
                    lo = mid
                else:
                    hi = mid
            dm = lo if variant == 0 else hi
            cx = np.concatenate([np.full(m, cx0 + d, F), [cx0 - dm], cx0 + sc.rng.uniform(-2, 2, 40).astype(F)])
            cy = np.concatenate([np.full(m, cy0 + d, F), [cy0], cy0 + sc.rng.uniform(-2, 2, 40).astype(F)])
            sc.add(cx, cy, r, f"stop{m}_{variant}", col=np.ones((cx.shape[0], 4), F))
    return sc


# ---- family d: free boxes ------------------------------------------------------------------------------------------

def family_d(w=200, h=150, seed=6):
    sc = Scene("d", w, h, seed)
    rng = sc.rng
    for mult, n in ((3.0, 40), (10.0, 24), (100.0, 8), (0.5, 40)):
        r = rng.uniform(0.5, 4.0, n).astype(F)
        cx, cy = rng.uniform(0, w, n).astype(F), rng.uniform(0, h, n).astype(F)
        hw = (r * F(mult)).astype(F)
        sc.add_free(np.stack([cx - hw, cy - hw, cx + hw, cy + hw], axis=1), r, f"box{mult:g}r")
    # the smallest radius the cull keeps, boxes reaching far to the left / above the centre: the Gaussian there is 0
    for mult in (6.6, 8.0, 20.0, 60.0):
        r = F(0.5)
        cx, cy = rng.uniform(0.3 * w, w, 4).astype(F), rng.uniform(0.3 * h, h, 4).astype(F)
        hw = F(r * mult)
        sc.add_free(np.stack([cx - hw, cy - hw, cx + F(1.0), cy + F(1.0)], axis=1), r, f"reach{mult:g}r")
    # centres off the screen, boxes over it
    for cx, cy in ((-30.0, 75.0), (w + 40.0, 20.0), (100.0, -60.0), (50.0, h + 25.0), (-500.0, -400.0)):
        r = F(3.0)
        sc.add_free([[cx - 700.0, cy - 700.0, cx + 700.0, cy + 700.0]], r, "offscreen")
        sc.add_free([[-5.0, -5.0, w + 5.0, h + 5.0]], rng.uniform(10.0, 80.0), "offscreen_cover")
    return sc


def scenes():
    """name -> Scene, every family (family c's stop tiles for both blends: the literal alpha differs from 1 - T)."""
    out = [family_a(333, 211, radii=(0.5, 0.75, 1.3, 3.7)), family_a(4100, 136, tiles=(16, 64), radii=(0.5, 1.3, 5.0), name="a_wide"), family_b(),
           family_b_free(), family_c(), family_c_stop(O.MODE_FRONT_TO_BACK), family_c_stop(O.MODE_REFERENCE_LITERAL), family_d()]
    return {s.name: s for s in out}


# ---- float64 evaluation --------------------------------------------------------------------------------------------

EPS = 2.0 ** -24
# per covered entry: the f32 evaluations' error in the Gaussian, relative (expf / v_exp_f32 ~1 ulp; k_composite_px's tables
# are a recurrence of up to 8 steps of two multiplies, with exp2 arguments up to ~30 in magnitude: a few 1e-6)
REL_G = 2.0 ** -16
NEAR_MARGIN = 2e-5  # oracle.c ORC_STOP_MARGIN


def composite_f64(mode, early_out, rec, col, nrm, counts, offsets, indices, w, h, tile, px, py):
    """The composite (ComputeShaderRenderer.ts:97-198) at pixels (px, py), in float64 but for the box test, which is
    evaluated on the f32 values (membership is discrete and exact).  max(dot, 0) drops a NaN (oracle.c, shade.h).
    Returns (rgb (P, 3), bound (P,), near (P,)): bound is an upper bound on how far a correct f32 evaluation of the same
    formulas may be from this one — per covered entry, the Gaussian's sensitivity to the f32 centre (lo + hi) * 0.5 and
    pixel offset (ulps of |lo| + |hi| and of the offset, in the oracle's and the kernels' tile-local forms), to the
    radius's relative error and to the exponential's, times what the Gaussian multiplies (2 max|colour| T), plus the
    blend's own rounding.  near: the pixel's f64 alpha came within that bound (+ 2e-5) of 0.99 — a correct f32 evaluation
    may then stop an entry earlier or later (worth up to (1 - 0.99) times the colours, see the tests)."""
    px = np.asarray(px, np.int64)
    py = np.asarray(py, np.int64)
    ntx = -(-w // tile)
    P = px.shape[0]
    out = np.zeros((P, 3))
    bound = np.zeros(P)
    near = np.zeros(P, bool)
    inv3 = 1.0 / np.sqrt(3.0)
    tiles = (py // tile) * ntx + (px // tile)
    with np.errstate(all="ignore"):
        for t in np.unique(tiles):
            sel = np.nonzero(tiles == t)[0]
            pxf32, pyf32 = px[sel].astype(F) + F(0.5), py[sel].astype(F) + F(0.5)
            pxd, pyd = pxf32.astype(np.float64), pyf32.astype(np.float64)
            n = sel.shape[0]
            c = np.zeros((n, 3))
            alpha = np.zeros(n)
            trans = np.ones(n)
            bnd = np.zeros(n)
            abnd = np.zeros(n)  # bound on the error of 1 - T (alpha)
            live = np.ones(n, bool)
            lmax = np.full(n, 0.1)
            nr = np.zeros(n, bool)
            for s in indices[offsets[t]:offsets[t] + counts[t]]:
                if early_out and not live.any():
                    break
                r32 = rec[s]
                inside = ~((pxf32 < r32[0]) | (pxf32 > r32[2]) | (pyf32 < r32[1]) | (pyf32 > r32[3]))
                b = r32[:4].astype(np.float64)
                r = float(r32[5])
                g = np.zeros(n)
                lit = np.zeros(3)
                eg = np.zeros(n)
                if not (r < 0.5):
                    cx, cy = (b[0] + b[2]) * 0.5, (b[1] + b[3]) * 0.5
                    ox, oy = pxd - cx, pyd - cy
                    nd = np.sqrt(ox * ox + oy * oy) / r
                    g = np.where(inside, np.exp(-0.5 * nd * nd / 0.25), 0.0)
                    v = nrm[s, :3].astype(np.float64)
                    ndl = v[0] * inv3 + v[1] * inv3 + v[2] * inv3
                    kd = 0.85 + 0.15 * (ndl if ndl > 0.0 else 0.0)  # (NaN > 0 is false: max drops the NaN)
                    lit = col[s, :3].astype(np.float64) * kd
                    ex = EPS * (abs(b[0]) + abs(b[2])) + 4 * EPS * (np.abs(ox) + 16.0)
                    ey = EPS * (abs(b[1]) + abs(b[3])) + 4 * EPS * (np.abs(oy) + 16.0)
                    dnd = np.hypot(ex, ey) / r + 8 * EPS * nd
                    lo = np.maximum(nd - dnd, 0.0)
                    slope = 4.0 * (nd + dnd) * np.exp(-2.0 * lo * lo)  # |d gaussian / d nd| on [nd - dnd, nd + dnd]
                    eg = np.where(inside, slope * dnd + REL_G * g + 1e-30, 0.0)
                    eg = np.where(np.isfinite(eg), eg, 0.0)
                g = np.where(live, g, 0.0)
                eg = np.where(live, eg, 0.0)
                cov = live & (g != 0)
                L = max(float(np.nanmax(np.abs(lit))) if lit.size else 0.0, 0.1)
                lmax = np.where(cov, np.maximum(lmax, L), lmax)
                if mode == O.MODE_REFERENCE_LITERAL:
                    c = np.where(live[:, None], c * (1.0 - g)[:, None] + lit[None, :] * g[:, None], c)
                    alpha = np.where(live, alpha * (1.0 - g) + g, alpha)
                    abnd = abnd + eg + np.where(cov, 4 * EPS, 0.0)
                    bnd = bnd + 2.0 * lmax * eg + np.where(cov, 6 * EPS * lmax, 0.0)
                    a = alpha
                else:
                    wgt = np.minimum(trans + abnd, 1.0)
                    c = c + lit[None, :] * (trans * g)[:, None]
                    abnd = abnd + wgt * eg + np.where(cov, 4 * EPS, 0.0)
                    bnd = bnd + 2.0 * lmax * wgt * eg + np.where(cov, 6 * EPS * lmax, 0.0)
                    trans = trans * (1.0 - g)
                    a = 1.0 - trans
                nr |= live & (np.abs(a - 0.99) <= abnd + NEAR_MARGIN)
                if early_out:
                    live &= ~(a >= 0.99)
            rem = (1.0 - alpha) if mode == O.MODE_REFERENCE_LITERAL else trans
            out[sel] = c + np.array([0.05, 0.05, 0.1])[None, :] * rem[:, None]
            bound[sel] = bnd + 4 * EPS * lmax + 1e-7
            near[sel] = nr
    return out, bound, near


def near_tolerance(bound, mode):
    """A pixel whose alpha crosses 0.99 within the evaluations' noise may stop one entry earlier or later.  Nearest on
    top, what it then gains or loses is at most the remaining transmittance (1 - 0.99, plus the bound) times the largest
    colour (the scenes' lit colours stay within +-3.2).  The literal blend (:183-185) has no such bound: the entry after
    the stop replaces the colour by up to its Gaussian, so such a pixel is only held to the colours' range."""
    return bound + (0.0101 * 3.2 if mode == O.MODE_FRONT_TO_BACK else 6.4)
