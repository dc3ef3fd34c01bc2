"""The composite backward differentiates the function the forward computed: at every pixel it consumes the list entries the
forward consumed, whichever forward kernel drew the frame (k_composite or k_composite_px, forced with splat_composite_options
or picked by screen size) and whichever entry points drew and differentiated it (splat_composite_aov with and without the
depth buffer, splat_composite_backward and splat_composite_backward_depth).

Both sides are observed through the public ABI only, at target pixels whose lists share no splat:
  forward   an entry was consumed exactly when changing its colour changes the pixel (colour enters neither T nor the stop);
  backward  with the upstream gradient non-zero only at the targets, an entry inside the cut was consumed exactly when its
            grad_color_opacity rgb is non-zero.
The pixels are (a) hand-built stacks whose last entry leaves T within a few ulps of T_STOP under the two kernels' update orders,
some stopping under one order and not the other (tests/grad_decisions_ref.py), and (b) the near and rim pixels of random
scenes, the pixels the other gradient tests give a zero upstream."""
import ctypes as C
import os

import numpy as np
import pytest

from oracle import np_oracle as NO
from splat_renderer_amd import _lib
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER
from tests import grad_decisions_ref as DR
from tests import test_gpu_ellipsoid_grad as TG

pytestmark = pytest.mark.gpu

PX_MIN_TILES = 2048  # csrc/composite_px.hip: the default forward is k_composite_px on screens of at least this many tiles
# routes: (name, kernel for splat_composite_options, screen); the last two are the default selection on both sides of 2048 tiles
ROUTES = [("quadrant", 0, (640, 360)), ("px", 1, (640, 360)), ("default-small", -1, (640, 360)), ("default-large", -1, (1024, 768))]
GEOMS = DR.GEOMS
TARGETS = ((3, 3), (12, 3), (3, 12), (12, 12))  # tile-local target pixels: their footprints stay inside the tile and apart
UP = np.array([1.0, -1.0, 0.5, 0.25], np.float32)  # the upstream at a target (rgb, alpha)


def route_order(kernel, w, h):
    """Which update order draws the frame: the forward's rule (composite_px.hip's composite_uses_px): the context's choice, else
    the SPLAT_COMPOSITE switch (pixel | quadrant), else the screen size."""
    if kernel == -1:
        forced = os.environ.get("SPLAT_COMPOSITE", "")[:1].lower()
        if forced in ("p", "q"):
            return "px" if forced == "p" else "quadrant"
        return "px" if -(-w // 16) * -(-h // 16) >= PX_MIN_TILES else "quadrant"
    return "px" if kernel == 1 else "quadrant"


class Frame:
    """Records, colours and lists on the device, with forward and backward calls on them."""

    def __init__(self, d, rec, col, counts, offsets, idx, w, h, z=None):
        self.d, self.w, self.h, self.n = d, w, h, rec.shape[0]
        self.col = np.ascontiguousarray(col, np.float32)
        self.z = np.ascontiguousarray(z if z is not None else np.linspace(1.0, 2.0, self.n), np.float32)
        self.bufs = [d.createBufferFrom(np.ascontiguousarray(a)) for a in
                     (rec, self.col, idx if idx.size else np.zeros(1, np.uint32), counts, offsets, self.z)]
        self.img, self.alpha = d.createBuffer(w * h * 16), d.createBuffer(w * h * 4)
        self.g, self.gd = d.createBuffer(w * h * 16), d.createBuffer(w * h * 4)
        self.grec, self.gcol, self.gz = d.createBuffer(self.n * 32), d.createBuffer(self.n * 16), d.createBuffer(self.n * 4)

    def lists(self):
        b = self.bufs
        return (b[0].ptr, b[2].ptr, b[3].ptr, b[4].ptr, self.w, self.h, None)

    def forward(self, col=None, depth=False, want_alpha=False):
        """(H, W, 4) image and (H, W) alpha (want_alpha; else None) of the forward with colours col (default: the frame's)."""
        d = self.d
        self.bufs[1].write(self.col if col is None else np.ascontiguousarray(col, np.float32))
        aov = _lib.Aov(None, self.alpha.ptr, None)
        if depth:
            rc = d.lib.splat_composite_aov_depth(d.ctx, C.byref(TG.cfg()), self.bufs[1].ptr, 1, None, 1, *self.lists(), self.img.ptr, None,
                                                  C.byref(aov), self.bufs[5].ptr, 1)
        else:
            rc = d.lib.splat_composite_aov(d.ctx, C.byref(TG.cfg()), self.bufs[1].ptr, 1, None, 1, *self.lists(), self.img.ptr, None,
                                           C.byref(aov))
        _lib.check(rc, d.ctx)
        alpha = self.alpha.read(np.float32, self.h * self.w).reshape(self.h, self.w) if want_alpha else None
        return self.img.read(np.float32, self.h * self.w * 4).reshape(self.h, self.w, 4), alpha

    def backward(self, g, depth=False, gd=None):
        """(grad_records (n, 8), grad_color_opacity (n, 4)) for upstream g (H, W, 4), added into zeros."""
        d = self.d
        self.bufs[1].write(self.col)
        self.g.write(np.ascontiguousarray(g, np.float32))
        for b in (self.grec, self.gcol, self.gz):
            b.zero()
        b = self.bufs
        args = (d.ctx, C.byref(TG.cfg()), b[1].ptr, 1, b[0].ptr, b[2].ptr, b[3].ptr, b[4].ptr, self.w, self.h, self.g.ptr, self.n,
                self.grec.ptr, self.gcol.ptr)
        if depth:
            self.gd.write(np.ascontiguousarray(gd if gd is not None else np.zeros((self.h, self.w)), np.float32))
            rc = d.lib.splat_composite_backward_depth(*args, b[5].ptr, 1, self.gd.ptr, self.gz.ptr)
        else:
            rc = d.lib.splat_composite_backward(*args)
        _lib.check(rc, d.ctx)
        return self.grec.read(np.float32, self.n * 8).reshape(self.n, 8), self.gcol.read(np.float32, self.n * 4).reshape(self.n, 4)

    def destroy(self):
        for b in self.bufs + [self.img, self.alpha, self.g, self.gd, self.grec, self.gcol, self.gz]:
            b.destroy()


def with_kernel(d, kernel):
    _lib.check(d.lib.splat_composite_options(d.ctx, kernel, 0, -1), d.ctx)


def consumed_forward(fr, probes, depth, base=None):
    """probes: per render, {pixel (y, x): splat} (at most one changed splat per pixel).  Returns {(pixel, splat): changed}.
    base: the image with the frame's own colours, if already rendered."""
    if base is None:
        base, _ = fr.forward(depth=depth)
    out = {}
    for probe in probes:
        col = fr.col.copy()
        for s in probe.values():
            col[s, :3] += 0.5
        img, _ = fr.forward(col, depth=depth)
        for (y, x), s in probe.items():
            out[((y, x), s)] = not np.array_equal(img[y, x, :3], base[y, x, :3])
    return out


def consumed_backward(fr, pixels, cands, depth):
    """{(pixel, splat): grad rgb non-zero} for every candidate of every target pixel (lists pairwise disjoint)."""
    g = np.zeros((fr.h, fr.w, 4), np.float32)
    gd = np.zeros((fr.h, fr.w), np.float32)
    for (y, x) in pixels:
        g[y, x] = UP
        gd[y, x] = 0.75
    grec, gcol = fr.backward(g, depth=depth, gd=gd)
    return {(p, s): bool((gcol[s, :3] != 0).any()) for p in pixels for s in cands[p]}, (grec, gcol)


# ---- (a) hand-built stacks ---------------------------------------------------------------------------------------------------
def measure_g(d, w, h):
    """The hardware footprint value of each GEOMS entry: at a single-entry pixel with opacity 1 the alpha AOV is 1 - (1 - g) = g
    exactly (Sterbenz: g >= 0.5), under both kernels."""
    recs, cols = [], []
    for k, (b, dl) in enumerate(GEOMS):
        x, y = 16 * k + 3, 3
        recs.append([x + 0.5 + dl, y + 0.5, b, 0, 0, b, 0, 0])
        cols.append([0.2, 0.2, 0.2, 1.0])
    rec, col = np.array(recs, np.float32), np.array(cols, np.float32)
    ntx, nty = -(-w // 16), -(-h // 16)
    counts = np.zeros(ntx * nty, np.uint32)
    counts[:len(GEOMS)] = 1
    offsets = np.zeros(ntx * nty + 1, np.uint32)
    offsets[1:] = np.cumsum(counts)
    idx = np.arange(len(GEOMS), dtype=np.uint32)
    fr = Frame(d, rec, col, counts, offsets, idx, w, h)
    gs = []
    try:
        for kernel in (0, 1):
            with_kernel(d, kernel)
            _, alpha = fr.forward(want_alpha=True)
            gs.append([alpha[3, 16 * k + 3] for k in range(len(GEOMS))])
    finally:
        with_kernel(d, -1)
        fr.destroy()
    assert gs[0] == gs[1], "the two kernels evaluate the stack footprints differently"
    for (b, dl), g in zip(GEOMS, gs[0]):
        u = np.float32(np.float32(b) * np.float32(-dl))
        assert g in DR.g_candidates(np.float32(u * u)), (b, dl, g)
    return [float(g) for g in gs[0]]


def build_stacks(gvals, w, h, seed):
    """Records, colours and lists of the stacks of DR.search on a w x h screen, four per tile.  Returns the frame's arrays and
    per stack (pixel (y, x), splat indices in list order, opacities, kind)."""
    rng = np.random.default_rng(seed)
    stacks = []
    for gi, g in enumerate(gvals):
        for kind, ops in DR.search(g, rng, want=12):
            stacks.append((gi, kind, ops))
    ntx, nty = -(-w // 16), -(-h // 16)
    assert len(stacks) <= 4 * ntx * nty
    recs, cols, placed = [], [], []
    tile_lists = [[] for _ in range(ntx * nty)]
    for k, (gi, kind, ops) in enumerate(stacks):
        t, slot = divmod(k, 4)
        tx, ty = t % ntx, t // ntx
        x, y = tx * 16 + TARGETS[slot][0], ty * 16 + TARGETS[slot][1]
        b, dl = GEOMS[gi]
        ids = []
        for o in ops:
            ids.append(len(recs))
            recs.append([x + 0.5 + dl, y + 0.5, b, 0, 0, b, 0, 0])
            cols.append([*rng.uniform(0.05, 0.45, 3), o])
        tile_lists[t] += ids
        placed.append(((y, x), ids, ops, kind, gvals[gi]))
    counts = np.array([len(l) for l in tile_lists], np.uint32)
    offsets = np.zeros(ntx * nty + 1, np.uint32)
    offsets[1:] = np.cumsum(counts)
    idx = np.array([i for l in tile_lists for i in l], np.uint32)
    return np.array(recs, np.float32), np.array(cols, np.float32), counts, offsets, idx, placed


def check_grads_at(fr, rec, gcol_got, grec_got, steps, pixels):
    """The backward's gradients against float64 over the forward's own consumed pairs, upstream UP at `pixels`."""
    g = np.zeros((fr.h, fr.w, 4), np.float32)
    for (y, x) in pixels:
        g[y, x] = UP
    want_rec, want_col = GR.composite_grads(rec, fr.col, steps, fr.w, fr.h, g)
    for name, got, want in [(f"rec[{k}]", grec_got[:, k], want_rec[:, k]) for k in TG.REC_COLS] + \
                           [(f"col[{k}]", gcol_got[:, k], want_col[:, k]) for k in range(4)]:
        assert TG.rel_l2(got, want) <= 1e-4, f"{name}: relative L2 {TG.rel_l2(got, want):.3g}"
        assert np.abs(got - want).max() <= 2e-3 * np.abs(want).max() + 1e-30, f"{name}: max {np.abs(got - want).max():.3g}"


@pytest.mark.parametrize("route,kernel,screen", ROUTES, ids=[r[0] for r in ROUTES])
def test_stacks_at_the_stop(device, route, kernel, screen):
    d = device
    w, h = screen
    gvals = measure_g(d, w, h)
    rec, col, counts, offsets, idx, placed = build_stacks(gvals, w, h, seed=7)
    order = route_order(kernel, w, h)
    fr = Frame(d, rec, col, counts, offsets, idx, w, h)
    try:
        with_kernel(d, kernel)
        maxlen = max(len(ids) for _, ids, _, _, _ in placed)
        probes = [{p: ids[j] for p, ids, _, _, _ in placed if j < len(ids)} for j in range(maxlen)]
        pixels = [p for p, *_ in placed]
        cands = {p: ids for p, ids, *_ in placed}
        seen = {}
        for depth in (False, True):
            fwd = consumed_forward(fr, probes, depth)
            bwd, _ = consumed_backward(fr, pixels, cands, depth)
            differ = [(p, kind) for p, ids, _, kind, _ in placed if any(fwd[(p, s)] != bwd[(p, s)] for s in ids)]
            seen[depth] = (fwd, bwd, differ)
        fwd, bwd, differ = seen[False]
        assert seen[True][0] == fwd, "splat_composite_aov_depth consumed other entries than splat_composite_aov"
        # the forward consumed what the exact model of its update order says: the stacks straddle T_STOP on the hardware too
        for p, ids, ops, kind, g in placed:
            L, _ = DR.walk(g, ops, order)
            assert [fwd[(p, s)] for s in ids] == [j < L for j in range(len(ids))], (route, kind, p, ops)
        n_split = sum(kind == "split" for *_, kind, _ in placed)
        for depth in (False, True):
            differ = seen[depth][2]
            assert not differ, (f"{route}: backward{'_depth' if depth else ''} consumed other entries than the forward at "
                                f"{len(differ)} of {len(placed)} stacks ({n_split} split): {differ[:6]}")
        # the gradients at those pixels, against float64 over the forward's own decisions
        steps = []
        for p, ids, *_ in placed:
            taken = [s for s in ids if fwd[(p, s)]]
            for j, s in enumerate(taken):
                while len(steps) <= j:
                    steps.append(([], [], []))
                steps[j][0].append(p[0] * w + p[1])
                steps[j][1].append(s)
                steps[j][2].append(j == len(taken) - 1)
        steps = [(np.array(a, np.int64), np.array(b, np.int64), np.array(c)) for a, b, c in steps]
        g = np.zeros((h, w, 4), np.float32)
        for p in pixels:
            g[p] = UP
        grec, gcol = fr.backward(g)
        check_grads_at(fr, rec, gcol, grec, steps, pixels)
    finally:
        with_kernel(d, -1)
        fr.destroy()


# ---- (b) near and rim pixels of random scenes -------------------------------------------------------------------------------
# (n, w, h, seed, spread, scale): the dense scene has near pixels by the thousand; every near, rim and box-edge pixel is compared
SCENES = [(20000, 640, 360, 5, 1.2, 0.015), (8000, 1024, 768, 12, 1.2, 0.012)]


def box_edge_pixels(rec, w, h):
    """Pixels whose centre lies within 1e-3 px of an edge of some splat's exact 3-sigma box (the binner's and the kernels' box
    tests meet there) and whose float64 d2 for that splat is at most 1.05."""
    bnd, okb = NO.disc_bounds(rec)
    r64 = rec.astype(np.float64)
    out = set()
    for s in np.nonzero(okb)[0]:
        x0, y0, x1, y1 = (float(v) for v in bnd[s])
        pts = []
        for e in (x0, x1):
            if abs(e - 0.5 - round(e - 0.5)) < 1e-3:
                pts += [(y, round(e - 0.5)) for y in range(max(int(np.ceil(y0 - 0.5)), 0), min(int(np.floor(y1 - 0.5)), h - 1) + 1)]
        for e in (y0, y1):
            if abs(e - 0.5 - round(e - 0.5)) < 1e-3:
                pts += [(round(e - 0.5), x) for x in range(max(int(np.ceil(x0 - 0.5)), 0), min(int(np.floor(x1 - 0.5)), w - 1) + 1)]
        for y, x in pts:
            if 0 <= x < w and 0 <= y < h:
                dx, dy = x + 0.5 - r64[s, 0], y + 0.5 - r64[s, 1]
                if (r64[s, 2] * dx + r64[s, 3] * dy) ** 2 + (r64[s, 5] * dy) ** 2 <= 1.05:
                    out.add((int(y), int(x)))
    return out


def scene_targets(rec, col, idx, counts, offsets, w, h):
    """Every near and rim pixel (ellipsoid_grad_ref.decisions) and every box-edge pixel, with its candidates: the entries of its
    tile list (in list order) whose box, grown by one pixel, holds its centre and whose float64 d2 is at most 1.05 — every entry
    either kernel could take there.  Packed into groups whose candidate lists are pairwise disjoint."""
    dec = GR.decisions(rec, col, idx, counts, offsets, w, h)
    bnd, okb = NO.disc_bounds(rec)
    edge = box_edge_pixels(rec, w, h)
    ys, xs = np.nonzero(dec["near"] | dec["rim"])
    pts = sorted(set(zip(ys.tolist(), xs.tolist())) | edge)
    ntx = -(-w // 16)
    r64 = rec.astype(np.float64)
    cands = {}
    for y, x in pts:
        t = (y // 16) * ntx + x // 16
        lst = idx[offsets[t]:offsets[t] + counts[t]].astype(np.int64)
        b = bnd[lst]
        cx, cy = x + 0.5, y + 0.5
        inb = okb[lst] & (cx >= b[:, 0] - 1) & (cx <= b[:, 2] + 1) & (cy >= b[:, 1] - 1) & (cy <= b[:, 3] + 1)
        r = r64[lst]
        dx, dy = cx - r[:, 0], cy - r[:, 1]
        uu, vv = r[:, 2] * dx + r[:, 3] * dy, r[:, 5] * dy
        c = lst[inb & (uu * uu + vv * vv <= 1.05)]
        cands[(y, x)] = c
    groups, used = [], []
    for p, c in cands.items():
        cs = set(c.tolist())
        for gi, grp in enumerate(groups):
            if not (used[gi] & cs):
                grp.append(p)
                used[gi] |= cs
                break
        else:
            groups.append([p])
            used.append(cs)
    return dec, edge, cands, groups


def probes_for(rec, c, p, took):
    """The candidates of pixel p (list order) whose forward consumption must be observed to know that the forward consumed what
    the backward did (took: the backward's verdict per candidate).  An entry with float64 d2 < 0.99 is inside the cut for both
    kernels ("sure"); consumed sets are prefixes of the in-cut entries.  So: the last sure entry at or before the backward's
    last consumed one (a) and the first sure entry after it (b), every entry between them, and every entry before (a) that is
    not sure.  If the forward consumed (a) and not (b) it agrees with the backward on all the sure entries, and the rest are
    observed."""
    if len(c) == 0:
        return []
    r = rec[c].astype(np.float64)
    dx, dy = p[1] + 0.5 - r[:, 0], p[0] + 0.5 - r[:, 1]
    sure = (r[:, 2] * dx + r[:, 3] * dy) ** 2 + (r[:, 5] * dy) ** 2 < 0.99
    last = max([j for j, t in enumerate(took) if t], default=-1)
    a = max([j for j in range(last + 1) if sure[j]], default=-1)
    b = next((j for j in range(last + 1, len(c)) if sure[j]), len(c) - 1)
    keep = [j for j in range(len(c)) if (j < a and not sure[j]) or a <= j <= b]
    if a < 0:
        keep = list(range(b + 1))
    return [c[j] for j in keep]


def group_steps(grp, cands, bwd, w):
    """ellipsoid_grad_ref steps over the pairs the backward consumed at the group's pixels (checked equal to the forward's)."""
    steps = []
    for (y, x) in grp:
        taken = [s for s in cands[(y, x)] if bwd[((y, x), s)]]
        for j, s in enumerate(taken):
            while len(steps) <= j:
                steps.append(([], [], []))
            steps[j][0].append(y * w + x)
            steps[j][1].append(s)
            steps[j][2].append(j == len(taken) - 1)
    return [(np.array(a, np.int64), np.array(b, np.int64), np.array(c, bool)) for a, b, c in steps]


@pytest.mark.parametrize("route,kernel,screen", ROUTES, ids=[r[0] for r in ROUTES])
def test_near_and_rim_pixels(device, route, kernel, screen):
    d = device
    w, h = screen
    n, sw, sh, seed, spread, scale = next(s for s in SCENES if (s[1], s[2]) == (w, h))
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale)
    u = TG.camera_u(w, h)
    rec, counts, offsets, idx = TG.lists(u, pos, scl, rot, w, h)
    dec, edge, cands, groups = scene_targets(rec, col, idx, counts, offsets, w, h)
    assert len(cands) >= 1000 and len(edge) >= 10
    fr = Frame(d, rec, col, counts, offsets, idx, w, h)
    compared, differ, graded = set(), [], 0
    try:
        with_kernel(d, kernel)
        base = {depth: fr.forward(depth=depth)[0] for depth in (False, True)}
        for gi, grp in enumerate(groups):
            depth = bool(gi % 2)  # (both backward entry points, and both forward ones, alternating)
            bwd, (grec, gcol) = consumed_backward(fr, grp, cands, depth)
            todo = {p: probes_for(rec, cands[p], p, [bwd[(p, s)] for s in cands[p]]) for p in grp}
            nprobe = max(len(v) for v in todo.values())
            probes = [{p: v[j] for p, v in todo.items() if j < len(v)} for j in range(nprobe)]
            fwd = consumed_forward(fr, probes, not depth, base[not depth])
            for p in grp:
                compared.add(p)
                bad = [s for s in todo[p] if fwd[(p, s)] != bwd[(p, s)]]
                if bad:
                    differ.append((p, bad))
            if not depth and not differ:
                # the gradients at these pixels against float64 over the same pairs (the colour-only backward: upstream UP)
                steps = group_steps(grp, cands, bwd, w)
                pixels = np.sort(np.array([y * w + x for y, x in grp], np.int64))
                g = np.zeros((h, w, 4), np.float32)
                g.reshape(-1, 4)[pixels] = UP
                want_rec, want_col = GR.composite_grads(rec, col, steps, w, h, g, pixels=pixels)
                for name, got, want in [(f"rec[{k}]", grec[:, k], want_rec[:, k]) for k in TG.REC_COLS] + \
                                       [(f"col[{k}]", gcol[:, k], want_col[:, k]) for k in range(4)]:
                    assert TG.rel_l2(got, want) <= 1e-4, f"{route} group {gi} {name}: relative L2 {TG.rel_l2(got, want):.3g}"
                    assert np.abs(got - want).max() <= 2e-3 * np.abs(want).max() + 1e-30, f"{route} group {gi} {name}"
                graded += len(grp)
    finally:
        with_kernel(d, -1)
        fr.destroy()
    near = set(zip(*(a.tolist() for a in np.nonzero(dec["near"]))))
    rim = set(zip(*(a.tolist() for a in np.nonzero(dec["rim"]))))
    assert near <= compared and rim <= compared and edge <= compared  # every one of them, none dropped
    print(f"{route}: {len(compared)} pixels compared ({len(near)} near, {len(rim)} rim, {len(edge)} box-edge) in {len(groups)} "
          f"groups, {graded} with gradients against float64; {len(differ)} consumed sets differ")
    assert not differ, f"{route}: {len(differ)} of {len(compared)} pixels: {differ[:5]}"
