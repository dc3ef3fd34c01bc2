"""Test-side restatement of the reference app's renderer (src/Renderer.ts:68-143,196-201,262-270; drawn by src/main.ts:183-190)
for tests/test_point_raster_cpu.py and tests/test_gpu_point_renderer.py.  Nothing under oracle/ is involved.

Per point i: n = normalize(gradient.yzw), the tangent frame of computeTangent, a quad of half-side s = 0.025 * scale with
corners p + (t ox s + b oy s), two triangles (-1,-1),(1,-1),(-1,1) and (-1,1),(1,-1),(1,1), clip = VP * corner.  The corners
are built in binary32 in the vertex stage's operation order (so the GPU's and these are the same numbers); everything after
that is f64: screen x = (x/w + 1) W/2, y = (1 - y/w) H/2, depth z/w interpolated linearly in screen space, pixel centres at
+0.5, the top-left fill rule of oracle.c's raster_tri.  A fragment survives when 0 <= depth < 1 and is nearer than what the
pixel holds ("less"; points drawn in index order, so on equal depth the lower index wins).  A quad with any corner at w <= 0
is dropped; a point whose normal, scale or corners are not finite covers nothing.  Colour n * 0.5 + 0.5 times
0.3 + 0.7 max(n . normalize(1,1,1), 0), alpha 1; clear (0.05, 0.05, 0.1, 1).

Where a different but correct rasteriser may differ, a pixel is CONTESTED:
  - its centre lies within EDGE_EPS = 2^-8 px of an edge of a triangle of some quad (covering it or not), or
  - its two nearest covering fragments (of different points) are less than DEPTH_EPS = 1e-6 apart, or a covering fragment's
    depth is within DEPTH_EPS of the [0, 1) range's ends.
There `acceptable[pixel]` holds every winner such a rasteriser could produce (EMPTY for none)."""
import numpy as np

F = np.float32
EMPTY = 0xFFFFFFFF
EDGE_EPS = 2.0 ** -8
DEPTH_EPS = 1e-6
CLEAR = np.array([0.05, 0.05, 0.1, 1.0], F)
TRIANGLES = ((0, 1, 2), (2, 1, 3))  # corner k = (ox, oy) = (+-1, +-1) with ox = +1 for k & 1, oy = +1 for k & 2


def unorm8(v):
    """oracle.c's orc_unorm8 on f32 values."""
    v = np.asarray(v, F)
    v = np.where(v > 0, v, F(0))
    v = np.minimum(v, F(1))
    return (v * F(255) + F(0.5)).astype(np.uint8)


def clear8():
    return unorm8(CLEAR)


def point_setup(vp, positions, gradients, scales):
    """Per point the four clip-space corners (n, 4, 4: x, y, z, w; f32), the lit colour (n, 4; f32) and the normal."""
    m = np.asarray(vp, F).reshape(-1)[:16]
    p = np.asarray(positions, F).reshape(-1, 4)[:, :3]
    g = np.asarray(gradients, F).reshape(-1, 4)
    s = F(0.025) * np.asarray(scales, F).reshape(-1)
    with np.errstate(all="ignore"):
        gx, gy, gz = g[:, 1], g[:, 2], g[:, 3]
        ig = F(1) / np.sqrt((gx * gx + gy * gy) + gz * gz)
        nx, ny, nz = gx * ig, gy * ig, gz * ig
        steep = np.abs(ny) > F(0.9)
        ux, uy, uz = np.where(steep, F(1), F(0)), np.where(steep, F(0), F(1)), F(0)
        tx, ty, tz = uy * nz - uz * ny, uz * nx - ux * nz, ux * ny - uy * nx
        itl = F(1) / np.sqrt((tx * tx + ty * ty) + tz * tz)
        tx, ty, tz = tx * itl, ty * itl, tz * itl
        bx, by, bz = ny * tz - nz * ty, nz * tx - nx * tz, nx * ty - ny * tx
        clip = np.zeros((p.shape[0], 4, 4), F)
        for k in range(4):
            ox, oy = F(1 if k & 1 else -1), F(1 if k & 2 else -1)
            wx = p[:, 0] + ((tx * ox) * s + (bx * oy) * s)
            wy = p[:, 1] + ((ty * ox) * s + (by * oy) * s)
            wz = p[:, 2] + ((tz * ox) * s + (bz * oy) * s)
            for r in range(4):
                clip[:, k, r] = ((m[r] * wx + m[4 + r] * wy) + m[8 + r] * wz) + m[12 + r]
        l = F(1) / np.sqrt(F(3))
        kd = F(0.3) + F(0.7) * np.maximum((nx * l + ny * l) + nz * l, F(0))
        color = np.stack([(nx * F(0.5) + F(0.5)) * kd, (ny * F(0.5) + F(0.5)) * kd, (nz * F(0.5) + F(0.5)) * kd, np.ones_like(kd)], 1)
    return clip, color.astype(F), np.stack([nx, ny, nz], 1)


def screen_corners(clip, width, height):
    """f64 screen x, y and depth z/w of every corner, and which points are drawn at all."""
    c = clip.astype(np.float64)
    with np.errstate(all="ignore"):
        ok = np.all(np.isfinite(clip.reshape(clip.shape[0], -1)), axis=1) & np.all(clip[:, :, 3] > 0, axis=1)
        X = (c[:, :, 0] / c[:, :, 3] + 1.0) * 0.5 * width
        Y = (1.0 - c[:, :, 1] / c[:, :, 3]) * 0.5 * height
        Z = c[:, :, 2] / c[:, :, 3]
    return X, Y, Z, ok


def _seg_dist(px, py, ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    ll = dx * dx + dy * dy
    with np.errstate(all="ignore"):
        t = np.where(ll > 0, ((px - ax) * dx + (py - ay) * dy) / np.where(ll > 0, ll, 1.0), 0.0)
    t = np.clip(t, 0.0, 1.0)
    return np.hypot(px - (ax + t * dx), py - (ay + t * dy))


def _fragments(X, Y, Z, ok, width, height, chunk=16384):
    """Every (pixel, point) pair that covers the pixel or passes within EDGE_EPS of one of the point's triangles: flat pixel,
    point index, depth (the triangle's plane, extrapolated for a near miss), covered (the exact rule), near-edge."""
    out = []
    idx_all = np.nonzero(ok)[0]
    for a, b, c in TRIANGLES:
        for lo in range(0, idx_all.shape[0], chunk):
            idx = idx_all[lo:lo + chunk]
            ax, ay, az = X[idx, a], Y[idx, a], Z[idx, a]
            bx, by, bz = X[idx, b], Y[idx, b], Z[idx, b]
            cx, cy, cz = X[idx, c], Y[idx, c], Z[idx, c]
            area = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
            swap = area < 0  # raster_tri: a negative area swaps the last two vertices
            bx, cx = np.where(swap, cx, bx), np.where(swap, bx, cx)
            by, cy = np.where(swap, cy, by), np.where(swap, by, cy)
            bz, cz = np.where(swap, cz, bz), np.where(swap, bz, cz)
            area = np.abs(area)
            x0 = np.minimum(np.minimum(ax, bx), cx) - EDGE_EPS
            x1 = np.maximum(np.maximum(ax, bx), cx) + EDGE_EPS
            y0 = np.minimum(np.minimum(ay, by), cy) - EDGE_EPS
            y1 = np.maximum(np.maximum(ay, by), cy) + EDGE_EPS
            # pixels whose centre k + 0.5 lies in [x0, x1], clipped to the screen
            i0 = np.clip(np.ceil(x0 - 0.5), 0, width).astype(np.int64)
            i1 = np.clip(np.floor(x1 - 0.5) + 1, 0, width).astype(np.int64)
            j0 = np.clip(np.ceil(y0 - 0.5), 0, height).astype(np.int64)
            j1 = np.clip(np.floor(y1 - 0.5) + 1, 0, height).astype(np.int64)
            nxs, nys = np.maximum(i1 - i0, 0), np.maximum(j1 - j0, 0)
            cnt = nxs * nys
            total = int(cnt.sum())
            if total == 0:
                continue
            own = np.repeat(np.arange(idx.shape[0]), cnt)
            local = np.arange(total) - np.repeat(np.cumsum(cnt) - cnt, cnt)
            px = (i0[own] + local % nxs[own]).astype(np.float64) + 0.5
            py = (j0[own] + local // nxs[own]).astype(np.float64) + 0.5
            pax, pay, pbx, pby, pcx, pcy = ax[own], ay[own], bx[own], by[own], cx[own], cy[own]
            w0 = (pcx - pbx) * (py - pby) - (pcy - pby) * (px - pbx)
            w1 = (pax - pcx) * (py - pcy) - (pay - pcy) * (px - pcx)
            w2 = (pbx - pax) * (py - pay) - (pby - pay) * (px - pax)

            def top_left(sx, sy, ex, ey):
                dx, dy = ex - sx, ey - sy
                return (dy < 0) | ((dy == 0) & (dx > 0))

            tl0, tl1, tl2 = top_left(pbx, pby, pcx, pcy), top_left(pcx, pcy, pax, pay), top_left(pax, pay, pbx, pby)
            pa = area[own]
            covered = (pa != 0) & (w0 >= 0) & (w1 >= 0) & (w2 >= 0) & ~((w0 == 0) & ~tl0) & ~((w1 == 0) & ~tl1) & ~((w2 == 0) & ~tl2)
            with np.errstate(all="ignore"):  # z/w is affine in screen space: the plane through the three vertices
                x1, y1, z1 = pbx - pax, pby - pay, bz[own] - az[own]
                x2, y2, z2 = pcx - pax, pcy - pay, cz[own] - az[own]
                depth = az[own] + ((z1 * y2 - z2 * y1) / pa) * (px - pax) + ((z2 * x1 - z1 * x2) / pa) * (py - pay)
            near = np.minimum(np.minimum(_seg_dist(px, py, pax, pay, pbx, pby), _seg_dist(px, py, pbx, pby, pcx, pcy)),
                              _seg_dist(px, py, pcx, pcy, pax, pay)) < EDGE_EPS
            keep = covered | near
            pix = (py[keep] - 0.5).astype(np.int64) * width + (px[keep] - 0.5).astype(np.int64)
            out.append((pix, idx[own][keep], depth[keep], covered[keep], near[keep]))
    if not out:
        e = np.zeros(0, np.int64)
        return e, e, np.zeros(0), np.zeros(0, bool), np.zeros(0, bool)
    return tuple(np.concatenate([o[k] for o in out]) for k in range(5))


class PointFrame:
    """The reference frame of one render() call: ids (H, W) u32, depth (H, W) f64 (1.0 where empty), rgba8 (H, W, 4),
    rgba32f (H, W, 4), colors (n, 4) f32 per point, contested (H, W) bool, acceptable {flat pixel: set of ids}."""

    def colour_of(self, ids):
        ids = np.asarray(ids, np.int64)
        c = np.where((ids == EMPTY)[..., None], CLEAR, self.colors[np.where(ids == EMPTY, 0, ids)] if self.colors.shape[0] else CLEAR)
        return c.astype(F)


def render(vp, positions, gradients, scales, width, height):
    """The reference image, depth, ids and the contested pixels (see the module docstring)."""
    clip, color, _ = point_setup(vp, positions, gradients, scales)
    X, Y, Z, ok = screen_corners(clip, width, height)
    pix, idx, depth, covered, near = _fragments(X, Y, Z, ok, width, height)
    npx = width * height
    fr = PointFrame()
    fr.colors = color
    # the exact reference: nearest covering fragment in [0, 1), lower index on equal depth
    live = covered & (depth >= 0) & (depth < 1)
    order = np.lexsort((idx[live], depth[live], pix[live]))
    lp, li, ld = pix[live][order], idx[live][order], depth[live][order]
    first = np.ones(lp.shape[0], bool)
    first[1:] = lp[1:] != lp[:-1]
    ids = np.full(npx, EMPTY, np.int64)
    dep = np.ones(npx)
    ids[lp[first]] = li[first]
    dep[lp[first]] = ld[first]
    # what another correct rasteriser may make of it
    edge_range = (np.abs(depth) < DEPTH_EPS) | (np.abs(depth - 1.0) < DEPTH_EPS)
    certain = covered & ~near & ~edge_range & (depth >= 0) & (depth < 1)
    dstar = np.full(npx, np.inf)
    np.minimum.at(dstar, pix[certain], depth[certain])
    cand = (certain | near | (covered & edge_range)) & (depth >= -DEPTH_EPS) & (depth < 1.0 + DEPTH_EPS) & (depth < dstar[pix] + DEPTH_EPS)
    acceptable = {}
    for p, i in zip(pix[cand].tolist(), idx[cand].tolist()):
        acceptable.setdefault(p, set()).add(i)
    for p, s in acceptable.items():
        if not np.isfinite(dstar[p]):
            s.add(EMPTY)
        s.add(int(ids[p]))
    contested = np.zeros(npx, bool)
    for p, s in list(acceptable.items()):
        if s == {int(ids[p])}:
            del acceptable[p]
        else:
            contested[p] = True
    fr.ids = ids.astype(np.uint32).reshape(height, width)
    fr.depth = dep.reshape(height, width)
    fr.contested = contested.reshape(height, width)
    fr.acceptable = acceptable
    fr.rgba32f = fr.colour_of(fr.ids.astype(np.int64))
    fr.rgba8 = unorm8(fr.rgba32f)
    fr.width, fr.height = width, height
    return fr


def compare(fr, ids, depth, rgba8, rgba32f=None):
    """Holds a renderer's outputs to the reference frame: off the contested pixels ids equal, depth within DEPTH_EPS, rgba8
    within 1 LSB; on them the id is an acceptable winner and the colour is that winner's.  Returns the contested fraction."""
    ids = np.asarray(ids, np.uint32).reshape(fr.height, fr.width)
    depth = np.asarray(depth, np.float32).reshape(fr.height, fr.width)
    rgba8 = np.asarray(rgba8, np.uint8).reshape(fr.height, fr.width, 4)
    free = ~fr.contested
    bad = np.argwhere(free & (ids != fr.ids))
    assert bad.shape[0] == 0, f"{bad.shape[0]} uncontested pixels with another winner, first at (y, x) {bad[0].tolist()}: " \
                              f"got {ids[tuple(bad[0])]}, want {fr.ids[tuple(bad[0])]}"
    dd = np.abs(depth.astype(np.float64) - fr.depth)
    assert dd[free].max(initial=0.0) <= DEPTH_EPS, f"depth off by {dd[free].max()}"
    d8 = np.abs(rgba8.astype(int) - fr.rgba8.astype(int)).max(axis=2)
    assert d8[free].max(initial=0) <= 1, f"rgba8 off by {d8[free].max()}"
    for p, s in fr.acceptable.items():
        y, x = divmod(p, fr.width)
        got = int(ids[y, x])
        assert got in s, f"pixel (y, x) ({y}, {x}): winner {got} is not one of {sorted(s)}"
    # every pixel's colour is its own winner's (on contested pixels too)
    want8 = unorm8(fr.colour_of(ids.astype(np.int64)))
    assert np.abs(rgba8.astype(int) - want8.astype(int)).max(initial=0) <= 1, "a pixel's colour is not its winner's"
    if rgba32f is not None:
        got32 = np.asarray(rgba32f, F).reshape(fr.height, fr.width, 4)
        assert np.array_equal(got32, fr.colour_of(ids.astype(np.int64))), "rgba32f is not the winner's colour"
    # the depth of a pixel nobody won is the cleared 1.0
    assert np.all(depth[ids == EMPTY] == 1.0)
    return float(fr.contested.mean())
