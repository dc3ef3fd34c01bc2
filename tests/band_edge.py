"""Adversarial band-edge scenes for the band projector's reach cull (project.hip: cannot_reach_band).

A band frame renders tile rows [row0, row1).  A splat belongs to the band iff the binner's tile range (tile_range.h)
meets those rows: its record's max_y >= row0 * T and its min_y < row1 * T.  The scenes built here put the ORACLE's exact
record edge on those two boundaries — on the boundary itself, one f32 ulp either side, and at +-0.5, +-1.5 and +-3 px —
by bisecting in float32, through the oracle, either the radius (fixed centre) or the centre's position along the camera's
up vector (fixed radius).  They also hold what a hand-derived bound tends to get wrong: centres far off-screen with a radius
that still reaches the band, splats near the eye, and (discs) |n| != 1, n.y at the 0.9 tangent switch, near edge-on discs.

Used by tests/test_band_reach_cpu.py (the bound restated in NumPy) and tests/test_gpu_band_reach.py (the kernels).
Nothing here is part of the product or of the oracle.
"""
import math

import numpy as np

from oracle import oracle as O

# (name, camera) — O.camera keywords; aspect is the screen's.  Axis-aligned views are where the bound is tight (max_i |VP[i][x]|
# is attained by the exact offset); the others are oblique, with elevations up to +-1.2 and fov from 10 to 120 degrees.
CAMERAS = {
    "axis": dict(azimuth=0.0, elevation=0.0, fov=45.0),
    "axis_side": dict(azimuth=math.pi / 2, elevation=0.0, fov=45.0),
    "oblique": dict(azimuth=0.5, elevation=0.5, fov=45.0),
    "high": dict(azimuth=2.1, elevation=1.2, fov=60.0),
    "low": dict(azimuth=-0.7, elevation=-1.2, fov=30.0),
    "narrow": dict(azimuth=0.0, elevation=0.0, fov=10.0, distance=12.0),
    "wide": dict(azimuth=0.3, elevation=-0.4, fov=120.0),
}

# target offsets of the oracle's edge from the band boundary, in pixels (one f32 ulp either side is added per boundary)
OFFSETS_PX = (0.0, 0.5, -0.5, 1.5, -1.5, 3.0, -3.0)


def screen_for(aspect, h=240):
    return max(1, int(round(h * aspect))), h


def make_camera(name, w, h, **over):
    cam = dict(CAMERAS[name])
    cam.update(over)
    cam["aspect"] = w / h
    vp, eye = O.camera(**cam)
    return O.uniforms(vp, eye, w, h)


def _vp(u):
    return np.asarray(u[:16], np.float64).reshape(4, 4).T  # row-major M: clip = M @ (p, 1)


def unproject(u, sx, sy, cw):
    """World positions (f64) whose clip w is cw and whose screen centre is (sx, sy) — exactly in f64."""
    M = _vp(u)
    w, h = float(u[20]), float(u[21])
    sx, sy, cw = np.broadcast_arrays(np.asarray(sx, np.float64), np.asarray(sy, np.float64), np.asarray(cw, np.float64))
    ndx, ndy = sx / w * 2.0 - 1.0, 1.0 - sy / h * 2.0
    A = M[[0, 1, 3], :3]
    rhs = np.stack([ndx * cw, ndy * cw, cw], axis=-1) - M[[0, 1, 3], 3]
    return np.linalg.solve(A, rhs.reshape(-1, 3).T).T.reshape(sx.shape + (3,))


def camera_up(u, axis=1):
    """World direction that moves a point straight up the screen (decreasing screen y) at fixed clip w; axis=0: right."""
    M = _vp(u)
    A = M[[0, 1, 3], :3]
    d = np.linalg.solve(A, np.eye(3)[axis])
    return d / np.linalg.norm(d)


def records(u, props, normals, footprint):
    """The oracle's (n, 8) ProjectedSplat records — for discs, the disc's exact bounds (O.disc_bounds via O.project_disc)."""
    if footprint == "disc":
        return O.project_disc(u, props, normals)[0]
    return O.project(u, props)


def in_band(rec, w, h, tile, row0, row1):
    """Whether the oracle's tile range of each record meets tile rows [row0, row1) — the comparisons of tile_range (f64, as
    TileBinner.ts), evaluated vectorised; tests/test_band_reach_cpu.py checks it against O.bin_sorted."""
    b = rec[:, :4].astype(np.float64)
    ok = ~np.isnan(b).any(axis=1)
    with np.errstate(invalid="ignore"):
        min_x, min_y = np.maximum(b[:, 0], 0.0), np.maximum(b[:, 1], 0.0)
        max_x, max_y = np.minimum(b[:, 2], w), np.minimum(b[:, 3], h)
        ok &= (min_x < max_x) & (min_y < max_y)
        ntx, nty = -(-w // tile), -(-h // tile)
        a, bb = np.floor(min_x / tile), np.minimum(np.floor(max_x / tile), ntx - 1)
        c, d = np.floor(min_y / tile), np.minimum(np.floor(max_y / tile), nty - 1)
        ok &= (a <= bb) & (c <= d)
        ok &= (np.maximum(c, row0) <= np.minimum(d, row1 - 1)) & (row1 > 0)
    return ok


def _bisect(f, lo, hi, target, rising):
    """Float32 bisection, vectorised: lo/hi bracket the crossing (f(lo) < target <= f(hi) when rising, else the reverse).
    Returns the final adjacent-float brackets (lo, hi)."""
    lo, hi = lo.astype(np.float32).copy(), hi.astype(np.float32).copy()
    for _ in range(200):
        mid = (lo.astype(np.float64) + hi.astype(np.float64)) * 0.5
        mid = mid.astype(np.float32)
        live = (mid != lo) & (mid != hi)
        if not live.any():
            break
        v = f(mid)
        below = (v < target) if rising else ~(v < target)  # (NaN counts as "at or past the target" when rising)
        lo = np.where(live & below, mid, lo)
        hi = np.where(live & ~below, mid, hi)
    return lo, hi


def _targets(edge):
    t = [np.float32(edge) + np.float32(d) for d in OFFSETS_PX]
    e = np.float32(edge)
    t += [np.nextafter(e, np.float32(np.inf)), np.nextafter(e, np.float32(-np.inf))]
    return np.array(t, np.float32)


class Scene:
    """props (n, 8) f32, normals (n, 4) f32, and per splat: the boundary it was aimed at ('row0' / 'row1' / '') and the kind."""

    def __init__(self):
        self.props, self.normals, self.aim, self.kind = [], [], [], []

    def add(self, pos, radius, normals, aim, kind, rng):
        n = pos.shape[0]
        p = np.zeros((n, 8), np.float32)
        p[:, :3] = pos
        p[:, 3] = radius
        p[:, 4:7] = rng.uniform(0.2, 1.0, (n, 3))
        p[:, 7] = 1.0
        self.props.append(p)
        self.normals.append(np.asarray(normals, np.float32).reshape(n, 4))
        self.aim += [aim] * n
        self.kind += [kind] * n

    def arrays(self):
        return (np.concatenate(self.props), np.concatenate(self.normals), np.array(self.aim), np.array(self.kind))


def _disc_normals(rng, n):
    """Unit and non-unit normals, n.y at the 0.9 tangent switch, and near edge-on orientations (normal ~ perpendicular to
    the view ray is arranged by the caller's camera; here: a spread over all directions and lengths)."""
    v = rng.standard_normal((n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    k = np.arange(n) % 6
    ny = np.float32(0.9)
    v[k == 1] = [0.3, 0.9, 0.3]                                               # n.y = 0.9f: not steep; one ulp above is
    v[k == 2] = [np.sqrt(1 - 0.9 ** 2) / np.sqrt(2), float(np.nextafter(ny, np.float32(1))), np.sqrt(1 - 0.9 ** 2) / np.sqrt(2)]
    v[k == 3] = [0.0, float(np.nextafter(ny, np.float32(0))), np.sqrt(1 - 0.9 ** 2)]
    scale = np.array([1.0, 0.2, 3.0])[np.arange(n) % 3]
    scale[(k >= 1) & (k <= 3)] = 1.0                                          # (keep n.y at the switch)
    out = np.zeros((n, 4), np.float32)
    out[:, :3] = v * scale[:, None]
    out[:, 3] = 1.0
    return out


def _edge_on(u, pos, rng):
    """Normals perpendicular (up to a small tilt) to the view ray of each position: near edge-on discs."""
    eye = np.asarray(u[16:19], np.float64)
    ray = pos - eye
    ray /= np.linalg.norm(ray, axis=1, keepdims=True)
    a = rng.standard_normal(pos.shape)
    a -= (a * ray).sum(axis=1, keepdims=True) * ray
    a /= np.linalg.norm(a, axis=1, keepdims=True)
    tilt = rng.choice([0.0, 1e-4, 1e-2], size=(pos.shape[0], 1))
    n = a + tilt * ray
    out = np.zeros((pos.shape[0], 4), np.float32)
    out[:, :3] = n * rng.choice([0.2, 1.0, 3.0], size=(pos.shape[0], 1))
    out[:, 3] = 1.0
    return out


def band_edge_scene(u, tile, row0, row1, footprint="isotropic", seed=0, per=4):
    """Splats whose oracle record edge lands on the band's boundaries, for one camera (uniforms u, screen in u[20:22]).
    per: splats per (boundary, target, placement).  Returns (props, normals, aim, kind)."""
    rng = np.random.default_rng(seed)
    w, h = int(u[20]), int(u[21])
    disc = footprint == "disc"
    up = camera_up(u)
    eye = np.asarray(u[16:19], np.float64)
    M = _vp(u)
    cw_eye = float(np.abs(M[3, :3]).max())  # clip w per unit distance along the view ray, roughly
    sc = Scene()

    def ymin_max(props, normals):
        r = records(u, props, normals, footprint)
        return r[:, 1], r[:, 3]

    def aim_at(pos, radius, normals, boundary, target, vary, kind):
        """Bisects radius (vary='radius') or the position along `up` (vary='up') so that the oracle's max_y (row0) or min_y
        (row1) crosses target; keeps both bracketing splats of every bracketed aim."""
        col = 3 if boundary == "row0" else 1
        radius = np.broadcast_to(np.asarray(radius, np.float32), pos.shape[:1])

        def splats(x, pos, radius):
            p = np.zeros((pos.shape[0], 8), np.float32)
            if vary == "radius":
                p[:, :3], p[:, 3] = pos, x
            else:
                p[:, :3], p[:, 3] = (pos + x[:, None].astype(np.float64) * up).astype(np.float32), radius
            return p

        if vary == "radius":  # (radius: the largest radius to try)
            lo, hi = np.zeros_like(radius), radius
        else:
            span = np.float32(4.0) * radius + np.float32(0.5)
            lo, hi = -span, span
        # max_y grows with the radius, min_y falls with it; both fall as the centre moves up
        rising = vary == "radius" and boundary == "row0"
        flo, fhi = (records(u, splats(x, pos, radius), normals, footprint)[:, col] for x in (lo, hi))
        ok = (flo < target) & (fhi >= target) if rising else (flo >= target) & (fhi < target)
        if not ok.any():
            return
        pos, normals, radius = pos[ok], normals[ok], radius[ok]
        lo, hi = _bisect(lambda x: records(u, splats(x, pos, radius), normals, footprint)[:, col], lo[ok], hi[ok], target, rising)
        for x in (lo, hi):
            p = splats(x, pos, radius)
            sc.add(p[:, :3], p[:, 3], normals, boundary, kind, rng)

    right = camera_up(u, 0)

    def normals_for(pos, sideways=False):
        if not disc:
            return np.tile(np.float32([0.0, 0.0, 1.0, 1.0]), (pos.shape[0], 1))
        nr = _disc_normals(rng, pos.shape[0])
        third = np.arange(pos.shape[0]) % 4 == 0
        nr[third] = _edge_on(u, pos[third].astype(np.float64), rng)
        if sideways:  # half of them in the plane of the view ray and the screen's up: the disc reaches furthest up and down
            half = np.arange(pos.shape[0]) % 2 == 1
            nr[half, :3] = right * rng.choice([0.2, 1.0, 3.0], size=(int(half.sum()), 1))
        return nr

    for boundary, edge in (("row0", row0 * tile), ("row1", row1 * tile)):
        if boundary == "row0" and row0 == 0 or boundary == "row1" and row1 * tile >= h:
            continue  # (the screen's own edge: nothing to cull there)
        side = -1.0 if boundary == "row0" else 1.0  # centres above row0 / below row1: outside the band
        for target in _targets(edge):
            m = per
            sx = rng.uniform(0.0, w, m)
            depth = rng.uniform(1.0, 6.0, m) * cw_eye * 3.0
            # 1. fixed centre a few pixels to a screen height outside, radius bisected
            dy = side * np.exp(rng.uniform(np.log(0.5), np.log(h), m))
            pos = unproject(u, sx, edge + dy, depth)
            rmax = (0.999 * depth / cw_eye).astype(np.float32)  # (every axis offset in front of the eye)
            aim_at(pos, rmax, normals_for(pos, True), boundary, target, "radius", "beside")
            # 2. centres several screen heights off-screen, radius bisected
            #    (a disc's quad must stay in front of the eye, and the disc's reach from its radius is less: one to three)
            mo = 4 * m if disc else m
            far = rng.uniform(0.3, 1.5, mo) if disc else rng.uniform(2.0, 6.0, mo)
            sy = -far * h if boundary == "row0" else h + far * h
            pos = unproject(u, rng.uniform(0.0, w, mo), sy, np.resize(depth, mo))
            rmax = np.resize(rmax, mo)
            aim_at(pos, rmax * np.float32(0.5 if disc else 1.0), normals_for(pos, True), boundary, target, "radius", "off-screen")
            # 3. fixed small radius (max_r from a fraction of a pixel to a few), centre moved along up: the bound's own slack
            #    is least here, since its 0.1 % of the reach is nothing and its +1 px is all
            pos = unproject(u, sx, edge + side * 2.0, depth)
            px_world = depth * 2.0 / (h * np.abs(M[1, :3]).max())  # one screen pixel in world units at that depth, roughly
            rad = (px_world * np.exp(rng.uniform(np.log(0.2), np.log(8.0), m))).astype(np.float32)
            aim_at(pos, rad, normals_for(pos), boundary, target, "up", "small")
            # 4. near the eye: clip w comparable to the radius (c_w - max|a_w| small or <= 0)
            cwn = rng.uniform(0.11, 0.6, m)
            pos = unproject(u, sx, edge + side * rng.uniform(1.0, 40.0, m), cwn)
            aim_at(pos, (cwn * rng.uniform(0.2, 1.5, m) / cw_eye).astype(np.float32), normals_for(pos), boundary, target, "radius", "near-eye")
    # a few degenerate splats: NaN position or radius, zero radius, zero normal, behind the eye
    k = 8
    pos = unproject(u, rng.uniform(0, w, k), rng.uniform(0, h, k), 3.0 * cw_eye)
    rad = np.float32([np.nan, 0.0, -0.0, 0.05, 0.05, np.inf, 0.05, 0.05])
    pos[3] = np.nan
    pos[7] = eye - 2.0 * (pos[7] - eye)  # behind the eye
    nr = normals_for(pos)
    nr[4, :3] = 0.0
    nr[6, :3] = np.nan
    sc.add(pos, rad, nr, "", "degenerate", rng)
    return sc.arrays()
