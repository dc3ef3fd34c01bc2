"""Reference for include/splat.h, "TSDF fusion and mesh extraction": a float64 NumPy restatement of the integration rule, and plain
Python / NumPy marching tetrahedra on the Kuhn split whose case handling is GENERATED from the contract's geometric rules
(tet_case below builds each case from the tetrahedron's vertices: which edges cross, which of them are neighbours on the quad,
and which way round they run counter-clockwise seen from outside; there is no typed-in table).  Also the inputs the CPU and GPU
tests share, and the binary32 error bounds the GPU tests hold the kernels to.

Bounds, all in units of eps = 2^-24 and to first order (the tests multiply them by a measured constant):

Integration, per node and view.  X_c = fma(voxel, i_c, origin_c) carries one rounding, eps |X_c|.  A row of clip = VP (X, 1) is a
chain of three fma: four roundings in all with the one in X, each at most eps times the sum of the absolute values of the row's
terms, A_r = sum_c |VP[r][c]| |X_c| + |VP[r][3]|; a fifth covers the second-order terms:
    |d clip_r| <= 5 A_r.
ndc = clip.x / clip.w:  |d ndc| <= (5 A_x + 5 A_w |ndc|) / |clip.w| + |ndc| (the divide's own rounding).
u = (ndc 0.5 + 0.5) W, two more roundings:   B_u = (W / 2) |d ndc| + 2 (|u| + W / 2);   B_v likewise with H.
r = |X - eye|: each difference carries X_c's rounding and its own, eps (|X_c| + |X_c - eye_c|); through the root (derivatives of
size at most 1) and with the roundings of the squares, the sums and the root (2.5 eps r):   B_r = |X|_1 + 5 r.   r = clip.w:
B_r = 5 A_w.   s = D - r, D exact:   B_s = B_r + |s|.
A node is DECISION-NEAR in a view, and left out of every comparison from that view on, when a rounding could change which way a
test of the rule goes: |clip.w| <= NEAR_K eps 5 A_w;  in front of the eye and within a pixel of the screen,
|u - round(u)| <= NEAR_K eps B_u or the same for v (the screen's borders 0, W, H are integers too);  or, having reached step 7,
|s + trunc| <= NEAR_K eps B_s.  NEAR_K = 4 is a safety factor over the first-order bounds.  (f = min(1, s / trunc) is
continuous at s = trunc, and the tests on D and a read exact inputs: neither is a decision a rounding can change.)
Every other node:  f = min(1, s / trunc):  B_f = B_s / trunc + |f|.  The weight after m additions has the relative bound m (one
rounding each; the clamp by max_weight is exact), so B_weight = m |weight|.  The running mean (tsdf w + f a) / w' inherits the
weighted mean of the bounds of its inputs, three roundings of its own (the product, the fma, the divide), each at most eps times
max(|tsdf|, |f|), and 2 (m + 1) times that from the relative errors of w and w':
    B_tsdf' = (B_tsdf w + B_f a) / w' + (5 + 2 m) max(|tsdf|, |f|),
and the colour likewise with B_f = 0 (the pixel is exact) and max(|color_c|, |image_c|) per channel.

Vertices.  t = f0 / (f0 - f1) from exact inputs of opposite sign (or zero): no cancellation, two roundings, |dt| <= 2 |t| <= 2.
p = fma(voxel, index, origin): eps |p| each end; their difference eps (|p0| + |p1| + |p1 - p0|); the final fma one more:
    B_position_c = 2 |p0_c| + 2 |p1_c| + 3 |p1_c - p0_c|,     B_colour_c = 2 |c0_c| + 2 |c1_c| + 3 |c1_c - c0_c|.
"""
import functools
import itertools
import math
import types

import numpy as np

EPS = 2.0 ** -24
NEAR_K = 4.0
DISTANCE, Z = "distance", "z"
KINDS = {DISTANCE: 0, Z: 1}
PERMS = tuple(itertools.permutations(range(3)))  # lexicographic: the tetrahedra's numbers
EDGE_DIRS = ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1))
INTEGRATE_BRICK = (32, 4, 4)  # csrc/tsdf.hip, k_tsdf_integrate's brick: the tests add grids one node beyond it


# ---- cameras ----------------------------------------------------------------------------------------------------------------------
def pinhole(width, height, eye, target, focal, mirrored=False, roll=0.2):
    """A 22-float pinhole block (float32; autograd.pinhole_uniforms' layout, in NumPy) with fx != fy and an off-centre principal
    point; mirrored: the x axis of the screen flipped."""
    eye = np.asarray(eye, np.float64)
    f = np.asarray(target, np.float64) - eye
    f /= np.linalg.norm(f)
    r = np.cross(f, (0.0, 1.0, 0.0))
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    c, s = math.cos(roll), math.sin(roll)
    R = np.stack([c * r + s * d, -s * r + c * d, f])
    t = -R @ eye
    if mirrored:
        R[0], t[0] = -R[0], -t[0]
    W, H, fx, fy, cx, cy = float(width), float(height), focal, 1.1 * focal, 0.47 * width, 0.55 * height
    P = np.array([[2 * fx / W, 0, 2 * cx / W - 1, 0], [0, -2 * fy / H, 1 - 2 * cy / H, 0], [0, 0, 1000 / 999.99, -10 / 999.99], [0, 0, 1, 0]])
    V = np.eye(4)
    V[:3, :3], V[:3, 3] = R, t
    u = np.zeros(22, np.float32)
    u[:16] = (P @ V).T.reshape(16)
    u[16:19] = eye
    u[20], u[21] = W, H
    return u


# ---- integration ------------------------------------------------------------------------------------------------------------------
class Volume:
    """The float64 volume beside its bounds: tsdf, weight (N,), color (N, 3) or None; touched (ever written); near (decision-near
    in some view so far); B_tsdf, B_color in units of eps; additions (m)."""

    def __init__(self, origin, voxel, dims, trunc, color=False):
        self.origin, self.voxel, self.trunc = np.asarray(origin, np.float32), np.float32(voxel), np.float32(trunc)
        self.dims = tuple(int(d) for d in dims)
        n = self.n = self.dims[0] * self.dims[1] * self.dims[2]
        self.tsdf, self.weight = np.zeros(n), np.zeros(n)
        self.color = np.zeros((n, 3)) if color else None
        self.touched, self.near = np.zeros(n, bool), np.zeros(n, bool)
        self.B_tsdf, self.B_color, self.additions = np.zeros(n), np.zeros((n, 3)), np.zeros(n)

    def indices(self):
        nx, ny, nz = self.dims
        k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
        return np.stack([i.reshape(-1), j.reshape(-1), k.reshape(-1)], axis=1)  # row n = i + nx (j + ny k)

    def positions(self):
        return self.origin.astype(np.float64) + np.float64(self.voxel) * self.indices()


def integrate(vol, u, kind, depth, obs=None, image=None, max_weight=0.0):
    """One view into vol (float64, the contract's ten steps).  Returns (written, near): the nodes this view wrote, and the ones
    decision-near in it (already added to vol.near)."""
    u = np.asarray(u, np.float32).astype(np.float64)
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    VP, eye = u[:16].reshape(4, 4).T, u[16:19]
    X = vol.positions()
    Xh = np.concatenate([X, np.ones((vol.n, 1))], axis=1)
    clip, A = Xh @ VP.T, np.abs(Xh) @ np.abs(VP).T
    cw = clip[:, 3]
    front = cw > 0
    near = np.abs(cw) <= NEAR_K * EPS * 5 * A[:, 3]
    with np.errstate(all="ignore"):
        safe_w = np.where(front, cw, 1.0)
        ndc = clip[:, :2] / safe_w[:, None]
        d_ndc = (5 * A[:, :2] + 5 * A[:, 3:4] * np.abs(ndc)) / safe_w[:, None] + np.abs(ndc)
        pu, pv = (ndc[:, 0] * 0.5 + 0.5) * W, (0.5 - 0.5 * ndc[:, 1]) * H
        B_u, B_v = W / 2 * d_ndc[:, 0] + 2 * (np.abs(pu) + W / 2), H / 2 * d_ndc[:, 1] + 2 * (np.abs(pv) + H / 2)
    close = front & (pu > -1) & (pu < W + 1) & (pv > -1) & (pv < H + 1)
    near |= close & ((np.abs(pu - np.rint(pu)) <= NEAR_K * EPS * B_u) | (np.abs(pv - np.rint(pv)) <= NEAR_K * EPS * B_v))
    on = front & (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
    p = np.where(on, np.floor(pv).astype(np.int64) * W + np.floor(pu).astype(np.int64), 0)
    D = depth.reshape(-1)[p].astype(np.float64)
    ok = on & np.isfinite(D) & (D > 0)
    a = np.ones(vol.n)
    if obs is not None:
        a = np.asarray(obs, np.float32).reshape(-1)[p].astype(np.float64)
        ok &= a > 0
    if kind == DISTANCE:
        r = np.linalg.norm(X - eye, axis=1)
        B_r = np.abs(X).sum(axis=1) + 5 * r
    else:
        r, B_r = cw, 5 * A[:, 3]
    trunc = np.float64(vol.trunc)
    with np.errstate(invalid="ignore"):
        s = D - r
        B_s = B_r + np.abs(s)
        near |= ok & (np.abs(s + trunc) <= NEAR_K * EPS * B_s)
        hit = ok & (s >= -trunc)
    s, B_s, a = np.where(hit, s, 0.0), np.where(hit, B_s, 0.0), np.where(hit, a, 1.0)
    f = np.minimum(1.0, s / trunc)
    B_f = B_s / trunc + np.abs(f)
    w0 = vol.weight
    w1 = w0 + a
    own = 5 + 2 * vol.additions
    t0 = np.where(w0 > 0, vol.tsdf, 0.0)
    vol.B_tsdf = np.where(hit, (vol.B_tsdf * w0 + B_f * a) / w1 + own * np.maximum(np.abs(t0), np.abs(f)), vol.B_tsdf)
    vol.tsdf = np.where(hit, (t0 * w0 + f * a) / w1, vol.tsdf)
    if vol.color is not None and image is not None:
        px = np.asarray(image, np.float32)[..., :3].reshape(-1, 3)[p].astype(np.float64)
        c0 = np.where((w0 > 0)[:, None], vol.color, 0.0)
        vol.B_color = np.where(hit[:, None], vol.B_color * (w0 / w1)[:, None] + own[:, None] * np.maximum(np.abs(c0), np.abs(px)), vol.B_color)
        vol.color = np.where(hit[:, None], (c0 * w0[:, None] + px * a[:, None]) / w1[:, None], vol.color)
    vol.weight = np.where(hit, np.minimum(w1, max_weight) if max_weight > 0 else w1, w0)
    vol.additions = vol.additions + hit
    vol.touched |= hit
    vol.near |= near
    return hit, near


# ---- marching tetrahedra ----------------------------------------------------------------------------------------------------------
def tet_vertices(p):
    """The four vertices of tetrahedron p of the unit cube: v0 = 0, v1 = v0 + e_pi1, v2 = v1 + e_pi2, v3 = (1, 1, 1)."""
    v = [np.zeros(3, int)]
    for axis in PERMS[p][:2]:
        nxt = v[-1].copy()
        nxt[axis] += 1
        v.append(nxt)
    v.append(np.ones(3, int))
    return v


@functools.lru_cache(maxsize=None)
def tet_case(p, inside):
    """The polygon tetrahedron p cuts out for the inside flags `inside` (a 4-tuple of bools): a tuple of its corners as (lo, hi)
    pairs of tetrahedron vertex indices (the edge each lies on), in the cyclic order that runs counter-clockwise seen from
    outside; () when nothing crosses.  Built from the geometry: the corners are the edges whose ends differ; two corners are
    neighbours on the polygon when their edges share a tetrahedron vertex (they then lie in one face); the direction is fixed by
    the normal of the polygon drawn through the edges' midpoints against the direction from the inside vertices to the outside."""
    v = tet_vertices(p)
    edges = [(a, b) for a in range(4) for b in range(a + 1, 4) if inside[a] != inside[b]]
    if not edges:
        return ()
    assert len(edges) in (3, 4)
    cycle, rest = [edges[0]], edges[1:]
    while rest:
        nxt = [e for e in rest if set(e) & set(cycle[-1])]
        if len(cycle) + len(rest) == 4 and len(cycle) == 1:  # a quad: the first corner has two neighbours; the opposite one is not among them
            assert len(nxt) == 2
        cycle.append(nxt[0])
        rest.remove(nxt[0])
    assert set(cycle[-1]) & set(cycle[0])
    mid = [(v[a] + v[b]) / 2.0 for a, b in cycle]
    normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
    outward = np.mean([v[k] for k in range(4) if not inside[k]], axis=0) - np.mean([v[k] for k in range(4) if inside[k]], axis=0)
    side = float(normal @ outward)
    assert abs(side) > 1e-9
    if side < 0:
        cycle = [cycle[0]] + cycle[:0:-1]
    return tuple(cycle)


def _shift(a, d, fill=False):
    """a[k + dz, j + dy, i + dx] on a's own grid (d = (dx, dy, dz), entries in {-1, 0, 1}), `fill` outside it."""
    out = np.full(a.shape, fill, a.dtype)
    src = [slice(None)] * 3
    dst = [slice(None)] * 3
    for ax, step in zip((2, 1, 0), d):
        if step > 0:
            src[ax], dst[ax] = slice(step, None), slice(None, -step)
        elif step < 0:
            src[ax], dst[ax] = slice(None, step), slice(-step, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def marching_tetrahedra(tsdf, weight, dims, origin, voxel, min_weight=0.0, color=None):
    """The contract's mesh of a float32 volume (tsdf, weight (N,); color (N, 3) or None), positions and colours in float64.
    A namespace: vertices (V, 3), triangles (T, 3) int64, colors (V, 3) or None, B_position, B_color (units of eps), and for the
    tests vertex_node, vertex_edge, triangle_cube, triangle_tet, inside, valid, meshed (node-indexed, meshed by lower corner)."""
    nx, ny, nz = (int(d) for d in dims)
    n = nx * ny * nz
    f32 = np.asarray(tsdf, np.float32).reshape(n)
    w32 = np.asarray(weight, np.float32).reshape(n)
    with np.errstate(invalid="ignore"):
        valid = (w32 > np.float32(min_weight)).reshape(nz, ny, nx)
        inside = (f32 < 0).reshape(nz, ny, nx) & valid
    meshed = np.ones((nz, ny, nx), bool)
    for c in itertools.product((0, 1), repeat=3):
        meshed &= _shift(valid, c)  # (a corner outside the grid is `False`: the cubes of the last layer do not exist)
    active = np.zeros((nz, ny, nx, 7), bool)
    for e, d in enumerate(EDGE_DIRS):
        differ = inside != _shift(inside, d)
        exists = _shift(np.ones((nz, ny, nx), bool), d)
        any_meshed = np.zeros((nz, ny, nx), bool)
        for o in itertools.product((0, 1), repeat=3):
            if not any(a and b for a, b in zip(o, d)):
                any_meshed |= _shift(meshed, tuple(-x for x in o))
        active[..., e] = differ & exists & any_meshed
    flat = active.reshape(n * 7)
    ids = np.where(flat, np.cumsum(flat) - 1, -1).reshape(n, 7)
    vertex_node, vertex_edge = np.nonzero(active.reshape(n, 7))
    f64 = f32.astype(np.float64)
    o64, h64 = np.asarray(origin, np.float32).astype(np.float64), np.float64(np.float32(voxel))
    idx = np.stack([vertex_node % nx, (vertex_node // nx) % ny, vertex_node // (nx * ny)], axis=1)
    dirs = np.asarray(EDGE_DIRS)[vertex_edge].reshape(-1, 3)
    other = vertex_node + dirs[:, 0] + nx * (dirs[:, 1] + ny * dirs[:, 2])
    p0, p1 = o64 + h64 * idx, o64 + h64 * (idx + dirs)
    with np.errstate(all="ignore"):
        t = f64[vertex_node] / (f64[vertex_node] - f64[other])
    out = types.SimpleNamespace(vertices=p0 + t[:, None] * (p1 - p0), B_position=2 * np.abs(p0) + 2 * np.abs(p1) + 3 * np.abs(p1 - p0),
                                colors=None, B_color=None, vertex_node=vertex_node, vertex_edge=vertex_edge, t=t,
                                inside=inside.reshape(n), valid=valid.reshape(n), meshed=meshed.reshape(n))
    if color is not None:
        c64 = np.asarray(color, np.float32).reshape(n, 3).astype(np.float64)
        c0, c1 = c64[vertex_node], c64[other]
        out.colors, out.B_color = c0 + t[:, None] * (c1 - c0), 2 * np.abs(c0) + 2 * np.abs(c1) + 3 * np.abs(c1 - c0)
    tris, tri_cube, tri_tet = [], [], []
    mixed = meshed & (_corner_count(inside) % 8 != 0)
    for cube in np.nonzero(mixed.reshape(n))[0]:
        ci, cj, ck = cube % nx, (cube // nx) % ny, cube // (nx * ny)
        for p in range(6):
            v = tet_vertices(p)
            node = [int(ci + q[0] + nx * (cj + q[1] + ny * (ck + q[2]))) for q in v]
            cycle = tet_case(p, tuple(bool(out.inside[m]) for m in node))
            if not cycle:
                continue
            q = [int(ids[node[lo], EDGE_DIRS.index(tuple(v[hi] - v[lo]))]) for lo, hi in cycle]
            assert min(q) >= 0
            m = q.index(min(q))
            q = q[m:] + q[:m]
            for tri in ([q] if len(q) == 3 else [q[:3], [q[0], q[2], q[3]]]):
                tris.append(tri)
                tri_cube.append(cube)
                tri_tet.append(p)
    out.triangles = np.asarray(tris, np.int64).reshape(-1, 3)
    out.triangle_cube, out.triangle_tet = np.asarray(tri_cube, np.int64), np.asarray(tri_tet, np.int64)
    return out


def _corner_count(inside):
    total = np.zeros(inside.shape, int)
    for c in itertools.product((0, 1), repeat=3):
        total += _shift(inside, c)
    return total


# ---- inputs the tests share -------------------------------------------------------------------------------------------------------
def node_grid(dims, origin, voxel):
    """(N, 3) float64 node positions of a grid (from the float32 origin and voxel, as the kernels see them)."""
    return Volume(origin, voxel, dims, 1.0).positions()


def sphere_volume(dims=(24, 24, 24), radius=0.71, voxel=0.083, centre_offset=(0.013, -0.021, 0.017)):
    """(tsdf float32 (N,), origin float32 (3,), voxel, centre float64 (3,)): |X - centre| - radius over 4 voxels, unclamped."""
    origin = (-0.5 * voxel * (np.asarray(dims) - 1) + np.asarray(centre_offset)).astype(np.float32)
    centre = np.asarray(centre_offset, np.float64) * 2.0
    X = node_grid(dims, origin, voxel)
    return ((np.linalg.norm(X - centre, axis=1) - radius) / (4 * voxel)).astype(np.float32), origin, voxel, centre


def torus_volume(dims=(32, 32, 16), major=0.8, minor=0.31, voxel=0.083, centre_offset=(0.011, 0.023, -0.017)):
    """The same for a torus around the z axis through `centre`."""
    origin = (-0.5 * voxel * (np.asarray(dims) - 1) + np.asarray(centre_offset)).astype(np.float32)
    centre = np.asarray(centre_offset, np.float64) * 2.0
    X = node_grid(dims, origin, voxel) - centre
    ring = np.hypot(X[:, 0], X[:, 1]) - major
    return ((np.hypot(ring, X[:, 2]) - minor) / (4 * voxel)).astype(np.float32), origin, voxel, centre


def holed_weights(dims, mixed=False, seed=3):
    """Weights 1 (mixed: 1 or 2, at random) with a block of zeros cut into the grid: (weight float32 (N,), block mask (N,))."""
    nx, ny, nz = dims
    w = np.ones((nz, ny, nx), np.float32)
    if mixed:
        w += (np.random.default_rng(seed).random((nz, ny, nx)) < 0.5).astype(np.float32)
    block = np.zeros((nz, ny, nx), bool)
    block[nz // 2 - 2:nz // 2 + 2, ny // 2 - 3:ny // 2 + 3, nx - 9:nx - 2] = True
    w[block] = 0.0
    return w.reshape(-1), block.reshape(-1)


def pattern_volume(seed=5):
    """All 256 inside patterns of one cube in one grid: cube q at lower corner (3 (q % 16), 3 (q // 16), 0) of a (47, 47, 2) grid,
    bit c of q the inside flag of corner c, random magnitudes; every node between the cubes has weight 0.
    (tsdf, weight, dims, cube lower-corner linear indices)."""
    dims = (47, 47, 2)
    rng = np.random.default_rng(seed)
    tsdf = rng.uniform(0.05, 1.0, dims[::-1]).astype(np.float32)
    weight = np.zeros(dims[::-1], np.float32)
    corners = []
    for q in range(256):
        x, y = 3 * (q % 16), 3 * (q // 16)
        corners.append(x + dims[0] * y)
        for c in range(8):
            k, j, i = c >> 2, y + ((c >> 1) & 1), x + (c & 1)
            weight[k, j, i] = 1.0
            if (q >> c) & 1:
                tsdf[k, j, i] = -tsdf[k, j, i]
    return tsdf.reshape(-1), weight.reshape(-1), dims, np.asarray(corners)


GRIDS = ((1, 1, 1), (2, 2, 2), (9, 8, 17), (17, 9, 8), (33, 17, 9), (33, 5, 5))  # the last: the integration brick + 1 on every axis
SCREENS = ((1, 1), (7, 5), (64, 48))


def integration_cases(dims):
    """The integration cases of one grid: dicts with the volume's geometry, and three views each of a camera, a depth kind, a depth
    map with +inf, 0, negative and NaN pixels, an optional weight map with zeros and an optional image.  The grid spans about
    [-1, 1] from an origin that is no round number; view 0 looks at it from outside, view 1 from inside it (part of the grid is
    behind the eye and whole integration bricks are off the screen), view 2 from outside through a long lens at one corner (part
    of the grid is off the screen); tests/test_tsdf_cpu.py asserts all three."""
    cases = []
    span = max(dims)
    voxel = np.float32(2.137 / max(span - 1, 1))
    origin = (np.array([-0.5137, -0.4871, -0.5093]) * np.float64(voxel) * (np.asarray(dims) - 1) + np.array([0.0131, -0.0173, 0.0097])).astype(np.float32)
    centre = origin.astype(np.float64) + 0.5 * np.float64(voxel) * (np.asarray(dims) - 1)
    corner = origin.astype(np.float64) + np.float64(voxel) * (np.asarray(dims) - 1) * np.array([0.93, 0.91, 0.07])
    sub = 0
    for (w, h) in SCREENS:
        for kind in (DISTANCE, Z):
            for mirrored in (False, True):
                rng = np.random.default_rng(1000 * sub + dims[0] + 7 * dims[2])
                eyes = ((centre + (0.4137, 0.3171, -3.0193), centre), (centre + (0.2113, -0.1371, -0.1931), centre + (0.1, 0.3, 1.0)),
                        (centre + (-2.4171, 1.1931, -2.6113), corner))
                focals = (0.9 * w, 0.6 * w, (2.5 if w > 1 else 0.9) * w)
                views = []
                for k, ((eye, target), focal) in enumerate(zip(eyes, focals)):
                    u = pinhole(w, h, eye, target, focal, mirrored, roll=0.2 + 0.3 * k)
                    ys, xs = np.mgrid[0:h, 0:w]
                    reach = np.linalg.norm(np.asarray(eye) - (corner if k == 2 else centre))
                    depth = (reach * (1.0 + 0.08 * np.sin(0.7 * xs + 0.3 * k) * np.cos(0.9 * ys)) + 0.05 * rng.standard_normal((h, w))).astype(np.float32)
                    if w * h > 4:
                        bad = rng.random((h, w))
                        depth[bad < 0.04] = np.inf
                        depth[(bad >= 0.04) & (bad < 0.07)] = 0.0
                        depth[(bad >= 0.07) & (bad < 0.10)] = -1.5
                        depth[(bad >= 0.10) & (bad < 0.13)] = np.nan
                    obs = None
                    if sub % 2:
                        obs = rng.uniform(0.2, 1.0, (h, w)).astype(np.float32)
                        if w * h > 4:
                            obs[rng.random((h, w)) < 0.1] = 0.0
                    image = rng.random((h, w, 3)).astype(np.float32) if sub % 3 else None
                    views.append(dict(u=u, depth=depth, obs=obs, image=image))
                cases.append(dict(dims=dims, origin=origin, voxel=voxel, trunc=np.float32(3.0 * voxel), kind=kind, screen=(w, h),
                                  mirrored=mirrored, stride=(0, 3, 5)[sub % 3], max_weight=(0.0, 2.0)[(sub // 2) % 2], views=views,
                                  name=f"{w}x{h}-{kind}-{'mirrored' if mirrored else 'pinhole'}"))
                sub += 1
    return cases


def run_case(case):
    """The float64 volume after the case's three views, and per view the nodes it wrote."""
    vol = Volume(case["origin"], case["voxel"], case["dims"], case["trunc"], color=case["stride"] > 0)
    written = []
    for v in case["views"]:
        hit, _ = integrate(vol, v["u"], case["kind"], v["depth"], v["obs"], v["image"] if case["stride"] else None, case["max_weight"])
        written.append(hit)
    return vol, written


# ---- mesh checks the CPU and GPU tests share -----------------------------------------------------------------------------------------
def directed_edges(triangles):
    t = np.asarray(triangles)
    return np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]])


def boundary_edges(triangles):
    """The directed edges whose reverse is not in the mesh; raises if a directed edge occurs twice (two triangles running the same
    way along it: not an oriented manifold)."""
    e = directed_edges(triangles)
    keys = {(int(a), int(b)) for a, b in e}
    assert len(keys) == len(e), "a directed edge is used by two triangles"
    return [k for k in keys if (k[1], k[0]) not in keys]


def euler_characteristic(n_vertices, triangles):
    e = directed_edges(triangles)
    undirected = {(min(int(a), int(b)), max(int(a), int(b))) for a, b in e}
    return n_vertices - len(undirected) + len(triangles)
