"""The test-side reference of the reference app's renderer (tests/point_raster.py) checked against what can be known
independently: analytic coverage and the GL depth formula, a ray-plane intersection in clip space, the fill and tie rules,
the oracle's own quad geometry (orc_sequential) and the culling rules."""
import numpy as np

from oracle import oracle as O
from tests import point_raster as P

F = np.float32


def look_down_z(distance, fovy=0.8, aspect=1.0, near=0.1, far=100.0):
    """VP (column-major, f32) of a camera at (0, 0, distance) looking at the origin, GL-form perspective."""
    f = 1.0 / np.tan(fovy / 2.0)
    a, b = (far + near) / (near - far), 2.0 * far * near / (near - far)
    m = np.zeros(16, np.float64)
    m[0], m[5], m[10], m[11], m[14], m[15] = f / aspect, f, a, -1.0, a * -distance + b, distance
    return m.astype(F), (f, near, far)


def cloud(n, seed, spread=0.6, scale=(0.5, 1.5)):
    rng = np.random.default_rng(seed)
    pos = np.zeros((n, 4), F)
    pos[:, :3] = rng.uniform(-spread, spread, (n, 3))
    grad = np.zeros((n, 4), F)
    grad[:, 1:] = rng.normal(size=(n, 3))
    return pos, grad, rng.uniform(*scale, n).astype(F)


def one_point(p, g, s):
    return np.array([[p[0], p[1], p[2], 0]], F), np.array([[0, g[0], g[1], g[2]]], F), np.array([s], F)


def test_camera_facing_quad_covers_the_analytic_square_at_the_gl_depth():
    W = H = 64
    D = 2.0
    vp, (f, near, far) = look_down_z(D)
    scale = F(7.3)  # half-side 0.1825 world units
    pos, grad, sc = one_point((0.01, -0.02, 0.0), (0, 0, 1), scale)
    fr = P.render(vp, pos, grad, sc, W, H)
    s = float(F(0.025) * scale)
    x0, x1 = ((f * (0.01 - s) / D + 1) * W / 2, (f * (0.01 + s) / D + 1) * W / 2)
    y0, y1 = ((1 - f * (-0.02 + s) / D) * H / 2, (1 - f * (-0.02 - s) / D) * H / 2)
    cx = np.arange(W) + 0.5
    cy = np.arange(H) + 0.5
    want = ((cy[:, None] >= y0) & (cy[:, None] < y1)) & ((cx[None, :] >= x0) & (cx[None, :] < x1))  # top-left: left/top edges in
    assert want.sum() > 100
    assert np.array_equal(fr.ids == 0, want)
    gl = (far + near) / (far - near) - 2 * far * near / ((far - near) * D)
    assert np.abs(fr.depth[want] - gl).max() < 1e-6
    assert np.all(fr.depth[~want] == 1.0) and not fr.contested.any()
    # colour: n = (0, 0, 1): c = (0.5, 0.5, 1) times 0.3 + 0.7 / sqrt(3)
    kd = 0.3 + 0.7 / np.sqrt(3)
    assert np.allclose(fr.rgba32f[want][0], [0.5 * kd, 0.5 * kd, kd, 1.0], atol=1e-6)
    assert np.array_equal(fr.rgba8[~want][0], [13, 13, 26, 255])


def test_depth_is_the_ray_plane_intersection_in_clip_space():
    W, H = 96, 80
    vp, _ = look_down_z(1.5, aspect=W / H)
    pos, grad, sc = one_point((0.05, 0.02, 0.1), (0.4, -0.3, 0.85), F(6.0))
    fr = P.render(vp, pos, grad, sc, W, H)
    clip, _, _ = P.point_setup(vp, pos, grad, sc)
    C = clip[0].astype(np.float64)  # corner k: (x, y, z, w)
    ys, xs = np.nonzero(fr.ids == 0)
    assert ys.shape[0] > 200
    worst = 0.0
    for y, x in zip(ys, xs):
        nx, ny = (x + 0.5) / W * 2 - 1, 1 - (y + 0.5) / H * 2
        depths = []
        for tri in P.TRIANGLES:
            V = C[list(tri)]
            A = np.stack([V[:, 0] - nx * V[:, 3], V[:, 1] - ny * V[:, 3], np.ones(3)])
            lam = np.linalg.solve(A, [0.0, 0.0, 1.0])
            if np.all(lam >= -1e-12):
                depths.append(lam @ V[:, 2] / (lam @ V[:, 3]))
        assert depths, (y, x)
        worst = max(worst, min(abs(d - fr.depth[y, x]) for d in depths))
    assert worst < 1e-9


def test_coplanar_quads_lower_index_wins():
    W = H = 48
    vp, _ = look_down_z(2.0)
    pos = np.array([[-0.05, 0.0, 0.0, 0], [0.05, 0.0, 0.0, 0]], F)
    grad = np.array([[0, 0, 0, 1], [0, 0, 0, 1]], F)
    sc = np.array([5.0, 5.0], F)
    left, right = P.render(vp, pos[:1], grad[:1], sc[:1], W, H), P.render(vp, pos[1:], grad[1:], sc[1:], W, H)
    overlap = (left.ids == 0) & (right.ids == 0)
    assert overlap.sum() > 20 and (left.ids == 0).sum() > overlap.sum() + 20
    # the same depth bit for bit (VP has no x, y terms in z and w and the quads lie in one plane z = 0): an exact tie
    assert np.array_equal(left.depth[overlap], right.depth[overlap])
    a = P.render(vp, pos, grad, sc, W, H)
    b = P.render(vp, pos[::-1].copy(), grad, sc, W, H)
    assert np.all(a.ids[overlap] == 0) and np.all(b.ids[overlap] == 0)  # the left quad in a, the right one in b
    assert np.array_equal(a.ids == 1, (right.ids == 0) & ~overlap) and np.array_equal(b.ids == 1, (left.ids == 0) & ~overlap)
    # another correct rasteriser may break a tie differently only through rounding: the overlap is contested, with both
    assert a.contested[overlap].all() and all(a.acceptable[y * W + x] == {0, 1} for y, x in zip(*np.nonzero(overlap)))


def test_every_pixel_orc_sequential_touches_is_inside_the_quad():
    W, H = 80, 64
    u = np.zeros(22, F)
    vp, _ = look_down_z(1.6, aspect=W / H)
    u[:16], u[20], u[21] = vp, W, H
    checked = 0
    for seed in range(6):
        pos, grad, sc = cloud(1, seed, spread=0.3, scale=(3.0, 6.0))
        fr = P.render(vp, pos, grad, sc, W, H)
        _, _, n = P.point_setup(vp, pos, grad, sc)
        props = np.zeros((1, 8), F)
        props[0, :3], props[0, 3], props[0, 4:] = pos[0, :3], F(0.025) * sc[0], (1, 0, 0, 1)
        _, out8 = O.sequential(u, props, n.astype(F), np.array([0], np.uint32), W, H)
        touched = np.any(out8 != P.clear8(), axis=2)
        assert np.all((fr.ids == 0)[touched] | fr.contested[touched])
        checked += int(touched.sum())
    assert checked > 100


def test_culling():
    W = H = 40
    vp, (f, near, far) = look_down_z(2.0)
    # behind the camera (a corner at w <= 0), beyond the far plane (z/w > 1), NaN gradient, zero scale, zero gradient
    for p, g, s in (((0, 0, 2.5), (0, 0, 1), 4.0), ((0, 0, -200.0), (0, 0, 1), 4.0), ((0, 0, 0), (np.nan, 0, 1), 4.0),
                    ((0, 0, 0), (0, 0, 1), 0.0), ((0, 0, 0), (0, 0, 0), 4.0)):
        fr = P.render(vp, *one_point(p, g, F(s)), W, H)
        assert np.all(fr.ids == P.EMPTY) and np.all(fr.depth == 1.0), (p, g, s)
    # a quad tilted through the z/w = 0 plane (view depth 2fn/(f+n)): only its far part is drawn, every depth >= 0
    zn = 2 * far * near / (far + near)
    fr = P.render(vp, *one_point((0, 0, 2.0 - zn), (0, 0.6, 0.8), F(4.0)), W, H)
    clip, _, _ = P.point_setup(vp, *one_point((0, 0, 2.0 - zn), (0, 0.6, 0.8), F(4.0)))
    _, _, Z, ok = P.screen_corners(clip, W, H)
    assert ok[0] and Z.min() < -0.01 and Z.max() > 0.01
    drawn = fr.ids == 0
    assert drawn.sum() > 20 and np.all(fr.depth[drawn] >= 0)


def test_random_cloud_contested_fraction_is_small():
    W, H = 120, 90
    vp, _ = look_down_z(2.2, aspect=W / H)
    fr = P.render(vp, *cloud(800, 5, scale=(1.5, 3.0)), W, H)
    covered = fr.ids != P.EMPTY
    assert covered.mean() > 0.3
    assert fr.contested.mean() < 0.03
    # the reference against itself: compare() accepts its own outputs
    P.compare(fr, fr.ids, fr.depth.astype(F), fr.rgba8, fr.rgba32f)
