"""The reference of tests/tsdf_ref.py (float64 TSDF integration, marching tetrahedra on the Kuhn split) held to facts that do not
come from it: what a mesh of a closed surface must look like, where an analytic surface lies, and a node worked by hand.  No GPU."""
import itertools
import os

import numpy as np
import pytest

from tests import tsdf_ref as TR


def winding_ok(mesh, dims, origin, voxel):
    """Every triangle's (b - a) x (c - a) points from its tetrahedron's inside vertices towards the outside ones (or is zero)."""
    nx, ny, _ = dims
    X = TR.node_grid(dims, origin, voxel)
    for tri, cube, p in zip(mesh.triangles, mesh.triangle_cube, mesh.triangle_tet):
        v = TR.tet_vertices(p)
        nodes = [int(cube + q[0] + nx * (q[1] + ny * q[2])) for q in v]
        ins = np.array([mesh.inside[m] for m in nodes])
        outward = X[nodes][~ins].mean(axis=0) - X[nodes][ins].mean(axis=0)
        a, b, c = mesh.vertices[tri]
        if np.cross(b - a, c - a) @ outward < -1e-12:
            return False
    return True


def test_every_sign_pattern_of_one_cube():
    rng = np.random.default_rng(11)
    dims, origin, voxel = (2, 2, 2), np.array([0.3, -0.2, 0.1], np.float32), 0.25
    for pattern in range(256):
        mag = rng.uniform(0.05, 1.0, 8)
        tsdf = np.where([(pattern >> c) & 1 for c in range(8)], -mag, mag).astype(np.float32)
        mesh = TR.marching_tetrahedra(tsdf, np.ones(8, np.float32), dims, origin, voxel)
        # every vertex lies on an edge whose endpoints differ in sign
        d = np.asarray(TR.EDGE_DIRS)[mesh.vertex_edge].reshape(-1, 3)
        other = mesh.vertex_node + d[:, 0] + 2 * d[:, 1] + 4 * d[:, 2]
        assert (mesh.inside[mesh.vertex_node] != mesh.inside[other]).all()
        assert ((mesh.t > 0) & (mesh.t < 1)).all()
        # none unreferenced; ordered by (node, edge)
        assert set(mesh.triangles.reshape(-1).tolist()) == set(range(len(mesh.vertices)))
        order = mesh.vertex_node * 7 + mesh.vertex_edge
        assert (np.diff(order) > 0).all()
        assert winding_ok(mesh, dims, origin, voxel)
        # 0 / 1 / 2 triangles per tetrahedron by the number of inside vertices; in tetrahedron order
        for p in range(6):
            ins = sum((pattern >> (q[0] + 2 * q[1] + 4 * q[2])) & 1 for q in TR.tet_vertices(p))
            assert (mesh.triangle_tet == p).sum() == {0: 0, 1: 1, 2: 2, 3: 1, 4: 0}[ins]
        assert (np.diff(mesh.triangle_tet) >= 0).all()
        # smallest id first
        if len(mesh.triangles):
            assert (mesh.triangles[:, 0] == mesh.triangles.min(axis=1)).all()
        # a closed pattern-independent fact: inside a single cube the surface has no edge used twice in the same direction
        TR.boundary_edges(mesh.triangles)


def test_the_six_tetrahedra_fill_the_cube_and_agree_on_its_faces():
    """The Kuhn split: six tetrahedra of volume 1/6 each; every face of the cube is cut by the diagonal from its lowest corner."""
    total = 0.0
    diagonals = set()
    for p in range(6):
        v = np.array(TR.tet_vertices(p), float)
        total += abs(np.linalg.det(v[1:] - v[0])) / 6.0
        for a, b in itertools.combinations(range(4), 2):
            d = tuple(int(x) for x in (v[b] - v[a]))
            assert d in TR.EDGE_DIRS  # every edge runs from its lower node in one of the seven directions
            if sum(d) == 2:
                diagonals.add((tuple(int(x) for x in v[a]), d))
    assert abs(total - 1.0) < 1e-12
    # six face diagonals, each from the lowest corner of its face: the face x = 0 and the face x = 1 carry the same one
    assert len(diagonals) == 6
    for d in ((1, 1, 0), (1, 0, 1), (0, 1, 1)):
        axis = d.index(0)
        starts = sorted(s for s, dd in diagonals if dd == d)
        assert starts == [(0, 0, 0), tuple(1 if k == axis else 0 for k in range(3))]


def closed_surface_checks(mesh, euler):
    assert len(mesh.triangles) > 100
    assert TR.boundary_edges(mesh.triangles) == []  # every edge: exactly two triangles, in opposite directions
    assert TR.euler_characteristic(len(mesh.vertices), mesh.triangles) == euler
    assert set(mesh.triangles.reshape(-1).tolist()) == set(range(len(mesh.vertices)))


def test_sphere_is_a_closed_surface_near_the_true_one():
    """Linear interpolation along an edge of length L <= sqrt(3) h of a distance field phi misses phi by at most L^2 / 8 max |phi''|
    along the edge; for a sphere |phi''| <= 1 / |X - centre| <= 1 / (R - L) on an edge that crosses the surface.  Where the
    interpolant is 0 the true distance is therefore at most 3 h^2 / (8 (R - sqrt(3) h)) (plus the float32 rounding of the samples)."""
    dims = (24, 24, 24)
    tsdf, origin, voxel, centre = TR.sphere_volume(dims)
    radius = 0.71
    mesh = TR.marching_tetrahedra(tsdf, np.ones(tsdf.size, np.float32), dims, origin, voxel)
    closed_surface_checks(mesh, 2)
    assert winding_ok(mesh, dims, origin, voxel)
    bound = 3 * voxel ** 2 / (8 * (radius - np.sqrt(3) * voxel)) + 1e-6
    miss = np.abs(np.linalg.norm(mesh.vertices - centre, axis=1) - radius)
    print(f"sphere: {len(mesh.vertices)} vertices, {len(mesh.triangles)} triangles, largest miss {miss.max():.3g} of {bound:.3g}")
    assert miss.max() <= bound
    # outward normals: the enclosed volume is positive and close to the ball's
    a, b, c = (mesh.vertices[mesh.triangles[:, k]] - centre for k in range(3))
    volume = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0
    assert abs(volume / (4 / 3 * np.pi * radius ** 3) - 1) < 0.02


def test_torus_is_a_closed_surface_of_genus_one():
    """As the sphere's bound, with |phi''| <= max(1 / (r - L), 1 / (R - r - L)): the two principal curvatures of the offset surfaces of
    a torus are 1 / (distance to the ring circle) and at most 1 / (distance to the axis)."""
    dims = (32, 32, 16)
    major, minor = 0.8, 0.31
    tsdf, origin, voxel, centre = TR.torus_volume(dims)
    mesh = TR.marching_tetrahedra(tsdf, np.ones(tsdf.size, np.float32), dims, origin, voxel)
    closed_surface_checks(mesh, 0)
    L = np.sqrt(3) * voxel
    bound = L ** 2 / 8 * max(1 / (minor - L), 1 / (major - minor - L)) + 1e-6
    X = mesh.vertices - centre
    miss = np.abs(np.hypot(np.hypot(X[:, 0], X[:, 1]) - major, X[:, 2]) - minor)
    print(f"torus: {len(mesh.vertices)} vertices, {len(mesh.triangles)} triangles, largest miss {miss.max():.3g} of {bound:.3g}")
    assert miss.max() <= bound


def test_sphere_with_a_block_of_unobserved_nodes():
    dims = (24, 24, 24)
    nx, ny, _ = dims
    tsdf, origin, voxel, _ = TR.sphere_volume(dims)
    weight, block = TR.holed_weights(dims)
    mesh = TR.marching_tetrahedra(tsdf, weight, dims, origin, voxel)
    full = TR.marching_tetrahedra(tsdf, np.ones(tsdf.size, np.float32), dims, origin, voxel)
    assert 0 < len(mesh.triangles) < len(full.triangles)
    # cubes touching the block are absent
    corners = [dx + nx * (dy + ny * dz) for dx, dy, dz in itertools.product((0, 1), repeat=3)]
    touches = lambda cube: any(block[cube + c] for c in corners)  # noqa: E731
    assert not any(touches(int(c)) for c in mesh.triangle_cube)
    # ... and only they: every other triangle of the full mesh is still there
    kept = [tuple(sorted((full.vertex_node[v] * 7 + full.vertex_edge[v]) for v in t)) for t, c in zip(full.triangles, full.triangle_cube)
            if not touches(int(c))]
    mine = [tuple(sorted((mesh.vertex_node[v] * 7 + mesh.vertex_edge[v]) for v in t)) for t in mesh.triangles]
    assert kept == mine
    assert set(mesh.triangles.reshape(-1).tolist()) == set(range(len(mesh.vertices)))
    # the remaining boundary edges are exactly those next to the block: both ends lie on edges of cubes that touch it
    boundary = TR.boundary_edges(mesh.triangles)
    assert boundary
    dropped = {int(c) for c in full.triangle_cube if touches(int(c))}
    near_block = set()
    for t, c in zip(full.triangles, full.triangle_cube):
        if int(c) in dropped:
            near_block.update(int(full.vertex_node[v]) * 7 + int(full.vertex_edge[v]) for v in t)
    for a, b in boundary:
        assert {int(mesh.vertex_node[a]) * 7 + int(mesh.vertex_edge[a]), int(mesh.vertex_node[b]) * 7 + int(mesh.vertex_edge[b])} <= near_block
    # and the full mesh's edges between a kept and a dropped triangle are all boundary now
    assert len(boundary) == sum(1 for e in TR.boundary_edges(full.triangles[[int(c) not in dropped for c in full.triangle_cube]]))


def test_exact_zeros_are_outside_and_give_legal_degenerate_triangles():
    dims = (3, 3, 3)
    tsdf = np.full(27, 0.5, np.float32)
    tsdf[13] = -0.5                    # the centre node is inside ...
    tsdf[14], tsdf[12] = 0.0, -0.0     # ... two neighbours are exactly 0 and -0: outside, t = 1 on their edges
    mesh = TR.marching_tetrahedra(tsdf, np.ones(27, np.float32), dims, np.zeros(3, np.float32), 1.0)
    assert mesh.inside.sum() == 1
    assert TR.boundary_edges(mesh.triangles) == [] and TR.euler_characteristic(len(mesh.vertices), mesh.triangles) == 2
    assert np.isfinite(mesh.vertices).all()
    assert (np.abs(mesh.vertices - np.array([2.0, 1.0, 1.0])).max(axis=1) == 0).sum() == 1  # the vertex that sits on the zero node


def test_one_node_against_one_pixel_by_hand():
    """A 1 x 1 x 1 volume at the origin, a camera at (0, 0, -2) looking down +z, a 1 x 1 screen: the node's distance and clip w are
    both 2.  trunc = 0.5."""
    u = TR.pinhole(1, 1, (0.0, 0.0, -2.0), (0.0, 0.0, 0.0), 1.0, roll=0.0)
    for kind in (TR.DISTANCE, TR.Z):
        vol = TR.Volume((0.0, 0.0, 0.0), 1.0, (1, 1, 1), 0.5)
        depth = lambda d: np.array([[d]], np.float32)  # noqa: E731
        hit, _ = TR.integrate(vol, u, kind, depth(3.0))          # the surface is 1 behind the node: free space
        assert hit[0] and vol.tsdf[0] == 1.0 and vol.weight[0] == 1.0
        hit, _ = TR.integrate(vol, u, kind, depth(1.4))          # the node is 0.6 behind the surface, beyond the band: not written
        assert not hit[0] and vol.tsdf[0] == 1.0 and vol.weight[0] == 1.0
        hit, _ = TR.integrate(vol, u, kind, depth(1.75), obs=np.array([[3.0]], np.float32))  # s = -0.25, f = -0.5, weight 3
        assert hit[0] and abs(vol.tsdf[0] - (1.0 * 1 + -0.5 * 3) / 4) < 1e-12 and vol.weight[0] == 4.0
        for bad in (np.inf, 0.0, -1.0, np.nan):
            hit, _ = TR.integrate(vol, u, kind, depth(bad))
            assert not hit[0] and vol.weight[0] == 4.0
        hit, _ = TR.integrate(vol, u, kind, depth(2.0), max_weight=4.5)  # s = 0: f = 0; the weight is clamped after the mean
        assert hit[0] and abs(vol.tsdf[0] - (-0.125 * 4 + 0) / 5) < 1e-12 and vol.weight[0] == 4.5
    behind = TR.pinhole(1, 1, (0.0, 0.0, 2.0), (0.0, 0.0, 4.0), 1.0, roll=0.0)  # looks away from the node
    vol = TR.Volume((0.0, 0.0, 0.0), 1.0, (1, 1, 1), 0.5)
    assert not TR.integrate(vol, behind, TR.DISTANCE, np.array([[3.0]], np.float32))[0][0]


@pytest.mark.parametrize("dims", TR.GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_integration_cases_have_few_decision_near_nodes(dims):
    """The GPU test leaves decision-near nodes out; its cases are chosen so that they are at most 2 % of the nodes the reference
    touches, and every case touches some and leaves some alone where the grid has more than a few nodes."""
    worst = 0.0
    for case in TR.integration_cases(dims):
        vol, written = TR.run_case(case)
        assert vol.touched.any(), case["name"]
        share = (vol.near & vol.touched).sum() / vol.touched.sum()
        worst = max(worst, share, vol.near.sum() / vol.touched.sum())
        assert vol.near.sum() <= 0.02 * vol.touched.sum(), (case["name"], int(vol.near.sum()), int(vol.touched.sum()))
        if vol.n > 8 and case["screen"] != (1, 1):
            assert not vol.touched.all(), case["name"]
        assert np.abs(vol.tsdf[vol.touched]).max() <= 1.0
    print(f"{dims}: largest share of decision-near nodes {worst:.4f}")
    if min(dims) < 5:
        return
    # what the cases are built to contain: part of the grid behind the eye of view 1, part of it off the screen of views 1 and 2,
    # and in some view at least one whole integration brick off the screen beside bricks that are on it
    nx, ny, nz = dims
    bx, by, bz = TR.INTEGRATE_BRICK
    case = TR.integration_cases(dims)[-1]
    X = np.concatenate([TR.node_grid(dims, case["origin"], case["voxel"]), np.ones((nx * ny * nz, 1))], axis=1)
    w, h = case["screen"]
    behind, on_screen, bricks_off = [], [], []
    for v in case["views"]:
        clip = X @ v["u"][:16].astype(np.float64).reshape(4, 4)
        with np.errstate(all="ignore"):
            pu, pv = (clip[:, 0] / clip[:, 3] * 0.5 + 0.5) * w, (0.5 - 0.5 * clip[:, 1] / clip[:, 3]) * h
        front = clip[:, 3] > 0
        on = (front & (pu >= 0) & (pu < w) & (pv >= 0) & (pv < h)).reshape(nz, ny, nx)
        bricks = [on[k:k + bz, j:j + by, i:i + bx].any() for k in range(0, nz, bz) for j in range(0, ny, by) for i in range(0, nx, bx)]
        behind.append(int((~front).sum()))
        on_screen.append(int(on.sum()))
        bricks_off.append(any(bricks) and not all(bricks))
    assert 0 < behind[1] < len(X) and 0 < on_screen[1] < len(X) and 0 < on_screen[2] < len(X) and any(bricks_off)


def test_save_mesh_ply_round_trip(tmp_path):
    import splat_renderer_amd as sr
    tsdf, origin, voxel, _ = TR.sphere_volume((12, 12, 12), radius=0.3)
    mesh = TR.marching_tetrahedra(tsdf, np.ones(tsdf.size, np.float32), (12, 12, 12), origin, voxel)
    v, t = mesh.vertices.astype(np.float32), mesh.triangles.astype(np.int32)
    colors = np.random.default_rng(2).random((len(v), 3)).astype(np.float32)
    colors[0], colors[1] = (-0.5, 0.0, 0.5), (1.0, 1.5, 0.999)  # clamped to [0, 255]
    for col in (None, colors):
        path = os.path.join(tmp_path, "mesh.ply")
        sr.save_mesh_ply(path, v, t, col)
        raw = open(path, "rb").read()
        head, body = raw.split(b"end_header\n", 1)
        lines = head.decode("ascii").split("\n")
        assert lines[0] == "ply" and lines[1] == "format binary_little_endian 1.0"
        assert f"element vertex {len(v)}" in lines and f"element face {len(t)}" in lines
        assert ("property uchar red" in lines) == (col is not None)
        vt = np.dtype([("xyz", "<f4", 3)] + ([("rgb", "u1", 3)] if col is not None else []))
        ft = np.dtype([("n", "u1"), ("idx", "<i4", 3)])
        assert len(body) == len(v) * vt.itemsize + len(t) * ft.itemsize
        verts = np.frombuffer(body, vt, len(v))
        faces = np.frombuffer(body, ft, len(t), offset=len(v) * vt.itemsize)
        assert np.array_equal(verts["xyz"], v) and (faces["n"] == 3).all() and np.array_equal(faces["idx"], t)
        if col is not None:
            assert np.array_equal(verts["rgb"], np.clip(np.rint(col.astype(np.float64) * 255.0), 0, 255).astype(np.uint8))
            assert verts["rgb"][0].tolist() == [0, 0, 128] and verts["rgb"][1].tolist() == [255, 255, 255]
    with pytest.raises(sr.SplatError):
        sr.save_mesh_ply(os.path.join(tmp_path, "bad.ply"), v, np.array([[0, 1, len(v)]], np.int32))
