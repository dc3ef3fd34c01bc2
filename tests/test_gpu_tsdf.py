"""GPU tests of TSDF fusion and mesh extraction through the C ABI (splat_tsdf_integrate, splat_tsdf_mesh_workspace_bytes,
splat_tsdf_mesh_count, splat_tsdf_mesh_emit) against tests/tsdf_ref.py: the integration against its float64 restatement within
the bounds its docstring derives, the mesh against its marching tetrahedra run on the same float32 volume bytes - counts and the
triangle index buffer exactly, positions and colours within the derived bound.

K_* are twice the largest ratio |error| / (2^-24 bound) measured on one MI355X over every case below (MEASURED_*;
profiles/tsdf_bench.txt records the measurement); each test prints its own largest ratios."""
import ctypes as C

import numpy as np
import pytest
import torch

from splat_renderer_amd import _lib
from splat_renderer_amd import autograd as AG
from tests import tsdf_ref as TR

pytestmark = pytest.mark.gpu

MEASURED_TSDF, MEASURED_WEIGHT, MEASURED_COLOR = 0.384, 0.500, 0.374  # integration: tsdf, weight, colour
MEASURED_POSITION, MEASURED_VERTEX_COLOR = 0.513, 0.394            # extraction: vertex positions, vertex colours
K_TSDF, K_WEIGHT, K_COLOR = 2 * MEASURED_TSDF, 2 * MEASURED_WEIGHT, 2 * MEASURED_COLOR
K_POSITION, K_VERTEX_COLOR = 2 * MEASURED_POSITION, 2 * MEASURED_VERTEX_COLOR
SENTINEL = np.float32(-7.25)


def cuda(a, dtype=np.float32):
    return torch.tensor(np.ascontiguousarray(a, dtype), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def fptr(u):
    return u.ctypes.data_as(C.POINTER(C.c_float)) if u is not None else None


def grid_of(origin, voxel, dims, trunc):
    return _lib.TsdfGrid((C.c_float * 3)(*[float(x) for x in origin]), float(voxel), (C.c_uint32 * 3)(*[int(d) for d in dims]), float(trunc))


def ptr(t):
    return t.data_ptr() if t is not None else None


def ratio(err, bound):
    """max of err / (2^-24 bound) where the bound is positive; the error must be exactly 0 where it is 0."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert (err[bound == 0] == 0).all()
    m = bound > 0
    return float((err[m] / (TR.EPS * bound[m])).max()) if m.any() else 0.0


# ---- integration ------------------------------------------------------------------------------------------------------------------
def gpu_integrate(case):
    """The case's three views through splat_tsdf_integrate into sentinel-filled planes of weight 0: host arrays."""
    n = int(np.prod(case["dims"]))
    g = grid_of(case["origin"], case["voxel"], case["dims"], case["trunc"])
    tsdf, weight = cuda(np.full(n, SENTINEL)), cuda(np.zeros(n))
    color = cuda(np.full((n, 3), SENTINEL)) if case["stride"] else None
    cx = AG._context(tsdf)
    w, h = case["screen"]
    for v in case["views"]:
        depth = cuda(v["depth"])
        obs = cuda(v["obs"]) if v["obs"] is not None else None
        image = None
        if case["stride"] and v["image"] is not None:
            buf = np.full((h, w, case["stride"]), SENTINEL, np.float32)
            buf[..., :3] = v["image"]
            image = cuda(buf)
        AG.check(cx.lib.splat_tsdf_integrate(cx.ctx, C.byref(g), tsdf.data_ptr(), weight.data_ptr(), ptr(color), fptr(v["u"]), TR.KINDS[case["kind"]],
                                             depth.data_ptr(), ptr(obs), ptr(image), case["stride"], w, h, case["max_weight"]), cx.ctx)
        torch.cuda.synchronize()
        if image is not None:
            assert (host(image)[..., 3:] == SENTINEL).all(), "the padding words of the image were written"
    return host(tsdf), host(weight), host(color) if color is not None else None


@pytest.mark.parametrize("dims", TR.GRIDS, ids=lambda d: "x".join(map(str, d)))
def test_integration_against_float64(device, dims):
    worst = {"tsdf": 0.0, "weight": 0.0, "color": 0.0}
    for case in TR.integration_cases(dims):
        vol, _ = TR.run_case(case)
        tsdf, weight, color = gpu_integrate(case)
        sure = ~vol.near
        assert vol.near.sum() <= 0.02 * vol.touched.sum(), case["name"]
        # written exactly when the reference writes it; what was never written keeps its sentinel (and weight 0)
        wrote = weight > 0
        assert np.array_equal(wrote[sure], vol.touched[sure]), (case["name"], int((wrote != vol.touched)[sure].sum()))
        assert (tsdf[~wrote] == SENTINEL).all() and np.isfinite(tsdf).all() and np.isfinite(weight).all(), case["name"]
        m = sure & vol.touched
        worst["tsdf"] = max(worst["tsdf"], ratio(np.abs(tsdf[m] - vol.tsdf[m]), vol.B_tsdf[m]))
        worst["weight"] = max(worst["weight"], ratio(np.abs(weight[m] - vol.weight[m]), vol.additions[m] * np.abs(vol.weight[m])))
        if case["max_weight"] > 0:
            assert weight.max() <= case["max_weight"]
        if color is not None:
            assert (color[~wrote] == SENTINEL).all() and np.isfinite(color).all(), case["name"]
            worst["color"] = max(worst["color"], ratio(np.abs(color[m] - vol.color[m]), vol.B_color[m]))
    print(f"{dims}: largest |error| / (2^-24 bound): tsdf {worst['tsdf']:.3f}, weight {worst['weight']:.3f}, colour {worst['color']:.3f}")
    assert worst["tsdf"] <= K_TSDF and worst["weight"] <= K_WEIGHT and worst["color"] <= K_COLOR, worst


def test_integration_twice_gives_the_same_bytes(device):
    case = TR.integration_cases((33, 17, 9))[9]
    a, b = gpu_integrate(case), gpu_integrate(case)
    for x, y in zip(a, b):
        if x is not None:
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    assert (a[1] > 0).any()


# ---- extraction -------------------------------------------------------------------------------------------------------------------
def gpu_mesh(tsdf, weight, dims, origin, voxel, min_weight=0.0, color=None, tail=96):
    """count, then emit into buffers with a sentinel tail: (vertices, triangles, colors | None) as host arrays of the counted sizes."""
    g = grid_of(origin, voxel, dims, 1.0)
    td, wd = cuda(tsdf), cuda(weight)
    cd = cuda(color) if color is not None else None
    cx = AG._context(td)
    nbytes = int(cx.lib.splat_tsdf_mesh_workspace_bytes(*[int(d) for d in dims]))
    assert nbytes >= 10 * int(np.prod(dims))
    ws = torch.zeros(nbytes, device="cuda", dtype=torch.uint8)
    assert ws.data_ptr() % 16 == 0
    nv, nt = C.c_uint32(12345), C.c_uint32(12345)
    AG.check(cx.lib.splat_tsdf_mesh_count(cx.ctx, C.byref(g), td.data_ptr(), wd.data_ptr(), float(min_weight), ws.data_ptr(), nbytes, C.byref(nv),
                                          C.byref(nt)), cx.ctx)
    nv, nt = nv.value, nt.value
    vertices = torch.full((3 * nv + tail,), float(SENTINEL), device="cuda")
    colors = torch.full((3 * nv + tail,), float(SENTINEL), device="cuda") if color is not None else None
    triangles = torch.full((3 * nt + tail,), -7, device="cuda", dtype=torch.int32)
    AG.check(cx.lib.splat_tsdf_mesh_emit(cx.ctx, C.byref(g), td.data_ptr(), ptr(cd), ws.data_ptr(), nbytes, vertices.data_ptr(), ptr(colors),
                                         triangles.data_ptr()), cx.ctx)
    torch.cuda.synchronize()
    v, t = host(vertices), host(triangles)
    assert (v[3 * nv:] == SENTINEL).all() and (t[3 * nt:] == -7).all(), "something was written past the counted sizes"
    c = None
    if colors is not None:
        c = host(colors)
        assert (c[3 * nv:] == SENTINEL).all()
        c = c[:3 * nv].reshape(nv, 3)
    return v[:3 * nv].reshape(nv, 3), t[:3 * nt].reshape(nt, 3), c


def check_mesh(name, tsdf, weight, dims, origin, voxel, min_weight, color, worst, twice=False):
    ref = TR.marching_tetrahedra(tsdf, weight, dims, origin, voxel, min_weight, color)
    v, t, c = gpu_mesh(tsdf, weight, dims, origin, voxel, min_weight, color)
    assert (len(v), len(t)) == (len(ref.vertices), len(ref.triangles)), (name, len(v), len(t), len(ref.vertices), len(ref.triangles))
    assert np.array_equal(t.astype(np.int64), ref.triangles), name
    worst["position"] = max(worst["position"], ratio(np.abs(v - ref.vertices), ref.B_position))
    if color is not None:
        worst["color"] = max(worst["color"], ratio(np.abs(c - ref.colors), ref.B_color))
    if twice:
        v2, t2, c2 = gpu_mesh(tsdf, weight, dims, origin, voxel, min_weight, color)
        assert np.array_equal(v.view(np.uint32), v2.view(np.uint32)) and np.array_equal(t, t2), name
        assert color is None or np.array_equal(c.view(np.uint32), c2.view(np.uint32)), name
    return ref


def test_extraction_against_the_reference(device):
    worst = {"position": 0.0, "color": 0.0}
    rng = np.random.default_rng(21)
    origin = np.array([0.137, -0.291, 0.413], np.float32)
    # the 256 patterns of one cube, in one grid of cubes kept apart by invalid nodes
    tsdf, weight, dims, _ = TR.pattern_volume()
    ref = check_mesh("patterns", tsdf, weight, dims, origin, 0.173, 0.0, rng.random((tsdf.size, 3)).astype(np.float32), worst, twice=True)
    assert len(ref.triangles) > 1000
    # grids without a cube
    for dims in ((1, 1, 1), (2, 1, 1), (5, 1, 3)):
        n = int(np.prod(dims))
        f = np.where(np.arange(n) % 2, -0.5, 0.5).astype(np.float32)
        ref = check_mesh(str(dims), f, np.ones(n, np.float32), dims, origin, 0.173, 0.0, None, worst)
        assert len(ref.vertices) == 0 and len(ref.triangles) == 0
    # closed surfaces across brick edges
    for make in (TR.sphere_volume, TR.torus_volume):
        tsdf, org, voxel, _ = make()
        dims = (24, 24, 24) if make is TR.sphere_volume else (32, 32, 16)
        color = rng.random((tsdf.size, 3)).astype(np.float32)
        ref = check_mesh(make.__name__, tsdf, np.ones(tsdf.size, np.float32), dims, org, voxel, 0.0, color, worst, twice=True)
        assert TR.boundary_edges(ref.triangles) == []
    # the sphere with a block of unobserved nodes; mixed weights at two thresholds
    dims = (24, 24, 24)
    tsdf, org, voxel, _ = TR.sphere_volume(dims)
    counts = []
    for mixed, min_weight in ((False, 0.0), (True, 0.0), (True, 1.5)):
        weight, _ = TR.holed_weights(dims, mixed)
        ref = check_mesh(f"holed {mixed} {min_weight}", tsdf, weight, dims, org, voxel, min_weight, None, worst)
        counts.append(len(ref.triangles))
    assert counts[0] == counts[1] > counts[2] > 0
    # exact zeros and -0.0 among the samples: outside, t = 0 or 1 on their edges
    tsdf, org, voxel, _ = TR.sphere_volume((12, 12, 12), radius=0.3)
    tsdf = tsdf.copy()
    picks = rng.choice(tsdf.size, 200, replace=False)
    tsdf[picks[:100]], tsdf[picks[100:]] = 0.0, -0.0
    ref = check_mesh("zeros", tsdf, np.ones(tsdf.size, np.float32), (12, 12, 12), org, voxel, 0.0, rng.random((tsdf.size, 3)).astype(np.float32),
                     worst, twice=True)
    assert ((ref.t == 0) | (ref.t == 1)).any() and len(ref.triangles) > 0
    print(f"extraction: largest |error| / (2^-24 bound): positions {worst['position']:.3f}, colours {worst['color']:.3f}")
    assert worst["position"] <= K_POSITION and worst["color"] <= K_VERTEX_COLOR, worst


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_invalid_arguments_are_refused(device):
    dims, w, h = (9, 8, 5), 7, 5
    n = int(np.prod(dims))
    u = TR.pinhole(w, h, (0.4, 0.3, -3.0), (0.0, 0.0, 0.0), 6.0)
    tsdf, weight, color = cuda(np.full(n, SENTINEL)), cuda(np.zeros(n)), cuda(np.full((n, 3), SENTINEL))
    depth, obs, image = cuda(np.full((h, w), 3.0)), cuda(np.ones((h, w))), cuda(np.ones((h, w, 4)))
    cx = AG._context(tsdf)
    lib = cx.lib
    nbytes = int(lib.splat_tsdf_mesh_workspace_bytes(*dims))
    ws = torch.zeros(nbytes, device="cuda", dtype=torch.uint8)
    vertices, vcolors = cuda(np.full(3 * 7 * n, SENTINEL)), cuda(np.full(3 * 7 * n, SENTINEL))
    triangles = torch.full((3 * 12 * n,), -7, device="cuda", dtype=torch.int32)
    nv, nt = C.c_uint32(777), C.c_uint32(777)
    base = dict(origin=(-0.5, -0.5, -0.5), voxel=0.125, dims=dims, trunc=0.4, tsdf=tsdf.data_ptr(), weight=weight.data_ptr(), color=color.data_ptr(),
                u=u, kind=0, depth=depth.data_ptr(), obs=obs.data_ptr(), image=image.data_ptr(), stride=4, w=w, h=h, max_weight=0.0, min_weight=0.0,
                ws=ws.data_ptr(), nbytes=nbytes, vertices=vertices.data_ptr(), vcolors=vcolors.data_ptr(), triangles=triangles.data_ptr(),
                grid=True)

    def calls(a):
        g = C.byref(grid_of(a["origin"], a["voxel"], a["dims"], a["trunc"])) if a["grid"] else None
        return {
            "integrate": lambda: lib.splat_tsdf_integrate(cx.ctx, g, a["tsdf"], a["weight"], a["color"], fptr(a["u"]), a["kind"], a["depth"], a["obs"],
                                                          a["image"], a["stride"], a["w"], a["h"], a["max_weight"]),
            "count": lambda: lib.splat_tsdf_mesh_count(cx.ctx, g, a["tsdf"], a["weight"], a["min_weight"], a["ws"], a["nbytes"], C.byref(nv), C.byref(nt)),
            "emit": lambda: lib.splat_tsdf_mesh_emit(cx.ctx, g, a["tsdf"], a["color"], a["ws"], a["nbytes"], a["vertices"], a["vcolors"], a["triangles"]),
        }

    def untouched():
        torch.cuda.synchronize()
        return ((host(tsdf) == SENTINEL).all() and (host(weight) == 0).all() and (host(color) == SENTINEL).all() and (host(ws) == 0).all()
                and (host(vertices) == SENTINEL).all() and (host(vcolors) == SENTINEL).all() and (host(triangles) == -7).all()
                and nv.value == 777 and nt.value == 777)

    inf, nan = float("inf"), float("nan")
    everywhere = (("grid", False), ("tsdf", None), ("tsdf", tsdf.data_ptr() + 2), ("dims", (0, 8, 5)), ("dims", (9, 2049, 5)), ("dims", (2048, 2048, 257)),
                  ("voxel", 0.0), ("voxel", -1.0), ("voxel", inf), ("voxel", nan), ("trunc", 0.0), ("trunc", inf), ("trunc", nan), ("origin", (nan, 0.0, 0.0)))
    only = {"integrate": (("weight", None), ("weight", weight.data_ptr() + 1), ("color", color.data_ptr() + 2), ("u", None), ("kind", 2), ("depth", None),
                          ("depth", depth.data_ptr() + 2), ("obs", obs.data_ptr() + 1), ("image", image.data_ptr() + 2), ("stride", 2), ("stride", 0),
                          ("w", 0), ("h", 0), ("w", 65536), ("h", 65536), ("max_weight", -1.0), ("max_weight", nan)),
            "count": (("weight", None), ("weight", weight.data_ptr() + 2), ("ws", None), ("ws", ws.data_ptr() + 4), ("nbytes", nbytes - 1),
                      ("min_weight", -1.0), ("min_weight", nan)),
            "emit": (("ws", None), ("ws", ws.data_ptr() + 8), ("nbytes", nbytes - 1), ("vertices", None), ("vertices", vertices.data_ptr() + 2),
                     ("triangles", None), ("triangles", triangles.data_ptr() + 1), ("vcolors", vcolors.data_ptr() + 2), ("color", None))}
    assert lib.splat_tsdf_mesh_workspace_bytes(0, 1, 1) == 0 and lib.splat_tsdf_mesh_workspace_bytes(2049, 1, 1) == 0
    assert lib.splat_tsdf_mesh_workspace_bytes(2048, 2048, 257) == 0 and lib.splat_tsdf_mesh_workspace_bytes(2048, 2048, 256) > 0
    for name in calls(base):
        for key, value in everywhere + only[name]:
            rc = calls(dict(base, **{key: value}))[name]()
            assert rc == -1, f"splat_tsdf_{name}({key}={value}): {rc}"
            assert lib.splat_last_error(cx.ctx)
    assert untouched()
    # ... and the same calls with nothing wrong succeed (optional pointers NULL too)
    assert calls(base)["integrate"]() == 0 and calls(dict(base, color=None, image=None, obs=None, stride=0))["integrate"]() == 0
    assert calls(base)["count"]() == 0 and calls(base)["emit"]() == 0 and calls(dict(base, color=None, vcolors=None))["emit"]() == 0
    torch.cuda.synchronize()
    assert (host(weight) > 0).any()
