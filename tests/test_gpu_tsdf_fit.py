"""GPU tests of the Python surface of TSDF fusion: TsdfVolume, GaussianFit.extract_mesh and save_mesh_ply, end to end on a sphere
of small opaque splats, against the reference of tests/tsdf_ref.py fed the same rendered depth and alpha maps, downloaded.

The comparison is made where the two pipelines can be held to each other exactly: the fused volume against the float64
integration of the same maps within the integration bounds (decision-near nodes left out), and the mesh against the reference's
marching tetrahedra of that volume's own float32 bytes - topology exactly, positions and colours within the vertex bound."""
import os

import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from splat_renderer_amd import autograd as AG
from tests import tsdf_ref as TR
from tests.test_gpu_tsdf import K_COLOR, K_POSITION, K_TSDF, K_VERTEX_COLOR, K_WEIGHT, ratio

pytestmark = pytest.mark.gpu

W = H = 96
VOXEL = 0.08
# median | |p| - 1 | of the mesh's vertices: what the reference pipeline gave on these maps when the test was written, and the
# sanity bound, twice that.  (The blended centre-distance depth biases the surface slightly, and a splat's soft rim widens each view's silhouette: a
# measurement, not a derivation.)
MEASURED_MEDIAN_MISS = 0.0300
MEDIAN_MISS_BOUND = 2 * MEASURED_MEDIAN_MISS


def sphere_fit():
    n = 4000
    k = np.arange(n) + 0.5
    phi, z = np.pi * (1 + 5 ** 0.5) * k, 1 - 2 * k / n
    r = np.sqrt(1 - z * z)
    means = np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(np.float32)
    # flat discs in the tangent plane, as a fit trained with the normal-consistency term has them: the quaternion (w, x, y, z) that
    # turns the z axis, the short one, into the outward normal
    scales = np.tile(np.array([0.045, 0.045, 0.005], np.float32), (n, 1))
    rotations = np.stack([1 + means[:, 2], -means[:, 1], means[:, 0], np.zeros(n, np.float32)], axis=1)
    rotations /= np.linalg.norm(rotations, axis=1, keepdims=True)
    sh = ((0.5 + 0.4 * means) - 0.5) / 0.28209479177387814  # degree 0: colour = 0.5 + C0 sh
    return sr.GaussianFit(means, scales, rotations, np.full(n, 0.95, np.float32), sh.astype(np.float32)[:, None, :])


def cameras():
    eyes = [(3.0 * np.cos(a) * np.cos(e), 3.0 * np.sin(e), 3.0 * np.sin(a) * np.cos(e))
            for a, e in zip(np.arange(8) * (2 * np.pi / 8) + 0.3, (0.2, -0.5, 0.9, -0.1, 0.6, -0.8, 0.35, -0.3))]
    return [TR.pinhole(W, H, eye, (0.0, 0.0, 0.0), 110.0, roll=0.1 * k) for k, eye in enumerate(eyes)]


@pytest.fixture(scope="module")
def fused(device):
    """The fit, its cameras, what extract_mesh returns (with the volume) and the downloaded maps of every view."""
    fit = sphere_fit()
    cams = cameras()
    vertices, triangles, colors, vol = fit.extract_mesh(cams, W, H, VOXEL, return_volume=True)
    maps = []
    with torch.no_grad():
        for u in cams:
            rgb, alpha, depth = fit.render(u, W, H, return_depth=True)
            maps.append((depth.cpu().numpy(), alpha.cpu().numpy(), rgb.cpu().numpy()))
    torch.cuda.synchronize()
    return fit, cams, vertices, triangles, colors, vol, maps


def test_extract_mesh_equals_the_reference_pipeline(fused):
    fit, cams, vertices, triangles, colors, vol, maps = fused
    assert vol.trunc == 4 * VOXEL and vol.color is not None
    lo = (fit.means.min(dim=0).values - vol.trunc).tolist()
    assert np.allclose(vol.origin, lo, rtol=0, atol=1e-6) and all(d > 2.6 / VOXEL for d in vol.dims)
    # the volume against the float64 integration of the same maps
    ref = TR.Volume(vol.origin, vol.voxel, vol.dims, vol.trunc, color=True)
    for u, (depth, alpha, rgb) in zip(cams, maps):
        TR.integrate(ref, u, TR.DISTANCE, depth, np.where(alpha >= 0.5, alpha, 0.0).astype(np.float32), rgb)
    tsdf, weight, color = (t.cpu().numpy().reshape(ref.n, -1).squeeze() for t in (vol.tsdf, vol.weight, vol.color))
    sure = ~ref.near
    assert ref.near.sum() <= 0.02 * ref.touched.sum() and ref.touched.sum() > 1000
    assert np.array_equal((weight > 0)[sure], ref.touched[sure])
    m = sure & ref.touched
    worst = (ratio(np.abs(tsdf[m] - ref.tsdf[m]), ref.B_tsdf[m]), ratio(np.abs(weight[m] - ref.weight[m]), ref.additions[m] * ref.weight[m]),
             ratio(np.abs(color[m] - ref.color[m]), ref.B_color[m]))
    print(f"fused volume: largest |error| / (2^-24 bound): tsdf {worst[0]:.3f}, weight {worst[1]:.3f}, colour {worst[2]:.3f}")
    assert worst[0] <= K_TSDF and worst[1] <= K_WEIGHT and worst[2] <= K_COLOR
    # the mesh against marching tetrahedra of the volume's own bytes
    mesh = TR.marching_tetrahedra(tsdf, weight, vol.dims, vol.origin, vol.voxel, 0.0, color)
    v, t, c = vertices.cpu().numpy(), triangles.cpu().numpy(), colors.cpu().numpy()
    assert v.dtype == np.float32 and t.dtype == np.int32 and c.dtype == np.float32
    assert len(t) > 1000 and v.shape == mesh.vertices.shape and np.array_equal(t.astype(np.int64), mesh.triangles)
    rp, rc = ratio(np.abs(v - mesh.vertices), mesh.B_position), ratio(np.abs(c - mesh.colors), mesh.B_color)
    print(f"mesh: {len(v)} vertices, {len(t)} triangles; largest |error| / (2^-24 bound): positions {rp:.3f}, colours {rc:.3f}")
    assert rp <= K_POSITION and rc <= K_VERTEX_COLOR
    # the sanity of the whole: the surface is the unit sphere, to the bias of the blended depth
    miss = float(np.median(np.abs(np.linalg.norm(mesh.vertices, axis=1) - 1.0)))
    print(f"median | |p| - 1 | = {miss:.4f} (bound {MEDIAN_MISS_BOUND:.4f})")
    assert miss <= MEDIAN_MISS_BOUND
    assert float(np.median(np.abs(np.linalg.norm(v.astype(np.float64), axis=1) - 1.0))) <= MEDIAN_MISS_BOUND
    assert ((c >= 0) & (c <= 1)).all()


def test_mesh_saves_and_loads_back(fused, tmp_path):
    _, _, vertices, triangles, colors, _, _ = fused
    path = os.path.join(tmp_path, "sphere.ply")
    sr.save_mesh_ply(path, vertices.cpu(), triangles.cpu(), colors.cpu())
    head, body = open(path, "rb").read().split(b"end_header\n", 1)
    assert f"element vertex {len(vertices)}".encode() in head and f"element face {len(triangles)}".encode() in head
    vt, ft = np.dtype([("xyz", "<f4", 3), ("rgb", "u1", 3)]), np.dtype([("n", "u1"), ("idx", "<i4", 3)])
    assert len(body) == len(vertices) * vt.itemsize + len(triangles) * ft.itemsize
    assert np.array_equal(np.frombuffer(body, vt, len(vertices))["xyz"], vertices.cpu().numpy())
    assert np.array_equal(np.frombuffer(body, ft, len(triangles), offset=len(vertices) * vt.itemsize)["idx"], triangles.cpu().numpy())


def test_extract_mesh_leaves_the_pending_frame_alone_and_takes_bounds(fused):
    fit, cams = fused[0], fused[1]
    rgb, alpha = fit.render(cams[0], W, H)
    frame = fit._frame
    v, t = fit.extract_mesh(cams[:2], W, H, 0.16, trunc=0.4, bounds=((-1.2, -1.2, -1.2), (1.2, 1.2, 1.2)), color=False)
    assert fit._frame is frame and v.shape[1] == 3 and t.shape[1] == 3 and len(t) > 0
    assert float(v.min()) >= -1.2 and float(v.max()) <= 1.2 + 0.16


def test_tsdf_volume_integrates_a_rendered_frame_in_place(device):
    fit = sphere_fit()
    u = cameras()[0]
    scales, opacity = torch.exp(fit.log_scales), torch.sigmoid(fit.opacity_logits)
    with torch.no_grad():
        rgb, alpha, depth = AG.render_gaussians(u, fit.means, scales, fit.rotations, opacity, sh=fit.sh, width=W, height=H, return_depth=True)
    assert depth.shape == (H, W) and rgb.stride(1) == 4  # the view of the frame's (H, W, 4) buffer: read where it lies
    vol = sr.TsdfVolume((-1.3, -1.3, -1.3), 0.1, (27, 27, 27), 0.3, color=True)
    before = (depth.clone(), alpha.clone(), rgb.clone())
    vol.integrate(depth, u, image=rgb, weight=alpha)
    ref = TR.Volume(vol.origin, vol.voxel, vol.dims, vol.trunc, color=True)
    TR.integrate(ref, u, TR.DISTANCE, depth.cpu().numpy(), alpha.cpu().numpy(), rgb.cpu().numpy())
    tsdf, weight = vol.tsdf.cpu().numpy().reshape(-1), vol.weight.cpu().numpy().reshape(-1)
    m = ~ref.near
    assert ref.touched.sum() > 100 and np.array_equal((weight > 0)[m], ref.touched[m])
    m &= ref.touched
    assert ratio(np.abs(tsdf[m] - ref.tsdf[m]), ref.B_tsdf[m]) <= K_TSDF
    assert ratio(np.abs(vol.color.cpu().numpy().reshape(-1, 3)[m] - ref.color[m]), ref.B_color[m]) <= K_COLOR
    for a, b in zip(before, (depth, alpha, rgb)):
        assert torch.equal(a, b)
    # "z" depth, no colour, a capped weight; then reset
    vol.integrate(depth, u, depth_kind="z", max_weight=1.5)
    assert float(vol.weight.max()) <= 1.5
    assert len(vol.extract_mesh()) == 3
    vol.reset()
    assert float(vol.weight.abs().max()) == 0.0
    v, t, c = vol.extract_mesh()
    assert v.shape == (0, 3) and t.shape == (0, 3) and c.shape == (0, 3) and t.dtype == torch.int32

    # refusals
    bad_u = torch.tensor(u, requires_grad=True)
    for call in (lambda: vol.integrate(depth.cpu(), u), lambda: vol.integrate(depth[:-1], u, weight=alpha), lambda: vol.integrate(depth, u, weight=alpha.cpu()),
                 lambda: vol.integrate(depth.reshape(-1), u), lambda: vol.integrate(depth, u, image=rgb[:, :-1]), lambda: vol.integrate(depth, bad_u),
                 lambda: vol.integrate(depth.double(), u), lambda: vol.integrate(depth, u, depth_kind="planar"), lambda: vol.integrate(depth, u, max_weight=-1.0),
                 lambda: vol.extract_mesh(min_weight=float("nan")), lambda: sr.TsdfVolume((0, 0, 0), 0.1, (0, 4, 4), 0.3),
                 lambda: sr.TsdfVolume((0, 0, 0), 0.1, (4, 4, 2049), 0.3), lambda: sr.TsdfVolume((0, 0, 0), 0.0, (4, 4, 4), 0.3),
                 lambda: sr.TsdfVolume((0, 0, 0), 0.1, (4, 4, 4), 0.3, device="cpu")):
        with pytest.raises(sr.SplatError):
            call()
    assert float(vol.weight.abs().max()) == 0.0
