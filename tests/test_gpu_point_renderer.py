"""PointRenderer / splat_point_frame (the reference app's own renderer, src/Renderer.ts) against the test-side reference
tests/point_raster.py: off the contested pixels the winning point's id exactly, its depth within 1e-6 and rgba8 within 1 LSB;
on them an acceptable winner with that winner's colour.  Every scene also bounds its contested fraction, so that no check
passes vacuously."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import splat_renderer_amd as sr
from tests import point_raster as P
from tests.test_point_raster_cpu import cloud, look_down_z
from tests.test_sdf_cpu import main_ts_scene

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAPI = os.path.join(ROOT, "splat_renderer_amd", "napi")


def camera_vp(w, h):
    cam = sr.Camera()
    cam.setAspect(w / h)
    return cam.uniforms(w, h)


def gpu_frame(device, u, pos, grad, scales, w, h, renderer=None, scale_stride=1):
    n = pos.shape[0]
    own = renderer is None
    r = renderer or sr.PointRenderer(device, None, "rgba8unorm", n)
    bufs = [device.createBufferFrom(np.ascontiguousarray(a, F)) for a in (pos, grad, scales)]
    r.render(u, *bufs, w, h, wantFloat=True, scaleStride=scale_stride)
    out = (r.readIds(), r.readDepth(), r.readPixels(), r.readPixelsFloat())
    for b in bufs:
        b.destroy()
    if own:
        r.destroy()
    return out


def check(device, u, pos, grad, scales, w, h, max_contested, renderer=None, min_free_covered=50):
    fr = P.render(u, pos, grad, scales, w, h)
    ids, depth, rgba8, rgba32f = gpu_frame(device, u, pos, grad, scales, w, h, renderer)
    frac = P.compare(fr, ids, depth, rgba8, rgba32f)
    assert frac <= max_contested, f"contested fraction {frac}"
    assert ((fr.ids != P.EMPTY) & ~fr.contested).sum() >= min_free_covered
    return fr, ids


@pytest.mark.parametrize("n,w,h,seed", [(300, 64, 48, 1), (3000, 250, 130, 2), (20000, 320, 200, 3), (8000, 1000, 37, 4)])
def test_random_clouds(device, n, w, h, seed):
    check(device, camera_vp(w, h), *cloud(n, seed, spread=0.8, scale=(0.3, 3.0)), w, h, 0.05)


def test_edges_on_pixel_centres(device):
    """Camera-facing quads whose edges run through pixel centres (in exact arithmetic): the fill rule decides there."""
    w = h = 64
    vp, (f, _, _) = look_down_z(2.0)
    pitch = 2 * 2.0 / (f * w)  # world units per pixel in the plane z = 0
    pos, grad, sc = [], [], []
    for k in range(16):  # centres and half-sides on the pixel grid: x = 6.5 + 3k, y = 12.5 + 12 (k % 4) (+-0.5), half = 3..5 px
        cx = (-0.5 * w + 6.5 + 3 * k) * pitch
        cy = (20.5 - (k % 4) * 12 - (k % 2)) * pitch
        half = (3 + k % 3) * pitch
        pos.append((cx, cy, 0.0, 0))
        grad.append((0, 0, 0, 1))
        sc.append(half / 0.025)
    check(device, vp, np.array(pos, F), np.array(grad, F), np.array(sc, F), w, h, 0.6, min_free_covered=100)


def test_crossing_quads_and_a_deep_stack(device):
    """Quads through one point with different normals (their planes cross inside the pixels), and 700 quads over one tile
    (lists longer than the resolve's 256-record batches)."""
    w, h = 128, 96
    u = camera_vp(w, h)
    rng = np.random.default_rng(7)
    n = 700
    pos = np.zeros((n, 4), F)
    pos[:, :3] = rng.normal(scale=0.02, size=(n, 3))
    pos[:200, :3] = 0.0  # 200 quads through the origin
    grad = np.zeros((n, 4), F)
    grad[:, 1:] = rng.normal(size=(n, 3))
    sc = rng.uniform(4.0, 10.0, n).astype(F)
    check(device, u, pos, grad, sc, w, h, 0.25)


def test_coplanar_ties_go_to_the_lower_index(device):
    w = h = 48
    vp, _ = look_down_z(2.0)
    pos = np.array([[-0.05, 0.0, 0.0, 0], [0.05, 0.0, 0.0, 0]], F)
    grad = np.array([[0, 0, 0, 1], [0, 0, 0, 1]], F)
    sc = np.array([5.0, 5.0], F)
    left, right = P.render(vp, pos[:1], grad[:1], sc[:1], w, h), P.render(vp, pos[1:], grad[1:], sc[1:], w, h)
    overlap = (left.ids == 0) & (right.ids == 0) & ~left.contested & ~right.contested
    assert overlap.sum() > 20
    for order in (pos, pos[::-1].copy()):
        ids, depth, _, _ = gpu_frame(device, vp, order, grad, sc, w, h)
        assert np.all(ids[overlap] == 0)  # exactly equal depths: "less" keeps the first drawn
        check(device, vp, order, grad, sc, w, h, 0.5, min_free_covered=20)


def test_quad_through_the_near_plane(device):
    w = h = 40
    vp, (_, near, far) = look_down_z(2.0)
    zn = 2 * far * near / (far + near)
    fr, ids = check(device, vp, np.array([[0, 0, 2.0 - zn, 0]], F), np.array([[0, 0, 0.6, 0.8]], F), np.array([4.0], F), w, h, 0.2, min_free_covered=20)
    assert (ids == 0).sum() > 20


def test_empty_frames_are_the_clear_colour(device):
    w, h = 37, 21
    u = camera_vp(w, h)
    empty = np.zeros((0, 4), F)
    for pos, grad, sc in ((empty, empty, np.zeros(0, F)),
                          (np.array([[0, 0, 50.0, 0]], F), np.array([[0, 0, 0, 1]], F), np.array([1.0], F)),  # behind the camera
                          (np.array([[0, 0, 0, 0]], F), np.array([[0, np.nan, 0, 1]], F), np.array([1.0], F))):
        ids, depth, rgba8, rgba32f = gpu_frame(device, u, pos, grad, sc, w, h)
        assert np.all(rgba8 == np.array([13, 13, 26, 255], np.uint8))
        assert np.all(rgba32f == P.CLEAR) and np.all(depth == 1.0) and np.all(ids == P.EMPTY)


def test_screen_wider_than_256_tiles(device):
    w, h = 4352, 64
    check(device, camera_vp(w, h), *cloud(6000, 9, spread=1.2, scale=(0.5, 2.0)), w, h, 0.05)


def test_alternating_sizes_on_one_renderer(device):
    r = sr.PointRenderer(device, None, "rgba8unorm", 2500)
    for k, (w, h) in enumerate(((200, 120), (64, 300), (200, 120), (17, 9))):
        check(device, camera_vp(w, h), *cloud(2500, 20 + k, spread=0.7, scale=(0.5, 3.0)), w, h, 0.05, renderer=r, min_free_covered=20)
    r.destroy()


def test_demo_scene_staged_and_fused_producers(device):
    """main.ts's whole frame: SdfSplatSource.step() then the reference's render call.  The staged producer hands over
    CurvatureSampler's scale factors (stride 1), the fused one the .w of vec4(normal, scale) (stride 4): the same image,
    depth and ids byte for byte, and both the reference's."""
    w, h = 480, 320
    u = camera_vp(w, h)
    outs = []
    for fused in (False, True):
        src = sr.SdfSplatSource(device, main_ts_scene(), seed=5)
        src.step(fused=fused)
        pos, grad, scales, stride = src.getPointBuffers()
        assert stride == (4 if fused else 1)
        r = sr.PointRenderer(device, None, "rgba8unorm", src.numPoints)
        r.render(u, pos, grad, scales, w, h, scaleStride=stride)
        outs.append((r.readPixels(), r.readDepth(), r.readIds()))
        n = src.numPoints
        host = (pos.read(F).reshape(n, 4), grad.read(F).reshape(n, 4), scales.read(F).reshape(n, stride)[:, stride - 1].copy())
        r.destroy()
        src.destroy()
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    fr = P.render(u, *host, w, h)
    # (neighbouring surfels are tangent planes of one smooth surface: where they overlap their depths are often within
    # DEPTH_EPS of each other, so this scene has more contested pixels than a random cloud: 5.4 % measured)
    assert P.compare(fr, outs[1][2], outs[1][1], outs[1][0]) < 0.12
    assert (fr.ids != P.EMPTY).mean() > 0.05


def test_frame_loop_render_points(device):
    w, h = 160, 120
    src = sr.SdfSplatSource(device, main_ts_scene(), seed=2)
    src.step()
    loop = sr.FrameLoop(device, src.numPoints, w, h)
    loop.renderPoints(*src.getPointBuffers()[:3], scaleStride=4)
    img = loop.readPixels()
    r = sr.PointRenderer(device, None, "rgba8unorm", src.numPoints)
    r.render(loop.camera.uniforms(w, h), *src.getPointBuffers()[:3], w, h, scaleStride=4)
    assert np.array_equal(img, r.readPixels()) and (img != np.array([13, 13, 26, 255], np.uint8)).any()
    for o in (r, loop, src):
        o.destroy()


def test_gaussian_renderer_is_untouched(device):
    """A PointRenderer frame between two Gaussian Renderer frames: the Gaussian image is bit for bit the same after it, and
    the device's lastBinner / lastProjector still name the Gaussian renderer's."""
    n, w, h = 4000, 160, 112
    props, normals = sr.scene.make_scene(n, seed=31)
    u = camera_vp(w, h)
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    r = sr.Renderer(device, None, "rgba8unorm", n)
    r.render(u, pbuf, nbuf, None, w, h)
    before = r.readPixels()
    last = (device.lastBinner, device.lastProjector)
    check(device, u, *cloud(1500, 11), w, h, 0.05)
    assert (device.lastBinner, device.lastProjector) == last
    r.render(u, pbuf, nbuf, None, w, h)
    assert np.array_equal(before, r.readPixels())
    for o in (r, pbuf, nbuf):
        o.destroy()


@pytest.mark.skipif(shutil.which("node") is None or not os.path.exists("/usr/include/node/node_api.h"),
                    reason="node / N-API headers not present")
def test_js_point_renderer_equals_python(device, tmp_path):
    w, h = 200, 136
    pos, grad, sc = cloud(3000, 13, spread=0.7, scale=(0.5, 3.0))
    for name, a in (("pos", pos), ("grad", grad), ("scales", sc)):
        np.ascontiguousarray(a, F).tofile(tmp_path / f"{name}.f32")
    r = subprocess.run([shutil.which("node"), "point_frame.js", str(tmp_path / "pos.f32"), str(tmp_path / "grad.f32"),
                        str(tmp_path / "scales.f32"), str(pos.shape[0]), str(w), str(h), str(tmp_path / "js_")],
                       cwd=NAPI, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    u = camera_vp(w, h)
    assert np.array_equal(np.array(info["uniforms"], F).view(np.uint32), u.view(np.uint32))
    ids, depth, rgba8, _ = gpu_frame(device, u, pos, grad, sc, w, h)
    assert np.array_equal(np.fromfile(tmp_path / "js_rgba8", np.uint8).reshape(h, w, 4), rgba8)
    assert np.array_equal(np.fromfile(tmp_path / "js_depth", F).reshape(h, w).view(np.uint32), depth.view(np.uint32))
    assert np.array_equal(np.fromfile(tmp_path / "js_ids", np.uint32).reshape(h, w), ids)
    assert np.array_equal(np.fromfile(tmp_path / "js_loop", np.uint8).reshape(h, w, 4), rgba8)  # FrameLoop.renderPoints
