"""GPU tests of the anisotropic Gaussian footprint (SPLAT_FOOTPRINT_ELLIPSOID) against the NumPy restatement
(tests/ellipsoid_ref.py).

Bit-exact: records, ProjectedSplat records, keys and payload of splat_project_ellipsoid; tile lists against the oracle's
bin_sorted on the GPU's ProjectedSplats.  Tolerances: SH colours within 2e-6 of float64; composited rgba32f within 1e-4 and
rgba8 within 1 LSB of the restated composite, off the rim (|d2 - 1| <= 1e-3: the cut is a step of opacity e^-4.5) and off
the pixels whose early-out stop may move by one entry (near); whole frames the same against it on every route."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import splat_renderer_amd as sr
from oracle import np_oracle as NO
from oracle import oracle as O
from splat_renderer_amd import _lib
from tests import ellipsoid_ref as ER
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu

TOL = 1e-4
MAX_RIM_FLIPS = 24
TOL_RIM = 0.02  # opacity e^-4.5 = 0.0111 times a colour <= 1, plus slack
CASES = [  # n, w, h, seed, spread, scale
    (3000, 160, 120, 1, 1.0, 0.03),
    (20000, 333, 200, 2, 1.0, 0.02),
    (500, 64, 64, 3, 0.5, 0.2),      # splats larger than the screen
    (10000, 256, 256, 4, 1.5, 0.01),
    (40000, 640, 360, 5, 1.2, 0.015),
]


def camera_u(w, h):
    vp, eye = O.camera(aspect=w / h)
    return O.uniforms(vp, eye, w, h)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cloud_of(device, pos, scl, rot, col):
    return sr.GaussianCloud.fromArrays(device, pos, scl, rot, colors=col)


def restated(u, pos, scl, rot, col, w, h, tile=16, early_out=True):
    rec, proj, keys = ER.project(u, pos, scl, rot)
    _, order = NO.sort_pairs(keys, np.arange(keys.shape[0], dtype=np.uint32))
    counts, offsets, idx = NO.bin_sorted(proj, order, w, h, tile)
    c = ER.composite(rec, col, proj[:, 4], idx, counts, offsets, w, h, tile, early_out)
    c.update(rec=rec, proj=proj, keys=keys, order=order, counts=counts, offsets=offsets, indices=idx)
    return c


def check_image(got, ref, what):
    bad = ref["rim"] | ref["near"]
    d = np.abs(got[..., :3].astype(np.float64) - ref["img"][..., :3]).max(axis=2)
    assert d[~bad].max(initial=0) <= TOL, f"{what}: {d[~bad].max()} off the rim"
    assert d.max() <= TOL_RIM, f"{what}: {d.max()} on the rim"
    assert (d > TOL).sum() <= MAX_RIM_FLIPS, f"{what}: {(d > TOL).sum()} pixels beyond {TOL}"


def check_image8(got8, ref, what):
    bad = ref["rim"] | ref["near"]
    want8 = NO.unorm8(ref["img"]).astype(np.int32)
    d = np.abs(got8[..., :3].astype(np.int32) - want8[..., :3]).max(axis=2)
    assert d[~bad].max(initial=0) <= 1, f"{what}: rgba8 off by {d[~bad].max()} LSB off the rim"


@pytest.mark.parametrize("n,w,h,seed,spread,scale", CASES)
def test_projector_bit_exact(device, n, w, h, seed, spread, scale):
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale)
    u = camera_u(w, h)
    rec, _, _ = ER.project(u, pos, scl, rot)
    assert (rec[:8] == 0).all(axis=1)[[2, 3, 4, 5]].all() and (rec != 0).any(axis=1).sum() > n // 2
    projector_bit_exact(device, u, pos, scl, rot, col)


def projector_bit_exact(device, u, pos, scl, rot, col):
    """splat_project_ellipsoid under the uniform block u against ER.project, bit for bit; returns the restated records."""
    n = pos.shape[0]
    rec, proj, keys = ER.project(u, pos, scl, rot)
    cloud = cloud_of(device, pos, scl, rot, col)
    p = sr.SplatProjector(device, n, footprint="ellipsoid")
    sorter = sr.RadixSorter(device, n)
    with pytest.raises(sr.SplatError):
        p.project(None, u, None)  # the cloud is required
    p.project(None, u, None, sorter.getKeysBuffer(), sorter.getPayloadBuffer(), sorter.paddedSize, cloud=cloud)
    assert_same(bits(p.getDiscBuffer().read(np.float32, n * 8).reshape(n, 8)), bits(rec), f"records {n}")
    assert_same(bits(p.getProjectedBuffer().read(np.float32, n * 8).reshape(n, 8)), bits(proj), f"projected {n}")
    kp = sorter.getKeysBuffer().read(np.uint32)
    assert_same(kp[:n], keys, f"keys {n}")
    assert (kp[n:] == 0xFFFFFFFF).all()
    assert_same(sorter.getPayloadBuffer().read(np.uint32)[:n], np.arange(n, dtype=np.uint32), f"payload {n}")
    # q, -q and 2q: the same bits
    cloud2 = cloud_of(device, pos, scl, -2.0 * rot, col)
    p.project(None, u, None, cloud=cloud2)
    assert_same(bits(p.getDiscBuffer().read(np.float32, n * 8)), bits(rec).reshape(-1), f"records -2q {n}")
    for o in (p, sorter, cloud, cloud2):
        o.destroy()
    return rec


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_sh_colors_float64(device, degree):
    n = 5000
    rng = np.random.default_rng(degree)
    pos, scl, rot, _ = ER.make_cloud(n, degree, degenerate=False)
    nb = (degree + 1) ** 2
    sh = rng.normal(0, 0.5, (n, nb, 3)).astype(np.float32)
    op = rng.uniform(0, 1, n).astype(np.float32)
    u = camera_u(64, 64)
    cloud = sr.GaussianCloud.fromArrays(device, pos, scl, rot, opacity=op, sh=sh)
    cloud.updateColors(u[16:19])
    got = cloud.colorOpacity.read(np.float32).reshape(n, 4)
    want = ER.sh_colors(u[16:19].astype(np.float64), pos, sh, degree, op)
    assert np.abs(got - want).max() <= 2e-6
    # a stride the float4 path cannot take: the scalar loads, the same values
    d = device
    sh5 = np.zeros((n, 3 * nb + 1), np.float32)
    sh5[:, :3 * nb] = sh.reshape(n, -1)
    b = d.createBufferFrom(sh5)
    out = d.createBuffer(n * 16)
    e = np.ascontiguousarray(u[16:19])
    _lib.check(d.lib.splat_sh_colors(d.ctx, e.ctypes.data_as(C.POINTER(C.c_float)), cloud.positions.ptr, 1, b.ptr, 3 * nb + 1, degree,
                                     cloud.opacity.ptr, n, out.ptr), d.ctx)
    assert np.abs(out.read(np.float32).reshape(n, 4) - want).max() <= 2e-6
    assert d.lib.splat_sh_colors(d.ctx, e.ctypes.data_as(C.POINTER(C.c_float)), cloud.positions.ptr, 1, b.ptr, 3 * nb - 1, degree,
                                 cloud.opacity.ptr, n, out.ptr) == -1
    for o in (b, out, cloud):
        o.destroy()


@pytest.mark.parametrize("n,w,h,seed,spread,scale", CASES[:4])
@pytest.mark.parametrize("kernel", ["px", "quadrant"])
def test_staged_pipeline(device, n, w, h, seed, spread, scale, kernel):
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale)
    u = camera_u(w, h)
    cloud = cloud_of(device, pos, scl, rot, col)
    p = sr.SplatProjector(device, n, footprint="ellipsoid")
    sorter = sr.RadixSorter(device, n)
    binner = sr.GPUTileBinner(device, 16)
    p.project(None, u, None, sorter.getKeysBuffer(), sorter.getPayloadBuffer(), sorter.paddedSize, cloud=cloud)
    keys = sorter.getKeysBuffer().read(np.uint32)[:n]  # (before the sort, which leaves its output in these buffers)
    sorter.sort()
    binner.binSplats(None, p.getProjectedBuffer(), sorter.getSortedIndicesBuffer(), n, w, h)
    gproj = p.getProjectedBuffer().read(np.float32, n * 8).reshape(n, 8)
    _, order = NO.sort_pairs(keys, np.arange(n, dtype=np.uint32))
    counts, offsets, idx = NO.bin_sorted(gproj, order, w, h)
    total = binner.getTotalIndices()
    assert total == idx.shape[0]
    assert_same(binner.getTileCountsBuffer().read(np.uint32), counts, "ellipsoid counts")
    assert_same(binner.getTileIndicesBuffer().read(np.uint32, total), idx, "ellipsoid lists", offsets=offsets)
    rec = p.getDiscBuffer().read(np.float32, n * 8).reshape(n, 8)
    ref = ER.composite(rec, col, gproj[:, 4], idx, counts, offsets, w, h)
    device.compositeOptions("pixel" if kernel == "px" else "quadrant")
    try:
        cr = sr.ComputeShaderRenderer(device, None, "rgba8unorm", footprint="ellipsoid")
        args = (u, cloud, binner.getTileIndicesBuffer(), None, p.getDiscBuffer(), binner.getTileCountsBuffer(),
                binner.getTileOffsetsBuffer(), 16, -(-w // 16), w, h)
        with pytest.raises(sr.SplatError):  # the 32-byte records carry no depth
            cr.render(*args, wantAov=True)
        cr.render(*args, wantFloat=True)
        check_image(cr.readPixelsFloat(), ref, f"staged {kernel} {n}")
        check_image8(cr.readPixels(), ref, f"staged {kernel} {n}")
        # alpha and ids (no depth) beside the same image
        d = device
        al, ids = d.createBuffer(w * h * 4), d.createBuffer(w * h * 4)
        aov = _lib.Aov(None, al.ptr, ids.ptr)
        cfg = sr.CompositeCfg(0, 1, 16, 0, _lib.U32_MAX, _lib.RECORDS_PROJECTED, 1, _lib.FOOTPRINT_ELLIPSOID)
        img = d.createBuffer(w * h * 16)
        _lib.check(d.lib.splat_composite_aov(d.ctx, C.byref(cfg), cloud.colorOpacity.ptr, 1, None, 1, p.getDiscBuffer().ptr,
                                             binner.getTileIndicesBuffer().ptr, binner.getTileCountsBuffer().ptr,
                                             binner.getTileOffsetsBuffer().ptr, w, h, None, img.ptr, None, C.byref(aov)), d.ctx)
        assert np.array_equal(bits(img.read(np.float32)), bits(cr.readPixelsFloat()).reshape(-1))
        check_aov(al.read(np.float32).reshape(h, w), ids.read(np.uint32).reshape(h, w), None, ref, f"staged {kernel} {n}")
        for b in (al, ids, img):
            b.destroy()
    finally:
        device.compositeOptions()
    for o in (p, sorter, binner, cr, cloud):
        o.destroy()


def check_aov(alpha, ids, dep, ref, what):
    bad = ref["rim"] | ref["near"]
    da = np.abs(alpha.astype(np.float64) - ref["alpha"])
    assert da[~bad].max(initial=0) <= 2e-5, f"{what}: alpha {da[~bad].max()}"
    empty = ~bad & (ref["id"] == 0xFFFFFFFF)
    assert (ids[empty] == 0xFFFFFFFF).all(), what
    agree = (ids[~bad] == ref["id"][~bad]).mean()
    assert agree >= 0.995, f"{what}: ids agree on {agree}"
    if dep is not None:
        dep = dep.astype(np.float64)
        m = ~bad & np.isfinite(ref["depth"]) & (ref["alpha"] > 1e-3)
        assert np.all(np.abs(dep[m] - ref["depth"][m]) <= 1e-3 * np.abs(ref["depth"][m]) + 1e-4), what
        assert np.isposinf(dep[empty]).all(), what


FRAMES = [  # frame order, records, write projected, tile, w, h
    ("default", "lit", True, 16, 333, 200),
    ("sortFirst", "lit", True, 16, 333, 200),
    ("default", "projected", True, 16, 333, 200),
    ("sortFirst", "projected", False, 16, 333, 200),
    ("default", "lit", False, 8, 160, 120),
    ("default", "projected", True, 32, 160, 120),
    ("default", "lit-always", True, 1, 300, 20),     # 300 x 20 tiles: beyond 256 tiles a side (wide ranges, sort-first)
    ("default", "projected", False, 1, 300, 20),
]


@pytest.mark.parametrize("order,records,write,tile,w,h", FRAMES)
def test_whole_frames(device, order, records, write, tile, w, h):
    pos, scl, rot, col = ER.make_cloud(6000, 11, 1.0, 0.03)
    whole_frame(device, camera_u(w, h), pos, scl, rot, col, order, records, write, tile, w, h)


def whole_frame(device, u, pos, scl, rot, col, order, records, write, tile, w, h):
    """One Renderer(footprint="ellipsoid") frame under the uniform block u against the restated frame; returns the restatement."""
    n = pos.shape[0]
    ref = restated(u, pos, scl, rot, col, w, h, tile, early_out=True)
    cloud = cloud_of(device, pos, scl, rot, col)
    r = sr.Renderer(device, None, "rgba8unorm", n, tileSize=tile, frameOrder=order, footprint="ellipsoid", writeProjected=write,
                    records=records)
    r.render(u, cloud, None, None, w, h, wantFloat=True, wantAov=True) if (write or records != "projected") else \
        r.render(u, cloud, None, None, w, h, wantFloat=True)
    r.finish()
    what = f"frame {order} {records} {write} {tile} {w}x{h}"
    total = r.binner.getTotalIndices()
    assert_same(r.binner.getTileCountsBuffer().read(np.uint32), ref["counts"], what + " counts")
    assert_same(r.binner.getTileIndicesBuffer().read(np.uint32, total), ref["indices"], what + " lists")
    if write:
        assert_same(bits(r.projector.getProjectedBuffer().read(np.float32, n * 8).reshape(n, 8)), bits(ref["proj"]), what + " projected")
    check_image(r.outputFloat.read(np.float32).reshape(h, w, 4), ref, what)
    check_image8(r.output.read(np.uint8).reshape(h, w, 4), ref, what)
    if write or records != "projected":
        check_aov(r.aov.readAlpha(), r.aov.readIds(), r.aov.readDepth(), ref, what)
    else:  # the 32-byte records carry no depth
        with pytest.raises(sr.SplatError):
            r.render(u, cloud, None, None, w, h, wantAov=True)
    cloud.destroy()
    return ref


def test_sh_frame_and_frames_alternate(device):
    """A cloud with SH: the frame evaluates the colour towards the camera; ellipsoid, disc and isotropic frames alternating on
    one device leave the disc and isotropic images bit-identical to standalone ones."""
    from tests.helpers import make_case
    n, w, h = 4000, 256, 200
    props, normals, u = make_case(n, w, h, 5)
    pos, scl, rot, _ = ER.make_cloud(n, 21, 1.0, 0.03)
    rng = np.random.default_rng(3)
    sh = rng.normal(0, 0.4, (n, 16, 3)).astype(np.float32)
    op = rng.uniform(0.3, 1, n).astype(np.float32)
    cloud = sr.GaussianCloud.fromArrays(device, pos, scl, rot, opacity=op, sh=sh)
    col = ER.sh_colors(u[16:19].astype(np.float64), pos, sh, 3, op).astype(np.float32)
    ref = restated(u, pos, scl, rot, col, w, h)
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    solo = {}
    for fp in ("disc", "isotropic"):
        r = sr.Renderer(device, None, "rgba8unorm", n, footprint=fp)
        r.render(u, pbuf, nbuf, None, w, h, wantFloat=True)
        solo[fp] = r.outputFloat.read(np.float32)
    rs = {fp: sr.Renderer(device, None, "rgba8unorm", n, footprint=fp) for fp in ("ellipsoid", "disc", "isotropic")}
    for _ in range(2):
        for fp, r in rs.items():
            if fp == "ellipsoid":
                r.render(u, cloud, None, None, w, h, wantFloat=True)
                check_image(r.outputFloat.read(np.float32).reshape(h, w, 4), ref, "sh frame")
            else:
                r.render(u, pbuf, nbuf, None, w, h, wantFloat=True)
                assert np.array_equal(bits(r.outputFloat.read(np.float32)), bits(solo[fp])), fp
    cloud.destroy()


def test_rejections(device):
    n, w, h = 64, 64, 64
    pos, scl, rot, col = ER.make_cloud(n, 1)
    u = camera_u(w, h)
    cloud = cloud_of(device, pos, scl, rot, col)
    d, lib = device, device.lib
    with pytest.raises(sr.SplatError):  # the literal blend
        sr.Renderer(device, None, "rgba8unorm", n, footprint="ellipsoid", mode=_lib.MODE_REFERENCE_LITERAL).render(u, cloud, None, None, w, h)
    with pytest.raises(sr.SplatError):  # a strict band of tile rows
        sr.Renderer(device, None, "rgba8unorm", n, footprint="ellipsoid").render(u, cloud, None, None, w, h, tileRows=(1, 3))
    with pytest.raises(sr.SplatError):  # normals passed
        sr.Renderer(device, None, "rgba8unorm", n, footprint="ellipsoid").render(u, cloud, cloud.positions, None, w, h)
    sorter, binner = sr.RadixSorter(device, n), sr.GPUTileBinner(device, 16)
    out = d.createBuffer(w * h * 4)
    uf = u.ctypes.data_as(C.POINTER(C.c_float))
    args = (cloud.positions.ptr, cloud.scales.ptr, cloud.rotations.ptr, cloud.colorOpacity.ptr, n, w, h, None, out.ptr, None, None)

    def frame(cfg, a=args):
        return lib.splat_render_frame_ellipsoids(d.ctx, sorter._s, binner._b, C.byref(cfg), uf, *a)
    ok = sr.CompositeCfg(0, 1, 16, 0, _lib.U32_MAX, _lib.RECORDS_PROJECTED, 1, _lib.FOOTPRINT_ELLIPSOID)
    assert frame(ok) == 0
    assert frame(sr.CompositeCfg(0, 1, 16, 0, _lib.U32_MAX, _lib.RECORDS_PROJECTED, 0, _lib.FOOTPRINT_ELLIPSOID)) == -1  # not prelit
    assert frame(sr.CompositeCfg(1, 1, 16, 0, _lib.U32_MAX, _lib.RECORDS_PROJECTED, 1, _lib.FOOTPRINT_ELLIPSOID)) == -1  # literal
    assert frame(sr.CompositeCfg(0, 1, 16, 0, _lib.U32_MAX, _lib.RECORDS_PROJECTED, 1, _lib.FOOTPRINT_DISC)) == -1
    assert frame(ok, (cloud.positions.ptr, cloud.scales.ptr + 4) + args[2:]) == -1  # misaligned plane
    # footprint 2 through the other frame entries (no planes) and the band frame
    assert lib.splat_render_frame_planes_aov(d.ctx, sorter._s, binner._b, C.byref(ok), uf, cloud.positions.ptr, cloud.colorOpacity.ptr,
                                             None, n, w, h, None, out.ptr, None, None) == -1
    assert lib.splat_band_frame(d.ctx, sorter._s, binner._b, C.byref(ok), cloud.colorOpacity.ptr, None, cloud.positions.ptr, n, w, h,
                                out.ptr, None, None) == -1
    with pytest.raises(sr.SplatError):
        sr.SequentialRenderer(device, None, "rgba8unorm", n, footprint="ellipsoid")
    for o in (sorter, binner, out, cloud):
        o.destroy()


def test_ply_cloud_renders_to_png(device, tmp_path):
    from tests.test_ellipsoid_cpu import write_ply
    n, w, h = 2000, 160, 120
    pos, scl, rot, _ = ER.make_cloud(n, 7, 1.0, 0.03, degenerate=False)
    rng = np.random.default_rng(7)
    sh = rng.normal(0, 0.5, (n, 9, 3)).astype(np.float32)
    op = rng.uniform(0.3, 1, n).astype(np.float32)
    path = tmp_path / "scene.ply"
    write_ply(path, pos[:, :3], np.log(scl[:, :3]), rot, np.log(op / (1 - op)), sh)
    g = sr.load_gaussian_ply(str(path))
    cloud = sr.GaussianCloud.fromArrays(device, g["positions"], g["scales"], g["rotations"], opacity=g["opacity"], sh=g["sh"])
    u = camera_u(w, h)
    r = sr.Renderer(device, None, "rgba8unorm", n, footprint="ellipsoid")
    r.render(u, cloud, None, None, w, h, wantFloat=True)
    col = ER.sh_colors(u[16:19].astype(np.float64), g["positions"], g["sh"], 2, g["opacity"]).astype(np.float32)
    check_image(r.outputFloat.read(np.float32).reshape(h, w, 4), restated(u, pos, g["scales"], g["rotations"], col, w, h), "ply")
    png = tmp_path / "scene.png"
    sr.write_png(str(png), r.output.read(np.uint8).reshape(h, w, 4))
    assert png.stat().st_size > 100
    cloud.destroy()


def test_js_frame_matches_python(device, tmp_path):
    node = shutil.which("node")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not node or not os.path.exists(os.path.join(root, "splat_renderer_amd", "napi", "splat_napi.node")):
        pytest.skip("node or the N-API addon is not here")
    n, w, h = 3000, 160, 120
    pos, scl, rot, col = ER.make_cloud(n, 9, 1.0, 0.03)
    u = camera_u(w, h)
    for name, a in (("pos", pos), ("scl", scl), ("rot", rot), ("col", col), ("u", u)):
        np.ascontiguousarray(a, np.float32).tofile(tmp_path / f"{name}.f32")
    cloud = cloud_of(device, pos, scl, rot, col)
    r = sr.Renderer(device, None, "rgba8unorm", n, footprint="ellipsoid")
    r.render(u, cloud, None, None, w, h)
    want = r.output.read(np.uint8)
    out = subprocess.run([node, os.path.join(root, "splat_renderer_amd", "napi", "ellipsoid_frame.js"), str(tmp_path), str(n), str(w), str(h)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-3000:]
    got = np.fromfile(tmp_path / "out.u8", np.uint8)
    assert np.array_equal(got, want)
    cloud.destroy()
