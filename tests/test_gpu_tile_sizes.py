"""GPU tests for tile sizes other than 16: the composite of any tile size the binner accepts (k_composite_tile).

The oracle's image does not depend on the tile size (a pixel visits the same depth-ordered entries whatever tile it lies
in), so every size is held to the oracle within the composite's stated tolerance (tests/test_gpu_stages.py), and the
lists of whole frames stay bit-exact against the oracle's binSorted at that size.
"""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import splat_renderer_amd as sr
from oracle import oracle as O
from splat_renderer_amd import _lib
from tests.helpers import assert_same, make_case, oracle_pipeline
from tests.test_gpu_disc import MAX_RIM_FLIPS, TOL, TOL_RIM, disc_case
from tests.test_gpu_stages import check_image_against_oracle, destroy_all, lit_records, run_gpu_pipeline, tile_max

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAPI = os.path.join(ROOT, "splat_renderer_amd", "napi")
NODE = shutil.which("node")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def cdiv(a, b):
    return -(-a // b)


# (tile, n, w, h, seed, radius scale): powers of two and not, ragged right / bottom tiles, a tile larger than the screen
STAGED = [
    (1, 2000, 48, 40, 3, 1.0),
    (4, 20000, 333, 211, 17, 1.5),
    (8, 20000, 333, 211, 17, 1.5),
    (10, 20000, 333, 211, 17, 1.5),
    (24, 20000, 333, 211, 17, 1.5),
    (32, 20000, 333, 211, 17, 1.5),
    (64, 20000, 333, 211, 17, 1.5),
    (400, 20000, 333, 211, 17, 1.5),
]


@pytest.mark.parametrize("tile,n,w,h,seed,rs", STAGED)
def test_staged_composite_vs_oracle(device, tile, n, w, h, seed, rs):
    """ComputeShaderRenderer.render(..., tileSize=T, numTilesX=ceil(w/T), ...): both modes, early-out on and off, ProjectedSplat
    and lit composite records; image within the stated tolerance, per-tile consumed entries the oracle's, staged in between."""
    props, normals, u = make_case(n, w, h, seed, rs)
    ref = oracle_pipeline(props, normals, u, w, h, tile=tile)
    g = run_gpu_pipeline(device, props, normals, u, n, w, h, tile=tile)
    b = g["binner"]
    assert_same(b.getTileCountsBuffer().read(np.uint32), ref["counts"], "tile counts")
    ntx, nty = cdiv(w, tile), cdiv(h, tile)
    counts64 = ref["counts"].astype(np.uint64)
    lit = device.createBufferFrom(lit_records(u, props, normals))
    for mode in (sr.MODE_FRONT_TO_BACK, sr.MODE_REFERENCE_LITERAL):
        for early_out in (False, True):
            want, want8, _, stop, near = O.composite(mode, early_out, props[:, 4:], normals, ref["proj"], ref["indices"],
                                                     ref["counts"], ref["offsets"], w, h, tile=tile, want_stops=True)
            for fmt, records in ((_lib.RECORDS_PROJECTED, g["proj"].getProjectedBuffer()), (_lib.RECORDS_LIT32, lit)):
                r = sr.ComputeShaderRenderer(device, None, "rgba8unorm", mode=mode, earlyOut=early_out, recordFormat=fmt)
                r.consumedBuffer = device.createBuffer(ntx * nty * 16)
                r.consumedBuffer.zero()
                r.render(u, g["pm"].getPropertyBuffer(), b.getTileIndicesBuffer(), g["nbuf"], records, b.getTileCountsBuffer(),
                         b.getTileOffsetsBuffer(), tile, ntx, w, h, wantFloat=True)
                got, got8 = r.readPixelsFloat(), r.readPixels()
                check_image_against_oracle(got, got8, want, want8, near if early_out else None)
                assert (got8[..., 3] == 255).all()
                cons = r.consumedBuffer.read(np.uint64).reshape(nty * ntx, 2)
                ok = ~(tile_max(near, tile) > 0).reshape(-1)
                assert_same(cons[ok, 1], tile_max(stop, tile).reshape(-1)[ok].astype(np.uint64), f"consumed T={tile}")
                assert np.all(cons[:, 1] <= cons[:, 0]) and np.all(cons[:, 0] <= counts64), "consumed <= staged <= count"
                if not early_out:
                    assert_same(cons[:, 1], counts64, f"consumed, early-out off, T={tile}")
                r.destroy()
    lit.destroy()
    destroy_all(g)


@pytest.mark.parametrize("tile", [8, 32])
@pytest.mark.parametrize("early_out", [False, True])
def test_disc_composite_vs_oracle(device, tile, early_out):
    """footprint="disc" at T = 8 and 32 against O.composite_disc(..., tile=T), with test_gpu_disc.py's tolerances."""
    n, w, h = 20000, 333, 200
    props, normals, u = disc_case(n, w, h, 9, 1.0)
    proj_ref, discs = O.project_disc(u, props, normals)
    keys, pay = O.extract_keys(proj_ref, sr.scene.padded_size(n))
    _, order = O.sort_pairs(keys, pay)
    counts, offsets, idx = O.bin_sorted(proj_ref, order, w, h, tile)
    img, img8, _, rim = O.composite_disc(early_out, props[:, 4:], normals, discs, idx, counts, offsets, w, h, tile=tile)
    pm = sr.SplatPropertyManager(device, n)
    pm.setFromArrays(props)
    nbuf = device.createBufferFrom(normals)
    proj = sr.SplatProjector(device, n, footprint="disc")
    sorter = sr.RadixSorter(device, n)
    binner = sr.GPUTileBinner(device, tile)
    proj.project(None, u, pm.getPropertyBuffer(), sorter.getKeysBuffer(), sorter.getPayloadBuffer(), sorter.paddedSize, normalsBuffer=nbuf)
    sorter.sort()
    binner.binSplats(None, proj.getProjectedBuffer(), sorter.getSortedIndicesBuffer(), n, w, h)
    assert_same(binner.getTileIndicesBuffer().read(np.uint32, idx.shape[0]), idx, "disc lists")
    r = sr.ComputeShaderRenderer(device, None, "rgba8unorm", earlyOut=early_out, footprint="disc")
    r.render(u, pm.getPropertyBuffer(), binner.getTileIndicesBuffer(), nbuf, proj.getDiscBuffer(), binner.getTileCountsBuffer(),
             binner.getTileOffsetsBuffer(), tile, cdiv(w, tile), w, h, wantFloat=True)
    got, got8 = r.readPixelsFloat(), r.readPixels()
    d = np.abs(got - img).max(axis=2)
    if early_out:
        assert d.max() <= TOL_RIM and d[rim == 0].max() <= 0.0101
    else:
        assert d[rim == 0].max() <= TOL and d.max() <= TOL_RIM and (d > TOL).sum() <= MAX_RIM_FLIPS
        assert np.abs(got8.astype(int) - img8.astype(int)).max(axis=2)[rim == 0].max() <= 1
    for o in (pm, nbuf, proj, sorter, binner, r):
        o.destroy()


def test_bands_stitch_bit_for_bit(device):
    """At T = 24, tile rows [0, k) and [k, nty) rendered into one image are the whole-screen image bit for bit."""
    tile, n, w, h = 24, 20000, 333, 211
    props, normals, u = make_case(n, w, h, 17, 1.5)
    g = run_gpu_pipeline(device, props, normals, u, n, w, h, tile=tile)
    b = g["binner"]
    ntx, nty = cdiv(w, tile), cdiv(h, tile)
    for mode in (sr.MODE_FRONT_TO_BACK, sr.MODE_REFERENCE_LITERAL):
        r = sr.ComputeShaderRenderer(device, None, "rgba8unorm", mode=mode)
        args = (u, g["pm"].getPropertyBuffer(), b.getTileIndicesBuffer(), g["nbuf"], g["proj"].getProjectedBuffer(),
                b.getTileCountsBuffer(), b.getTileOffsetsBuffer(), tile, ntx, w, h)
        r.render(*args, wantFloat=True)
        whole, whole8 = r.readPixelsFloat().copy(), r.readPixels().copy()
        for k in (1, nty // 2, nty - 1):
            r.outputFloat.zero()
            r.outputTexture.zero()
            for rows in ((0, k), (k, nty)):
                r.tileRows = rows
                r.render(*args, wantFloat=True)
            assert_same(bits(r.readPixelsFloat()), bits(whole), f"bands [0,{k}) + [{k},{nty})")
            assert_same(r.readPixels(), whole8, f"bands [0,{k}) + [{k},{nty}), rgba8")
        r.destroy()
    destroy_all(g)


def test_tile_size_does_not_change_the_picture(device):
    """The oracle's image is tile-size invariant (T = 16 against T = 32, on the CPU arrays); the GPU image at T = 8, 32 and 64
    is within the tolerance of the oracle's T = 16 image."""
    n, w, h = 20000, 333, 211
    props, normals, u = make_case(n, w, h, 17, 1.5)
    ref16 = oracle_pipeline(props, normals, u, w, h, tile=16)
    ref32 = oracle_pipeline(props, normals, u, w, h, tile=32)
    want, want8, _, _, near = O.composite(O.MODE_FRONT_TO_BACK, True, props[:, 4:], normals, ref16["proj"], ref16["indices"],
                                          ref16["counts"], ref16["offsets"], w, h, tile=16, want_stops=True)
    img32, img32_8, _ = O.composite(O.MODE_FRONT_TO_BACK, True, props[:, 4:], normals, ref32["proj"], ref32["indices"],
                                    ref32["counts"], ref32["offsets"], w, h, tile=32)
    assert_same(bits(img32), bits(want), "oracle image, T = 32 against T = 16")
    assert_same(img32_8, want8, "oracle rgba8, T = 32 against T = 16")
    for tile in (8, 32, 64):
        g = run_gpu_pipeline(device, props, normals, u, n, w, h, tile=tile)
        b = g["binner"]
        r = sr.ComputeShaderRenderer(device, None, "rgba8unorm")
        r.render(u, g["pm"].getPropertyBuffer(), b.getTileIndicesBuffer(), g["nbuf"], g["proj"].getProjectedBuffer(),
                 b.getTileCountsBuffer(), b.getTileOffsetsBuffer(), tile, cdiv(w, tile), w, h, wantFloat=True)
        check_image_against_oracle(r.readPixelsFloat(), r.readPixels(), want, want8, near)
        r.destroy()
        destroy_all(g)


@pytest.mark.parametrize("records", ["lit", "projected"])
@pytest.mark.parametrize("order", ["tileFirst", "sortFirst"])
@pytest.mark.parametrize("tile", [8, 32])
def test_whole_frame(device, tile, order, records):
    """Renderer(..., tileSize=T): tile counts, offsets and lists are O.bin_sorted's at that T, the image the oracle's."""
    n, w, h = 20000, 333, 211
    props, normals, u = make_case(n, w, h, 17, 1.5)
    ref = oracle_pipeline(props, normals, u, w, h, tile=tile)
    want, want8, _, _, near = O.composite(O.MODE_FRONT_TO_BACK, True, props[:, 4:], normals, ref["proj"], ref["indices"],
                                          ref["counts"], ref["offsets"], w, h, tile=tile, want_stops=True)
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    r = sr.Renderer(device, None, "rgba8unorm", n, tile, frameOrder=order, records=records)
    r.render(u, pbuf, nbuf, None, w, h, wantFloat=True)
    got, got8 = r.readPixelsFloat(), r.readPixels()
    assert r.binner.getTotalIndices() == ref["indices"].shape[0]
    assert_same(r.binner.getTileCountsBuffer().read(np.uint32), ref["counts"], "frame tile counts")
    offsets = r.binner.getTileOffsetsBuffer().read(np.uint32)
    assert_same(offsets[:ref["counts"].shape[0]], ref["offsets"][:ref["counts"].shape[0]], "frame tile offsets")
    assert_same(r.binner.getTileIndicesBuffer().read(np.uint32, ref["indices"].shape[0]), ref["indices"], "frame tile lists",
                offsets=ref["offsets"])
    check_image_against_oracle(got, got8, want, want8, near)
    r.destroy()
    pbuf.destroy()
    nbuf.destroy()


def test_c2_frame_orders_agree_at_tile_32(device):
    """A C2-size frame at T = 32 (lists about four times longer than at 16): tile-first and sort-first give the same lists and
    the same image bits."""
    n, w, h = sr.scene.CONFIGS["C2"]
    props, normals = sr.scene.make_scene(n)
    cam = sr.Camera()
    cam.setAspect(w / h)
    u = cam.uniforms(w, h)
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    out = {}
    for order in ("tileFirst", "sortFirst"):
        r = sr.Renderer(device, None, "rgba8unorm", n, 32, frameOrder=order)
        r.render(u, pbuf, nbuf, None, w, h, wantFloat=True)
        total = r.finish()
        out[order] = (total, r.binner.getTileCountsBuffer().read(np.uint32).copy(),
                      r.binner.getTileIndicesBuffer().read(np.uint32, total).copy(), bits(r.readPixelsFloat()).copy())
        r.destroy()
    a, b = out["tileFirst"], out["sortFirst"]
    assert a[0] == b[0] and a[0] > 0
    assert_same(a[1], b[1], "C2 T=32 tile counts")
    assert_same(a[2], b[2], "C2 T=32 tile lists")
    assert_same(a[3], b[3], "C2 T=32 image bits")
    pbuf.destroy()
    nbuf.destroy()


def test_tile_renderer_tile_32(device):
    """TileRenderer.render with the reference's eleven arguments and tileSize = 32: the bytes of the ComputeShaderRenderer call
    it fronts."""
    tile, n, w, h = 32, 4000, 208, 120
    props, normals, u = make_case(n, w, h, 23, 1.5)
    g = run_gpu_pipeline(device, props, normals, u, n, w, h, tile=tile)
    b = g["binner"]
    ntx, nty = cdiv(w, tile), cdiv(h, tile)
    cs = sr.ComputeShaderRenderer(device, None, "rgba8unorm")
    cs.render(u, g["pm"].getPropertyBuffer(), b.getTileIndicesBuffer(), g["nbuf"], g["proj"].getProjectedBuffer(),
              b.getTileCountsBuffer(), b.getTileOffsetsBuffer(), tile, ntx, w, h)
    want8 = cs.readPixels().copy()
    tr = sr.TileRenderer(device, None, "rgba8unorm")
    tr.render(u, g["pm"].getPropertyBuffer(), b.getTileIndicesBuffer(), g["nbuf"], b.getTileCountsBuffer().read(np.uint32),
              ntx, nty, tile, 4096, w, h)
    assert_same(tr.readPixels(), want8, "TileRenderer at T = 32")
    cs.destroy()
    tr.destroy()
    destroy_all(g)


JS_FRAME = r"""
const fs = require('fs');
const sr = require('./index.js');
const [propsPath, normalsPath, nStr, wStr, hStr, tStr, outPath] = process.argv.slice(1);
const n = +nStr, W = +wStr, H = +hStr, T = +tStr;
const f32 = (p) => { const b = fs.readFileSync(p); return new Float32Array(b.buffer, b.byteOffset, b.length / 4); };
const device = new sr.Device(0);
const props = new sr.SplatPropertyManager(device, n); props.setFromArrays(f32(propsPath));
const normals = device.createBufferFrom(f32(normalsPath));
const camera = new sr.Camera(); camera.setAspect(W / H);
const r = new sr.Renderer(device, null, 'rgba8unorm', n, T);
r.render(camera.uniforms(W, H), props.getPropertyPlanes(), normals, null, W, H);
fs.writeFileSync(outPath, Buffer.from(r.readPixels().buffer));
console.log(JSON.stringify({ pairs: r.binner.getTotalIndices() }));
"""


@pytest.mark.skipif(NODE is None or not os.path.exists("/usr/include/node/node_api.h"), reason="node / N-API headers not present")
def test_napi_renderer_tile_32(device, tmp_path):
    """The N-API Renderer with tileSize = 32 renders the bytes of the Python Renderer."""
    if not os.path.exists(os.path.join(NAPI, "splat_napi.node")):
        pytest.skip("the N-API addon is not built")
    tile, n, w, h = 32, 4000, 208, 120
    props, normals = sr.scene.make_scene(n, seed=23)
    props.tofile(tmp_path / "props.f32")
    normals.tofile(tmp_path / "normals.f32")
    r = subprocess.run([NODE, "-e", JS_FRAME, str(tmp_path / "props.f32"), str(tmp_path / "normals.f32"), str(n), str(w), str(h),
                        str(tile), str(tmp_path / "frame.rgba8")], cwd=NAPI, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout.strip().splitlines()[-1])
    cam = sr.Camera()
    cam.setAspect(w / h)
    pm = sr.SplatPropertyManager(device, n)
    pm.setFromArrays(props)
    nbuf = device.createBufferFrom(normals)
    py = sr.Renderer(device, None, "rgba8unorm", n, tile)
    py.render(cam.uniforms(w, h), pm.getPropertyPlanes(), nbuf, None, w, h)
    want8 = py.readPixels()
    assert info["pairs"] == py.binner.getTotalIndices() > 0
    assert_same(np.fromfile(tmp_path / "frame.rgba8", np.uint8).reshape(h, w, 4), want8, "N-API Renderer at T = 32")
    py.destroy()
    nbuf.destroy()
    pm.destroy()
