"""GPU tests of the frame path on screens beyond 256 x 256 tiles.

There a frame carries each splat's tile range in 8 bytes with 16-bit coordinates (tile_range.h: pack_range_wide) instead of the
4-byte range32, and bins sort-first.  With that range the binner never reads the records, so these frames work on every screen
the binner takes (at most 65535 tiles a side, 2^24 in all):
- whole frames with lit composite records (SPLAT_RECORDS_LIT32, Renderer(records="lit-always"));
- oriented-disc frames without the ProjectedSplat by-product (writeProjected=False), and with lit disc records;
- splat_band_frame over oriented-disc exchange records (SPLAT_RECORDS_DISC48), as well as ProjectedSplat and 16-byte ones.

Every case is held to O.bin_sorted's lists at its tile size and to the bits of the frame it replaces: the isotropic frame with
ProjectedSplat records, the disc frame that writes them, the whole frame that the bands stitch to.  Each screen lies just past
one edge (the cases at or below 256 tiles a side are in test_gpu_tile_counts.py).
"""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import splat_renderer_amd as sr
from oracle import oracle as O
from splat_renderer_amd import _lib
from tests.helpers import assert_same, make_case, oracle_pipeline
from tests.test_gpu_stages import check_image_against_oracle

pytestmark = pytest.mark.gpu


def cdiv(a, b):
    return -(-a // b)


# (tile, width, height, splats, radius scale): scenes of at most about 10 M pairs (seed 17)
SCREENS = [
    pytest.param(8, 2049, 1024, 20000, 1.0, id="257x128-tiles-T8-2049x1024"),
    pytest.param(8, 1024, 2049, 20000, 0.8, id="128x257-tiles-T8-1024x2049"),
    pytest.param(16, 4112, 2160, 20000, 1.0, id="257x135-tiles-T16-4112x2160"),
    pytest.param(4, 1920, 1080, 20000, 0.6, id="17bit-T4-1920x1080"),
    pytest.param(7, 3840, 2160, 20000, 0.5, id="18bit-T7-3840x2160"),
    pytest.param(1, 1920, 1080, 20000, 0.1, id="21bit-T1-1920x1080"),
    pytest.param(1, 65535, 1, 2000, 1.0, id="65535-tiles-wide-T1-65535x1"),
    pytest.param(1, 1, 65535, 2000, 0.3, id="65535-tiles-high-T1-1x65535"),
]
DISC_SCREENS = [SCREENS[0], SCREENS[1], SCREENS[2], SCREENS[3]]


def check_lists(binner, ref, ntx, nty, what):
    total = ref["indices"].shape[0]
    assert binner.getTotalIndices() == total, what
    assert_same(binner.getTileCountsBuffer().read(np.uint32), ref["counts"], what + ("counts",))
    assert_same(binner.getTileOffsetsBuffer().read(np.uint32)[:ntx * nty], ref["offsets"][:ntx * nty], what + ("offsets",))
    assert_same(binner.getTileIndicesBuffer().read(np.uint32, total), ref["indices"], what + ("lists",), offsets=ref["offsets"])


def oracle_disc_lists(props, normals, u, w, h, tile):
    proj, discs = O.project_disc(u, props, normals)
    keys, pay = O.extract_keys(proj)
    _, order = O.sort_pairs(keys, pay)
    counts, offsets, idx = O.bin_sorted(proj, order, w, h, tile)
    return dict(proj=proj, discs=discs, counts=counts, offsets=offsets, indices=idx)


@pytest.mark.parametrize("tile,w,h,n,rs", SCREENS)
def test_lit_whole_frames(device, tile, w, h, n, rs):
    """splat_render_frame and splat_render_frame_planes with SPLAT_RECORDS_LIT32 (Renderer(records="lit-always")), in both binner
    orders: the oracle's counts, offsets and lists; the rgba32f image of records="projected" bit for bit; the oracle's image
    within the composite's tolerance.  records="lit" still falls back to ProjectedSplat records on these screens."""
    ntx, nty = cdiv(w, tile), cdiv(h, tile)
    assert ntx > 256 or nty > 256
    props, normals, u = make_case(n, w, h, 17, rs)
    ref = oracle_pipeline(props, normals, u, w, h, tile=tile)
    assert ref["indices"].shape[0] > 0
    want, want8, _, _, near = O.composite(O.MODE_FRONT_TO_BACK, True, props[:, 4:], normals, ref["proj"], ref["indices"],
                                          ref["counts"], ref["offsets"], w, h, tile=tile, want_stops=True)
    pm = sr.SplatPropertyManager(device, n)
    pm.setFromArrays(props)
    nbuf = device.createBufferFrom(normals)
    base = sr.Renderer(device, None, "rgba8unorm", n, tile, records="projected")
    base.render(u, pm.getPropertyBuffer(), nbuf, None, w, h, wantFloat=True)
    projected = base.readPixelsFloat().view(np.uint32).copy()
    assert base.frameRecordFormat == _lib.RECORDS_PROJECTED
    base.destroy()
    for order in ("tileFirst", "sortFirst"):
        for layout in ("interleaved", "planes"):
            what = (tile, w, h, order, layout)
            r = sr.Renderer(device, None, "rgba8unorm", n, tile, frameOrder=order, records="lit-always")
            src = pm.getPropertyBuffer() if layout == "interleaved" else pm.getPropertyPlanes()
            r.render(u, src, nbuf, None, w, h, wantFloat=True)
            assert r.frameRecordFormat == _lib.RECORDS_LIT32 and r.recordFormat == _lib.RECORDS_LIT32, what
            assert r.projector.contents == "lit", what
            check_lists(r.binner, ref, ntx, nty, what)
            got, got8 = r.readPixelsFloat().copy(), r.readPixels().copy()
            assert_same(got.view(np.uint32), projected, what + ("image of records='projected'",))
            check_image_against_oracle(got, got8, want, want8, near)
            r.destroy()
    # the default records="lit" keeps its fallback
    r = sr.Renderer(device, None, "rgba8unorm", n, tile)
    r.render(u, pm.getPropertyBuffer(), nbuf, None, w, h)
    assert r.frameRecordFormat == _lib.RECORDS_PROJECTED and r.projector.contents == "projected"
    r.destroy()
    pm.destroy()
    nbuf.destroy()


def test_lit_always_is_lit_on_small_screens(device):
    """At or below 256 x 256 tiles records="lit-always" is records="lit": the same format, lists and image bits."""
    tile, w, h, n = 8, 2048, 1024, 20000
    props, normals, u = make_case(n, w, h, 17, 1.0)
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    images = {}
    for records in ("lit", "lit-always"):
        r = sr.Renderer(device, None, "rgba8unorm", n, tile, records=records)
        r.render(u, pbuf, nbuf, None, w, h, wantFloat=True)
        assert r.frameRecordFormat == _lib.RECORDS_LIT32
        images[records] = r.readPixelsFloat().view(np.uint32).copy()
        r.destroy()
    assert_same(images["lit-always"], images["lit"], "lit-always vs lit at 256 x 128 tiles")
    with pytest.raises(sr.SplatError):
        sr.Renderer(device, None, "rgba8unorm", n, tile, records="always")
    pbuf.destroy()
    nbuf.destroy()


@pytest.mark.parametrize("order", ["tileFirst", "sortFirst"])
@pytest.mark.parametrize("tile,w,h,n,rs", DISC_SCREENS)
def test_disc_frames_without_projected_records(device, tile, w, h, n, rs, order):
    """footprint="disc" with writeProjected=False, with plain and with lit disc records: the oracle's lists, the image of the
    disc frame that writes its ProjectedSplat records bit for bit, and a zeroed ProjectedSplat buffer that stays zero."""
    ntx, nty = cdiv(w, tile), cdiv(h, tile)
    props, normals, u = make_case(n, w, h, 23, rs)
    ref = oracle_disc_lists(props, normals, u, w, h, tile)
    assert ref["indices"].shape[0] > 0
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    full = sr.Renderer(device, None, "rgba8unorm", n, tile, frameOrder=order, footprint="disc", records="projected")
    full.render(u, pbuf, nbuf, None, w, h, wantFloat=True)
    check_lists(full.binner, ref, ntx, nty, (tile, w, h, order, "disc writeProjected"))
    want = full.readPixelsFloat().view(np.uint32).copy()
    full.destroy()
    for records in ("projected", "lit-always"):
        what = (tile, w, h, order, "disc", records)
        r = sr.Renderer(device, None, "rgba8unorm", n, tile, frameOrder=order, footprint="disc", writeProjected=False, records=records)
        r.projector.getProjectedBuffer().zero()
        for _ in range(2):  # the second one is a sync-free frame
            r.render(u, pbuf, nbuf, None, w, h, wantFloat=True)
        assert r.frameRecordFormat == (_lib.RECORDS_LIT32 if records == "lit-always" else _lib.RECORDS_PROJECTED), what
        assert r.recordFormat == _lib.RECORDS_PROJECTED, what  # (a disc frame's lit records live inside the binner)
        check_lists(r.binner, ref, ntx, nty, what)
        assert_same(r.readPixelsFloat().view(np.uint32), want, what + ("image",))
        assert not r.projector.getProjectedBuffer().read(np.uint32).any(), what
        r.destroy()
    pbuf.destroy()
    nbuf.destroy()


@pytest.mark.parametrize("footprint", ["isotropic", "disc"])
def test_sync_free_frames_and_overflow(device, footprint):
    """Three frames, then a denser one that outgrows the sync-free pair limit sized from them: every frame has its own
    oracle's lists, and the overflow is detected (previousFrameOverflowed) and the frame rendered again."""
    tile, w, h, n = 8, 2049, 1024, 20000
    small, normals, u = make_case(n, w, h, 61, 0.5)
    big = small.copy()
    big[:, 3] *= 2.0
    if footprint == "disc":
        ref_s, ref_b = oracle_disc_lists(small, normals, u, w, h, tile), oracle_disc_lists(big, normals, u, w, h, tile)
        kw = dict(footprint="disc", writeProjected=False)
    else:
        ref_s, ref_b = oracle_pipeline(small, normals, u, w, h, tile=tile), oracle_pipeline(big, normals, u, w, h, tile=tile)
        kw = {}
    assert ref_b["indices"].shape[0] > 2 * ref_s["indices"].shape[0]
    ntx, nty = cdiv(w, tile), cdiv(h, tile)
    sbuf, bbuf, nbuf = device.createBufferFrom(small), device.createBufferFrom(big), device.createBufferFrom(normals)
    r = sr.Renderer(device, None, "rgba8unorm", n, tile, records="lit-always", **kw)
    first = None
    for k in range(3):
        r.render(u, sbuf, nbuf, None, w, h, wantFloat=True)
        check_lists(r.binner, ref_s, ntx, nty, (footprint, "frame", k))
        img = r.readPixelsFloat().view(np.uint32).copy()
        if first is None:
            first = img
        assert_same(img, first, (footprint, "frame", k, "image"))
    assert not r.previousFrameOverflowed
    r.render(u, bbuf, nbuf, None, w, h, wantFloat=True)  # outgrows the sync-free limit
    r.readPixelsFloat()  # finish(): detects, renders again
    if os.environ.get("SPLAT_BIN_SYNC") != "1":
        assert r.previousFrameOverflowed
    check_lists(r.binner, ref_b, ntx, nty, (footprint, "overflowed frame"))
    for o in (r, sbuf, bbuf, nbuf):
        o.destroy()


@pytest.mark.parametrize("tile,w,h,n,rs", [SCREENS[0], SCREENS[1], SCREENS[3]])
def test_strict_lit_bands_stitch_to_the_whole_frame(device, tile, w, h, n, rs):
    """splat_render_frame with strict tile-row bands and SPLAT_RECORDS_LIT32: the bands' pixel rows are the whole frame's bits."""
    nty = cdiv(h, tile)
    props, normals, u = make_case(n, w, h, 17, rs)
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    r = sr.Renderer(device, None, "rgba8unorm", n, tile, records="lit-always")
    r.render(u, pbuf, nbuf, None, w, h, wantFloat=True)
    whole = r.readPixelsFloat().view(np.uint32).copy()
    got = np.zeros_like(whole)
    cuts = [0, 1, nty // 3, nty // 2 + 1, nty]
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        r.render(u, pbuf, nbuf, None, w, h, tileRows=(r0, r1), wantFloat=True)
        assert r.frameRecordFormat == _lib.RECORDS_LIT32
        band = r.readPixelsFloat().view(np.uint32)
        got[r0 * tile:min(r1 * tile, h)] = band[r0 * tile:min(r1 * tile, h)]
    assert_same(got, whole, (tile, w, h, "strict lit bands"))
    for o in (r, pbuf, nbuf):
        o.destroy()


def run_band_frame(device, sorter, binner, cfg, props_ptr, normals_ptr, records_ptr, n, w, h, out8, out32):
    """splat_band_frame, settled (as dist.HipStages.band_frame(settle=True))."""
    lib, ctx = device.lib, device.ctx
    args = (ctx, sorter._s, binner._b, C.byref(cfg), props_ptr, normals_ptr, records_ptr, n, w, h, out8.ptr, out32.ptr, None)
    rc = lib.splat_band_frame(*args)
    if rc in _lib.RENDER_AGAIN:
        rc = lib.splat_band_frame(*args)
    _lib.check(rc, ctx)
    t, k = C.c_uint64(), C.c_uint32()
    for _ in range(4):
        rc = lib.splat_band_settle(ctx, sorter._s, binner._b, C.byref(k), C.byref(t))
        if rc not in _lib.RENDER_AGAIN:
            break
        _lib.check(lib.splat_band_frame(*args), ctx)
    _lib.check(rc, ctx)


@pytest.mark.parametrize("order", ["tileFirst", "sortFirst"])
@pytest.mark.parametrize("fmt", ["projected", "compact", "disc48"])
@pytest.mark.parametrize("tile,w,h,n,rs", [SCREENS[0], SCREENS[1], SCREENS[3]])
def test_band_frames_stitch_to_the_whole_frame(device, tile, w, h, n, rs, fmt, order):
    """splat_band_frame over gathered ProjectedSplat, 16-byte and 48-byte oriented-disc records, on one rank and on three
    virtual ranks: the stitched rgba8 and rgba32f images are the whole frame's bits (the disc whole frame's for DISC48)."""
    nty = cdiv(h, tile)
    disc = fmt == "disc48"
    props, normals, u = make_case(n, w, h, 41, rs)
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    full = sr.Renderer(device, None, "rgba8unorm", n, tile, footprint="disc" if disc else "isotropic", records="projected")
    full.render(u, pbuf, nbuf, None, w, h, wantFloat=True)
    want32 = full.readPixelsFloat().view(np.uint32).copy()
    want8 = full.readPixels().copy()
    lib, ctx = device.lib, device.ctx
    uf = np.ascontiguousarray(u, np.float32)
    up = uf.ctypes.data_as(C.POINTER(C.c_float))
    if fmt == "projected":
        records, rf = full.projector.getProjectedBuffer(), _lib.RECORDS_PROJECTED
    elif fmt == "compact":
        records, rf = device.createBuffer(n * 16), _lib.RECORDS_COMPACT
        _lib.check(lib.splat_project_slice_compact(ctx, up, pbuf.ptr, 2, 0, n, records.ptr), ctx)
    else:
        records, rf = device.createBuffer(n * 48), _lib.RECORDS_DISC48
        _lib.check(lib.splat_project_slice_disc(ctx, up, pbuf.ptr, 2, nbuf.ptr, 1, 0, n, records.ptr), ctx)
    sorter, binner = sr.RadixSorter(device, n), sr.GPUTileBinner(device, tile)
    binner.setFrameOrder(order)
    out8, out32 = device.createBuffer(w * h * 4), device.createBuffer(w * h * 16)
    for world in (1, 3):
        got8, got32 = np.zeros_like(want8), np.zeros_like(want32)
        for rank in range(world):
            r0, r1 = nty * rank // world, nty * (rank + 1) // world
            cfg = _lib.CompositeCfg(_lib.MODE_FRONT_TO_BACK, 1, tile, r0, r1, rf, 0,
                                    _lib.FOOTPRINT_DISC if disc else _lib.FOOTPRINT_ISOTROPIC)
            run_band_frame(device, sorter, binner, cfg, pbuf.ptr, nbuf.ptr, records.ptr, n, w, h, out8, out32)
            p0, p1 = r0 * tile, min(r1 * tile, h)
            got8[p0:p1] = out8.read(np.uint8).reshape(h, w, 4)[p0:p1]
            got32[p0:p1] = out32.read(np.uint32).reshape(h, w, 4)[p0:p1]
        assert_same(got8, want8, (tile, w, h, fmt, order, world, "rgba8"))
        assert_same(got32, want32, (tile, w, h, fmt, order, world, "rgba32f"))
    for o in (out8, out32, sorter, binner, full, pbuf, nbuf):
        o.destroy()
    if fmt != "projected":
        records.destroy()


def test_disc_hip_stages_band_renderer_at_T8(device):
    """dist.HipStages(footprint="disc") with dist.BandRenderer at T = 8 on 2049 x 1024 (257 x 128 tiles), virtual ranks: the
    stitched image is the single-GPU disc frame's bit for bit."""
    import torch
    from splat_renderer_amd import dist
    tile, n, w, h, world = 8, 30001, 2049, 1024, 3
    props, normals, u = make_case(n, w, h, 41, 1.0)
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    full = sr.Renderer(device, None, "rgba8unorm", n, tile, footprint="disc")
    full.render(u, pbuf, nbuf, None, w, h)
    want = full.readPixels().copy()
    device.sync()
    pt, nt = torch.from_numpy(props).cuda(), torch.from_numpy(normals).cuda()
    per = dist.shard_size(n, world)
    stages = dist.HipStages(torch, 0, per * world, w, h, tile=tile, footprint="disc")
    renderers = [dist.BandRenderer(stages, n, w, h, r, world, None, tile=tile) for r in range(world)]
    for br in renderers:
        stages.project_slice(u, pt.data_ptr(), br.first, br.count, br.shard, nt.data_ptr())
    gathered = torch.cat([br.shard for br in renderers], dim=0).contiguous()
    got = np.zeros_like(want)
    for br in renderers:
        # (settled: the virtual ranks share one binner, and a rank's band may outgrow the limits sized from the rank before it)
        for _ in range(2):  # the second one is sized from the first
            stages.band_frame(gathered, per * world, pt.data_ptr(), nt.data_ptr(), br.row0, br.row1, br.image, settle=True)
        torch.cuda.synchronize()
        r0, r1 = br.pixel_rows()
        got[r0:r1] = br.image.cpu().numpy()[r0:r1]
    assert_same(got, want, "HipStages disc bands at T=8, 2049x1024")
    stages.destroy()
    for o in (full, pbuf, nbuf):
        o.destroy()


NAPI = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "splat_renderer_amd", "napi")
NAPI_FRAME = r"""
const fs = require('fs');
const sr = require('./index.js');
const [propsPath, normalsPath, uPath, n, W, H, T, outPath] = process.argv.slice(1);
const f32 = (p) => { const b = fs.readFileSync(p); return new Float32Array(b.buffer, b.byteOffset, b.length / 4); };
const device = new sr.Device(0);
const props = device.createBufferFrom(f32(propsPath)), normals = device.createBufferFrom(f32(normalsPath));
const r = new sr.Renderer(device, null, 'rgba8unorm', +n, +T, { records: 'lit-always' });
r.render(f32(uPath), props, normals, null, +W, +H);
fs.writeFileSync(outPath, Buffer.from(r.readPixels().buffer));
console.log(JSON.stringify({ recordFormat: r.recordFormat, contents: r.projector.contents, pairs: r.binner.getTotalIndices() }));
r.destroy();
device.destroy();
"""


@pytest.mark.skipif(not os.path.exists("/usr/include/node/node_api.h") or not os.path.exists(os.path.join(NAPI, "index.js")),
                    reason="node / N-API headers not present")
def test_napi_lit_always_frame(device, tmp_path):
    """The N-API Renderer with records 'lit-always' at T = 4 on 1920 x 1080 (480 x 270 tiles): lit records, and the Python
    frame's image bytes."""
    import shutil
    node = shutil.which("node")
    if node is None:
        pytest.skip("node not present")
    tile, n, w, h = 4, 20000, 1920, 1080
    props, normals, u = make_case(n, w, h, 17, 0.6)
    ref = oracle_pipeline(props, normals, u, w, h, tile=tile)
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    r = sr.Renderer(device, None, "rgba8unorm", n, tile, records="lit-always")
    r.render(u, pbuf, nbuf, None, w, h)
    want = r.readPixels().copy()
    for o in (r, pbuf, nbuf):
        o.destroy()
    device.sync()
    props.tofile(tmp_path / "props.f32")
    normals.tofile(tmp_path / "normals.f32")
    np.ascontiguousarray(u, np.float32).tofile(tmp_path / "u.f32")
    p = subprocess.run([node, "-e", NAPI_FRAME, str(tmp_path / "props.f32"), str(tmp_path / "normals.f32"), str(tmp_path / "u.f32"),
                        str(n), str(w), str(h), str(tile), str(tmp_path / "frame.rgba8")], cwd=NAPI, capture_output=True, text=True,
                       timeout=300)
    assert p.returncode == 0, p.stderr
    info = json.loads(p.stdout.strip().splitlines()[-1])
    assert info["recordFormat"] == _lib.RECORDS_LIT32 and info["contents"] == "lit"
    assert info["pairs"] == ref["indices"].shape[0]
    assert_same(np.fromfile(tmp_path / "frame.rgba8", np.uint8).reshape(h, w, 4), want, "N-API lit-always frame")
