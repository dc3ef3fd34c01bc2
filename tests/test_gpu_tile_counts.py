"""GPU tests over the binner's tile-count regimes, at tile sizes other than 16.

The number of tiles on a screen picks the binner's code path: up to 256 tiles a side a frame bins tile-first (one pass over
the records per tile-id digit, then a per-tile depth sort), beyond that sort-first (global depth sort, then a radix sort of
the tile ids).  The width of the tile ids picks the passes: one for up to 8 bits, two tile-first passes with a 7- or 8-bit high
digit for 9 to 16 bits, and from 17 bits on three or more sort-first passes whose first digit is at most 8 bits wide.  Each
case below lands in one regime on purpose (its id names it); every case holds the whole frame, in both orders of work, and the
staged GPUTileBinner to O.bin_sorted's counts, offsets and lists bit for bit, and the image to the oracle's.

Also here: sync-free frames, overflow recovery, entry counting and band counters at tile sizes other than 16.
"""
import ctypes as C
import os

import numpy as np
import pytest

import splat_renderer_amd as sr
from oracle import oracle as O
from splat_renderer_amd import _lib
from tests.helpers import assert_same, make_case, oracle_pipeline
from tests.test_gpu_stages import check_image_against_oracle, destroy_all, run_gpu_pipeline

pytestmark = pytest.mark.gpu


def cdiv(a, b):
    return -(-a // b)


def id_bits(tiles):
    """The binner's tile-id width (common.h: tile_id_bits)."""
    b = 1
    while (1 << b) < tiles:
        b += 1
    return b


# (tile, width, height, splats, radius scale, tile-id bits, tile-first): scenes of at most about 10 M pairs (seed 17)
MATRIX = [
    pytest.param(40, 600, 400, 20000, 1.0, 8, True, id="8bit-one-pass-T40-600x400"),
    pytest.param(12, 1280, 1080, 20000, 1.0, 14, True, id="14bit-tile-first-hi7-T12-1280x1080"),
    pytest.param(5, 1280, 1280, 20000, 0.6, 16, True, id="16bit-tile-first-hi8-256x256-tiles-T5-1280x1280"),
    pytest.param(8, 2048, 1024, 20000, 1.0, 15, True, id="fast-edge-256-tiles-wide-T8-2048x1024"),
    pytest.param(8, 2049, 1024, 20000, 1.0, 16, False, id="fast-edge-257-tiles-wide-T8-2049x1024"),
    pytest.param(4, 1920, 1080, 20000, 0.6, 17, False, id="17bit-T4-1920x1080"),
    pytest.param(3, 1920, 1080, 20000, 0.5, 18, False, id="18bit-T3-1920x1080"),
    pytest.param(7, 3840, 2160, 20000, 0.5, 18, False, id="18bit-T7-3840x2160"),
    pytest.param(2, 1920, 1080, 20000, 0.3, 19, False, id="19bit-T2-1920x1080"),
    pytest.param(1, 1920, 1080, 20000, 0.1, 21, False, id="21bit-T1-1920x1080"),
    pytest.param(1, 4096, 4096, 4000, 0.04, 24, False, id="24bit-16M-tiles-T1-4096x4096"),
    # windows (16 x 16 pixels, ceil(T/16)^2 per tile) clipped at the tile and at the screen
    pytest.param(17, 333, 211, 20000, 1.5, 9, True, id="windows-T17-333x211"),
    pytest.param(33, 333, 211, 20000, 1.5, 7, True, id="windows-T33-333x211"),
    pytest.param(100, 333, 211, 20000, 1.5, 4, True, id="windows-T100-333x211"),
    pytest.param(4096, 333, 211, 20000, 1.5, 1, True, id="windows-T4096-333x211"),
] + [
    pytest.param(tile, w, h, 2000, 1.0, id_bits(cdiv(w, tile) * cdiv(h, tile)), cdiv(w, tile) <= 256 and cdiv(h, tile) <= 256,
                 id=f"degenerate-T{tile}-{w}x{h}")
    for tile in (1, 16, 17) for w, h in ((1, 1), (1, 333), (333, 1))
]


@pytest.mark.parametrize("tile,w,h,n,rs,bits,tile_first", MATRIX)
def test_tile_count_regime(device, tile, w, h, n, rs, bits, tile_first):
    """Renderer(..., tileSize=T) in both orders of work and the staged GPUTileBinner.binSplats: counts, offsets and lists
    O.bin_sorted's at T; the image the oracle's, and the same bits in both orders.  (2^24 tiles: lists and the orders' rgba8
    images only.)"""
    ntx, nty = cdiv(w, tile), cdiv(h, tile)
    assert id_bits(ntx * nty) == bits and (ntx <= 256 and nty <= 256) == tile_first, "the case left its regime"
    image = ntx * nty < (1 << 24)
    props, normals, u = make_case(n, w, h, 17, rs)
    ref = oracle_pipeline(props, normals, u, w, h, tile=tile)
    total = ref["indices"].shape[0]
    assert total > 0
    if image:
        want, want8, _, _, near = O.composite(O.MODE_FRONT_TO_BACK, True, props[:, 4:], normals, ref["proj"], ref["indices"],
                                              ref["counts"], ref["offsets"], w, h, tile=tile, want_stops=True)
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    images = {}
    for order in ("tileFirst", "sortFirst"):
        what = (tile, w, h, order)
        r = sr.Renderer(device, None, "rgba8unorm", n, tile, frameOrder=order)
        r.render(u, pbuf, nbuf, None, w, h, wantFloat=image)
        assert r.finish() == total, what
        # beyond 256 x 256 tiles the frame composites from ProjectedSplat records (host.py), not lit ones
        assert r.frameRecordFormat == (_lib.RECORDS_LIT32 if tile_first else _lib.RECORDS_PROJECTED), what
        assert_same(r.binner.getTileCountsBuffer().read(np.uint32), ref["counts"], what + ("frame counts",))
        assert_same(r.binner.getTileOffsetsBuffer().read(np.uint32)[:ntx * nty], ref["offsets"][:ntx * nty], what + ("frame offsets",))
        assert_same(r.binner.getTileIndicesBuffer().read(np.uint32, total), ref["indices"], what + ("frame lists",),
                    offsets=ref["offsets"])
        got8 = r.readPixels().copy()
        if image:
            got = r.readPixelsFloat().copy()
            check_image_against_oracle(got, got8, want, want8, near)
            images[order] = got.view(np.uint32)
        else:
            images[order] = got8
        r.destroy()
    assert_same(images["tileFirst"], images["sortFirst"], (tile, w, h, "image of both orders"))
    pbuf.destroy()
    nbuf.destroy()
    g = run_gpu_pipeline(device, props, normals, u, n, w, h, tile=tile)
    b = g["binner"]
    assert b.getTotalIndices() == total
    assert_same(b.getTileCountsBuffer().read(np.uint32), ref["counts"], (tile, w, h, "staged counts"))
    assert_same(b.getTileOffsetsBuffer().read(np.uint32)[:ntx * nty], ref["offsets"][:ntx * nty], (tile, w, h, "staged offsets"))
    assert_same(b.getTileIndicesBuffer().read(np.uint32, total), ref["indices"], (tile, w, h, "staged lists"), offsets=ref["offsets"])
    destroy_all(g)


def test_more_than_2_24_tiles_is_an_argument_error(device):
    """4097 x 4096 tiles of one pixel are more than the binner's 2^24: binSplats refuses the screen with a host-side argument check
    (no launch), and the binner stays usable."""
    n = 64
    props, normals, u = make_case(n, 64, 64, 3)
    ref = oracle_pipeline(props, normals, u, 64, 64, tile=1)
    g = run_gpu_pipeline(device, props, normals, u, n, 64, 64, tile=1)
    b = g["binner"]
    with pytest.raises(sr.SplatError, match="argument check failed"):
        b.binSplats(None, g["proj"].getProjectedBuffer(), g["sorter"].getSortedIndicesBuffer(), n, 4097, 4096)
    # and the binner goes on: the 64 x 64 screen again gives the oracle's lists
    b.binSplats(None, g["proj"].getProjectedBuffer(), g["sorter"].getSortedIndicesBuffer(), n, 64, 64)
    assert b.getTotalIndices() == ref["indices"].shape[0] > 0
    assert_same(b.getTileCountsBuffer().read(np.uint32), ref["counts"], "T=1 64x64 counts after the refused screen")
    assert_same(b.getTileIndicesBuffer().read(np.uint32, ref["indices"].shape[0]), ref["indices"], "T=1 64x64 lists after the refused screen")
    destroy_all(g)


@pytest.mark.parametrize("order", ["tileFirst", "sortFirst"])
@pytest.mark.parametrize("tile", [8, 24])
def test_sync_free_repeat_and_overflow(device, tile, order):
    """tests/test_gpu_stages.py's sync-free repeat and overflow recovery at T = 8 and 24: frames 2..5 of a static scene are
    frame 1 bit for bit and the oracle's lists; a frame that outgrows its sync-free pair limit is detected at the next call and
    rendered again, with the oracle's lists and image.  (The frame report is written by k_composite_tile at these sizes.)"""
    n, w, h = 20000, 320, 200
    small, normals, u = make_case(n, w, h, 61, 0.5)
    big = small.copy()
    big[:, 3] *= 6.0
    ref_s, ref_b = oracle_pipeline(small, normals, u, w, h, tile=tile), oracle_pipeline(big, normals, u, w, h, tile=tile)
    assert ref_b["indices"].shape[0] > 3 * ref_s["indices"].shape[0]
    want, want8, _, _, near = O.composite(O.MODE_FRONT_TO_BACK, True, big[:, 4:], normals, ref_b["proj"], ref_b["indices"],
                                          ref_b["counts"], ref_b["offsets"], w, h, tile=tile, want_stops=True)
    sbuf, bbuf, nbuf = device.createBufferFrom(small), device.createBufferFrom(big), device.createBufferFrom(normals)
    r = sr.Renderer(device, None, "rgba8unorm", n, tile, frameOrder=order)
    r.render(u, sbuf, nbuf, None, w, h, wantFloat=True)
    first = r.readPixelsFloat().copy()
    for _ in range(4):
        r.render(u, sbuf, nbuf, None, w, h, wantFloat=True)  # sync-free
    assert not r.previousFrameOverflowed
    assert_same(r.readPixelsFloat().view(np.uint32), first.view(np.uint32), (tile, order, "sync-free repeat image"))
    assert r.binner.getTotalIndices() == ref_s["indices"].shape[0]
    assert_same(r.binner.getTileCountsBuffer().read(np.uint32), ref_s["counts"], (tile, order, "sync-free counts"))
    assert_same(r.binner.getTileIndicesBuffer().read(np.uint32, ref_s["indices"].shape[0]), ref_s["indices"],
                (tile, order, "sync-free lists"), offsets=ref_s["offsets"])
    r.render(u, bbuf, nbuf, None, w, h, wantFloat=True)  # outgrows the sync-free limit
    got, got8 = r.readPixelsFloat(), r.readPixels()     # finish(): detects, renders again
    if os.environ.get("SPLAT_BIN_SYNC") != "1":  # (with it every frame reads its total back first: none can overflow)
        assert r.previousFrameOverflowed
    assert r.binner.getTotalIndices() == ref_b["indices"].shape[0]
    assert_same(r.binner.getTileCountsBuffer().read(np.uint32), ref_b["counts"], (tile, order, "overflowed frame counts"))
    assert_same(r.binner.getTileIndicesBuffer().read(np.uint32, ref_b["indices"].shape[0]), ref_b["indices"],
                (tile, order, "overflowed frame lists"), offsets=ref_b["offsets"])
    check_image_against_oracle(got, got8, want, want8, near)
    for o in (r, sbuf, bbuf, nbuf):
        o.destroy()


def staged_consumed(device, g, u, w, h, tile, tile_rows_list):
    """Per-tile {staged, consumed} of the staged composite (ComputeShaderRenderer.consumedBuffer), rendered as the given
    tile-row bands into one zeroed counter buffer."""
    b = g["binner"]
    ntx, nty = cdiv(w, tile), cdiv(h, tile)
    r = sr.ComputeShaderRenderer(device, None, "rgba8unorm")
    r.consumedBuffer = device.createBuffer(ntx * nty * 16)
    r.consumedBuffer.zero()
    for rows in tile_rows_list:
        r.tileRows = rows
        r.render(u, g["pm"].getPropertyBuffer(), b.getTileIndicesBuffer(), g["nbuf"], g["proj"].getProjectedBuffer(),
                 b.getTileCountsBuffer(), b.getTileOffsetsBuffer(), tile, ntx, w, h)
    cons = r.consumedBuffer.read(np.uint64).reshape(ntx * nty, 2).copy()
    r.destroy()
    return cons


def test_frame_entry_counts_equal_the_staged_per_tile_counts_at_tile_24(device):
    """At T = 24, a whole frame's counted entries (splat_timing_consumed: staged, consumed) are the sums of the staged
    composite's per-tile consumedBuffer for the same lists, in both orders of work."""
    tile, n, w, h = 24, 20000, 333, 211
    props, normals, u = make_case(n, w, h, 17, 1.5)
    ref = oracle_pipeline(props, normals, u, w, h, tile=tile)
    g = run_gpu_pipeline(device, props, normals, u, n, w, h, tile=tile)
    assert_same(g["binner"].getTileIndicesBuffer().read(np.uint32, ref["indices"].shape[0]), ref["indices"], "staged lists T=24")
    cons = staged_consumed(device, g, u, w, h, tile, [(0, 0xFFFFFFFF)])
    want = (int(cons[:, 0].sum()), int(cons[:, 1].sum()))
    assert want[0] >= want[1] > 0
    destroy_all(g)
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    lib, ctx = device.lib, device.ctx
    try:
        for order in ("tileFirst", "sortFirst"):
            r = sr.Renderer(device, None, "rgba8unorm", n, tile, frameOrder=order)
            _lib.check(lib.splat_set_timing_stages(ctx, 0xFFFFFFFF), ctx)
            device.setTiming(True)
            r.render(u, pbuf, nbuf, None, w, h)
            assert r.finish() == ref["indices"].shape[0]
            staged, consumed = C.c_uint64(), C.c_uint64()
            _lib.check(lib.splat_timing_consumed(ctx, C.byref(staged), C.byref(consumed)), ctx)
            device.setTiming(False)
            assert (staged.value, consumed.value) == want, (order, staged.value, consumed.value, want)
            r.destroy()
    finally:
        device.setTiming(False)
        _lib.check(lib.splat_set_timing_stages(ctx, 0xFFFFFFFF), ctx)
        pbuf.destroy()
        nbuf.destroy()


@pytest.mark.parametrize("tile", [8, 24])
def test_band_counters_stitch(device, tile):
    """The staged composite's per-tile counters rendered as bands [0, k) + [k, nty) are the whole screen's, tile for tile (the
    band's tile-row offset in k_window_counts at T = 24, in k_composite_tile's own counting at T = 8)."""
    n, w, h = 20000, 333, 211
    props, normals, u = make_case(n, w, h, 17, 1.5)
    g = run_gpu_pipeline(device, props, normals, u, n, w, h, tile=tile)
    nty = cdiv(h, tile)
    whole = staged_consumed(device, g, u, w, h, tile, [(0, 0xFFFFFFFF)])
    assert whole[:, 1].sum() > 0
    for k in (1, nty // 2, nty - 1):
        bands = staged_consumed(device, g, u, w, h, tile, [(0, k), (k, nty)])
        assert_same(bands, whole, (tile, f"counters of bands [0,{k}) + [{k},{nty})"))
    destroy_all(g)
