"""Band frames of the adversarial band-edge scenes (tests/band_edge.py) against the oracle, list for list.

A tile-first frame of a strict band of tile rows (screens of at most 256 x 256 tiles) first rejects the splats that
cannot_reach_band (project.hip) proves cannot reach it; k_project_hist_bandc runs bands of at most 2/5 of the rows,
k_project_hist_band wider ones, each in four <DISC, LIT> variants.  A wrongly rejected splat is one whose padded box only
just reaches the band: its pixels are faint and rgba8 images rarely show it.  So every case here holds
- the band's tile counts to the oracle's whole-frame counts on the band's rows, and to zero elsewhere;
- the band's lists to the oracle's, bit for bit — a missing splat is named with its oracle bounds and the band edge;
- the band's FLOAT image rows to the whole frame's, bit for bit.
Sort-first frames and a screen beyond 256 tiles a side project every splat: they are controls that must give the same lists.
"""
import zlib

import numpy as np
import pytest

import splat_renderer_amd as sr
from oracle import oracle as O
from tests import band_edge as B
from tests.helpers import assert_same

pytestmark = pytest.mark.gpu


def oracle_lists(u, props, normals, w, h, tile, footprint):
    rec = B.records(u, props, normals, footprint)
    keys, pay = O.extract_keys(rec)
    _, order = O.sort_pairs(keys, pay)
    counts, offsets, idx = O.bin_sorted(rec, order, w, h, tile)
    return rec, counts, offsets, idx


def band_rows(kind, nty):
    """'narrow': at most 2/5 of the rows (k_project_hist_bandc); 'wide': more (k_project_hist_band); 'top' / 'bottom': a
    band touching row 0 / the last row."""
    if kind == "narrow":
        r0 = nty // 3
        return r0, r0 + max(1, (2 * nty) // 5 - 1)
    if kind == "wide":
        r0 = max(1, nty // 6)
        return r0, min(nty - 1, r0 + (3 * nty) // 5)
    if kind == "top":
        return 0, max(1, nty // 3)
    return nty - max(1, nty // 3), nty


def check_band(device, u, props, normals, w, h, tile, rows, footprint, records, order, what):
    n = props.shape[0]
    r0, r1 = rows
    ntx, nty = -(-w // tile), -(-h // tile)
    rec, counts, offsets, idx = oracle_lists(u, props, normals, w, h, tile, footprint)
    in_band = B.in_band(rec, w, h, tile, r0, r1)
    assert in_band.sum() >= 20, (what, "too few band splats to mean anything")
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    kw = dict(tileSize=tile, frameOrder=order, footprint=footprint, records=records)
    full = sr.Renderer(device, None, "rgba8unorm", n, **kw)
    full.render(u, pbuf, nbuf, None, w, h, wantFloat=True)
    whole = full.readPixelsFloat().view(np.uint32).copy()
    band = sr.Renderer(device, None, "rgba8unorm", n, **kw)
    band.render(u, pbuf, nbuf, None, w, h, tileRows=(r0, r1), wantFloat=True)
    total = band.finish()
    got_counts = band.binner.getTileCountsBuffer().read(np.uint32).reshape(nty, ntx)
    got_offsets = band.binner.getTileOffsetsBuffer().read(np.uint32).reshape(-1)
    got_idx = band.binner.getTileIndicesBuffer().read(np.uint32, total) if total else np.zeros(0, np.uint32)
    want_counts = counts.reshape(nty, ntx)
    lo = int(offsets[r0 * ntx])
    hi = int(offsets[r1 * ntx]) if r1 < nty else idx.shape[0]
    want_idx = idx[lo:hi]
    # every splat the oracle puts in a band tile must be in that tile's list: name the first one that is not
    got_band = np.concatenate([got_idx[int(got_offsets[t]):int(got_offsets[t]) + int(got_counts.reshape(-1)[t])]
                               for t in range(r0 * ntx, r1 * ntx)] + [np.zeros(0, np.uint32)])
    missing = np.setdiff1d(np.unique(want_idx), np.unique(got_band))
    if missing.size:
        i = int(missing[0])
        raise AssertionError(
            f"[{what}] {missing.size} splat(s) the oracle bins into tile rows [{r0}, {r1}) are missing from the band's lists; "
            f"first: #{i} pos/radius {props[i, :4].tolist()} normal {normals[i, :3].tolist()} oracle bounds {rec[i, :4].tolist()} "
            f"(band edges y = {r0 * tile}, {r1 * tile}; T={tile}, screen {w}x{h})")
    assert_same(got_counts[r0:r1], want_counts[r0:r1], (what, "band counts"))
    assert not got_counts[:r0].any() and not got_counts[r1:].any(), (what, "counts outside the band")
    assert total == want_idx.shape[0], (what, total, want_idx.shape[0])
    assert_same(got_band, want_idx, (what, "band lists"))
    y0, y1 = r0 * tile, min(r1 * tile, h)
    assert_same(band.readPixelsFloat().view(np.uint32)[y0:y1], whole[y0:y1], (what, "float rows"))
    for o in (full, band, pbuf, nbuf):
        o.destroy()
    return int(in_band.sum())


# (camera, aspect, tile, band, footprint, records, order)
CASES = []
for fp in ("isotropic", "disc"):
    for rec in ("lit", "projected"):
        for cam, aspect, tile, kind in (("axis", 1.0, 16, "narrow"), ("oblique", 1.0, 16, "wide"), ("high", 0.2, 24, "narrow"),
                                        ("low", 5.0, 24, "wide"), ("narrow", 1.6, 64, "top"), ("wide", 1.6, 16, "bottom"),
                                        ("axis_side", 2.0, 24, "top"), ("axis", 0.5, 64, "bottom")):
            CASES.append((cam, aspect, tile, kind, fp, rec, "tileFirst"))
# controls: the sort-first order projects every splat
CASES += [("axis", 1.0, 16, "narrow", fp, "lit", "sortFirst") for fp in ("isotropic", "disc")]
CASES += [("oblique", 0.2, 24, "wide", "disc", "projected", "sortFirst")]


@pytest.mark.parametrize("cam,aspect,tile,kind,footprint,records,order", CASES)
def test_band_edge_lists_are_the_oracles(device, cam, aspect, tile, kind, footprint, records, order):
    w, h = B.screen_for(aspect)
    u = B.make_camera(cam, w, h)
    nty = -(-h // tile)
    rows = band_rows(kind, nty)
    props, normals, _, _ = B.band_edge_scene(u, tile, rows[0], rows[1], footprint, seed=zlib.crc32(f"{cam}{tile}{kind}".encode()))
    check_band(device, u, props, normals, w, h, tile, rows, footprint, records, order,
               (cam, aspect, tile, kind, footprint, records, order))


@pytest.mark.parametrize("footprint", ["isotropic", "disc"])
def test_band_edge_lists_beyond_256_tiles(device, footprint):
    """Control: a screen of more than 256 tiles a side (the 8-byte range, sort-first) projects every splat."""
    w, h, tile = 1100, 240, 4
    u = B.make_camera("axis", w, h)
    nty = -(-h // tile)
    rows = (nty // 3, nty // 3 + 10)
    props, normals, _, _ = B.band_edge_scene(u, tile, rows[0], rows[1], footprint, seed=5)
    check_band(device, u, props, normals, w, h, tile, rows, footprint, "lit", "default", ("wide screen", footprint))


@pytest.mark.parametrize("footprint", ["isotropic", "disc"])
def test_local_band_renderer_on_band_edge_scene(device, footprint):
    """dist.LocalBandRenderer (the exchange-free multi-GPU cut bench.py runs): every rank of three renders its band from all
    splats of an adversarial scene aimed at the ranks' boundaries; the stitched image is the whole frame's, and each rank's
    lists are the oracle's."""
    import torch
    from splat_renderer_amd import dist
    world, w, h, tile = 3, 320, 240, dist.TILE
    u = B.make_camera("axis", w, h)
    nty = -(-h // tile)
    parts = [B.band_edge_scene(u, tile, *dist.band_rows(nty, r, world), footprint, seed=r) for r in range(world)]
    props = np.concatenate([p[0] for p in parts])
    normals = np.concatenate([p[1] for p in parts])
    n = props.shape[0]
    rec, counts, offsets, idx = oracle_lists(u, props, normals, w, h, tile, footprint)
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    full = sr.Renderer(device, None, "rgba8unorm", n, footprint=footprint)
    full.render(u, pbuf, nbuf, None, w, h)
    want = full.readPixels().copy()
    pt, nt = torch.from_numpy(props).cuda(), torch.from_numpy(normals).cuda()
    stages = dist.HipStages(torch, 0, n, w, h, footprint=footprint)
    view = sr.GPUTileBinner.__new__(sr.GPUTileBinner)  # the stages' binner, read through the test context's buffers
    view.device, view.tileSize, view._b, view._tiles = device, tile, stages.binner, nty * -(-w // tile)
    got = np.zeros_like(want)
    for rank in range(world):
        lr = dist.LocalBandRenderer(stages, n, w, h, rank, world)
        lr.render(u, pt.data_ptr(), nt.data_ptr(), settle=True)
        torch.cuda.synchronize()
        y0, y1 = lr.pixel_rows()
        got[y0:y1] = lr.image.cpu().numpy()[y0:y1]
        ntx = -(-w // tile)
        lo, hi = int(offsets[lr.row0 * ntx]), int(offsets[lr.row1 * ntx]) if lr.row1 < nty else idx.shape[0]
        assert_same(view.getTileIndicesBuffer().read(np.uint32, stages.pairs), idx[lo:hi], ("local band lists", footprint, rank))
    assert_same(got, want, ("local bands", footprint))
    stages.destroy()
    for o in (full, pbuf, nbuf):
        o.destroy()
