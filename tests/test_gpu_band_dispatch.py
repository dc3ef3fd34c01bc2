"""GPU cell walk of the band paths on a screen of at most 256 x 256 tiles.

The band-frame walk in test_gpu_wide_screens.py uses screens beyond 256 x 256 tiles only, where a band frame bins sort-first
from the 8-byte range.  Here the screen is 80 x 80 with 16-pixel tiles (5 x 5 tiles) and 5000 splats — two compaction groups
of 4096 records, five 1024-splat blocks — cut into the bands of tile rows [0, 2) and [2, 5): by the rule 5 * rows <= 2 * nty
the first band takes the compacting prepare pass (k_band_prepare_tfc; the whole-frame projector's k_project_hist_bandc) and the
second the plain one (k_band_prepare_tf; k_project_hist_band), for every record format and both frame orders.  Every cell is
held to the bits of the same library's whole frame, which the other tests hold to the oracle.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import splat_renderer_amd as sr
from splat_renderer_amd import _lib
from tests.band_dispatch_child import BANDS, H, N, SEED, TILE, W, compacted_scatter_digests, strict_bands, whole_frame
from tests.helpers import assert_same, make_case
from tests.test_gpu_wide_screens import run_band_frame

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif("SPLAT_BAND_COMPACT" in os.environ, reason="SPLAT_BAND_COMPACT forces one prepare pass for every band")]

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def case():
    assert -(-H // TILE) == 5 and 5 * (BANDS[0][1] - BANDS[0][0]) <= 2 * 5 < 5 * (BANDS[1][1] - BANDS[1][0])
    return make_case(N, W, H, SEED)


@pytest.mark.parametrize("order", ["tileFirst", "sortFirst"])
@pytest.mark.parametrize("fmt", ["projected", "compact", "disc48"])
def test_band_frames_stitch_to_the_whole_frame(device, case, fmt, order):
    """splat_band_frame over gathered ProjectedSplat, 16-byte and 48-byte oriented-disc records: the two bands' rgba8 and rgba32f
    rows are the whole frame's bit for bit.  (Oriented-disc records have no sort-first band frame at or below 256 x 256 tiles:
    that cell is the refusal.)"""
    props, normals, u = case
    disc = fmt == "disc48"
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    full, want8, want32 = whole_frame(device, pbuf, nbuf, u, disc)
    lib, ctx = device.lib, device.ctx
    up = np.ascontiguousarray(u, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    if fmt == "projected":
        records, rf = full.projector.getProjectedBuffer(), _lib.RECORDS_PROJECTED
    elif fmt == "compact":
        records, rf = device.createBuffer(N * 16), _lib.RECORDS_COMPACT
        _lib.check(lib.splat_project_slice_compact(ctx, up, pbuf.ptr, 2, 0, N, records.ptr), ctx)
    else:
        records, rf = device.createBuffer(N * 48), _lib.RECORDS_DISC48
        _lib.check(lib.splat_project_slice_disc(ctx, up, pbuf.ptr, 2, nbuf.ptr, 1, 0, N, records.ptr), ctx)
    sorter, binner = sr.RadixSorter(device, N), sr.GPUTileBinner(device, TILE)
    binner.setFrameOrder(order)
    out8, out32 = device.createBuffer(W * H * 4), device.createBuffer(W * H * 16)
    got8, got32 = np.zeros_like(want8), np.zeros_like(want32)
    for r0, r1 in BANDS:
        cfg = _lib.CompositeCfg(_lib.MODE_FRONT_TO_BACK, 1, TILE, r0, r1, rf, 0, _lib.FOOTPRINT_DISC if disc else _lib.FOOTPRINT_ISOTROPIC)
        if disc and order == "sortFirst":
            with pytest.raises(sr.SplatError):
                run_band_frame(device, sorter, binner, cfg, pbuf.ptr, nbuf.ptr, records.ptr, N, W, H, out8, out32)
            continue
        run_band_frame(device, sorter, binner, cfg, pbuf.ptr, nbuf.ptr, records.ptr, N, W, H, out8, out32)
        p0, p1 = r0 * TILE, min(r1 * TILE, H)
        got8[p0:p1] = out8.read(np.uint8).reshape(H, W, 4)[p0:p1]
        got32[p0:p1] = out32.read(np.uint32).reshape(H, W, 4)[p0:p1]
    if not (disc and order == "sortFirst"):
        assert_same(got8, want8, ("band dispatch", fmt, order, "rgba8"))
        assert_same(got32, want32, ("band dispatch", fmt, order, "rgba32f"))
    for o in (out8, out32, sorter, binner, full, pbuf, nbuf):
        o.destroy()
    if fmt != "projected":
        records.destroy()


@pytest.mark.parametrize("order", ["tileFirst", "sortFirst"])
@pytest.mark.parametrize("footprint", ["isotropic", "disc"])
@pytest.mark.parametrize("records", ["lit", "projected"])
def test_strict_bands_stitch_to_the_whole_frame(device, case, records, footprint, order):
    """splat_render_frame's own strict bands (Renderer.render(tileRows=...)): the first band's projector leaves its splats
    compacted per group of 4096 in the tile-first order, the second's does not; both bands' rows are the whole frame's bits."""
    strict_bands(device, case, records, footprint, order)




def test_compacted_scatter_with_ballot_ranking(device, case):
    """SPLAT_RANK=ballot (a child process, tests/band_dispatch_child.py: the policy is read once per context) gives the bits this
    process's policy gives: the compacted scatter's ballot-ranking kernel, which no other test launches."""
    env = dict(os.environ, SPLAT_RANK="ballot")
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "band_dispatch_child.py")], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True, timeout=300)
    line = "band_dispatch_child ok: rank=ballot " + " ".join(compacted_scatter_digests(device, case))
    assert p.returncode == 0 and line in p.stdout.splitlines(), p.stdout[-2000:] + p.stderr[-3000:]
