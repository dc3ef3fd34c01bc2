#!/usr/bin/env python3
"""The strict bands of tests/test_gpu_band_dispatch.py in a process of their own, for a ranking policy of its own: SPLAT_RANK is
read once per context, and test_compacted_scatter_with_ballot_ranking holds what this prints to its own process's bits.
strict_bands() is what that file's in-process tests call too.

    SPLAT_RANK=ballot python tests/band_dispatch_child.py
"""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import splat_renderer_amd as sr  # noqa: E402
from tests.helpers import assert_same, make_case  # noqa: E402

TILE, W, H, N, SEED = 16, 80, 80, 5000, 41
BANDS = [(0, 2), (2, 5)]


def whole_frame(device, pbuf, nbuf, u, disc):
    """The whole frame (records="projected"): its renderer, rgba8 and rgba32f bits."""
    full = sr.Renderer(device, None, "rgba8unorm", N, TILE, footprint="disc" if disc else "isotropic", records="projected")
    full.render(u, pbuf, nbuf, None, W, H, wantFloat=True)
    want32, want8 = full.readPixelsFloat().view(np.uint32).copy(), full.readPixels().copy()
    assert full.finish() > 0 and len(np.unique(want8.reshape(-1, 4), axis=0)) > 1  # (splats in the picture)
    return full, want8, want32


def strict_bands(device, case, records, footprint, order):
    """The two strict bands stitched, held to the whole frame's bits; returns them (rgba8, rgba32f as uint32)."""
    props, normals, u = case
    pbuf, nbuf = device.createBufferFrom(props), device.createBufferFrom(normals)
    full, want8, want32 = whole_frame(device, pbuf, nbuf, u, footprint == "disc")
    r = sr.Renderer(device, None, "rgba8unorm", N, TILE, frameOrder=order, footprint=footprint, records=records)
    got8, got32 = np.zeros_like(want8), np.zeros_like(want32)
    for r0, r1 in BANDS:
        r.render(u, pbuf, nbuf, None, W, H, tileRows=(r0, r1), wantFloat=True)
        p0, p1 = r0 * TILE, min(r1 * TILE, H)
        got32[p0:p1] = r.readPixelsFloat().view(np.uint32)[p0:p1]
        got8[p0:p1] = r.readPixels()[p0:p1]
    assert_same(got8, want8, ("strict bands", records, footprint, order, "rgba8"))
    assert_same(got32, want32, ("strict bands", records, footprint, order, "rgba32f"))
    for o in (r, full, pbuf, nbuf):
        o.destroy()
    return got8, got32


def compacted_scatter_digests(device, case):
    """sha256 of the stitched tile-first strict bands, per record kind: the first band's projector leaves its kept splats
    compacted, so these frames launch k_tf_scatter<_, 4, COMPACTED> under the device's ranking policy."""
    return [hashlib.sha256(b"".join(a.tobytes() for a in strict_bands(device, case, records, "isotropic", "tileFirst"))).hexdigest()
            for records in ("lit", "projected")]


def main():
    dev = sr.Device(0)
    try:
        policy = dev.rankStatus()["policy"]
        assert policy == (os.environ.get("SPLAT_RANK") or "checked"), policy
        print(f"band_dispatch_child ok: rank={policy} " + " ".join(compacted_scatter_digests(dev, make_case(N, W, H, SEED))))
    finally:
        dev.destroy()


if __name__ == "__main__":
    main()
