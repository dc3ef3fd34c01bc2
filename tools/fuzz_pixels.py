#!/usr/bin/env python3
"""Differential sweep of whole frames against the oracle's composite: random scenes, screens, tile sizes (a quarter of
the cases at 16, the rest log-uniform over 1 to 4096), splat scales, cameras, both composite modes, early-out on and off, the three property layouts and both record formats; every pixel within
the stated tolerance (2e-5 and 1 LSB off the saturation threshold; where the oracle flags a pixel whose alpha grazes
0.99 within 2e-5, one entry earlier or later is allowed: worth at most 0.0101 / 3 LSB with nearest-on-top blending; with
the reference's blend as written a later entry is laid OVER the pixel, so one more or less of them is not bounded and
those flagged pixels are only counted).  Test infrastructure (it loads oracle/):
    python tools/fuzz_pixels.py [cases=150] [seed=1]"""
import os
import sys
import time

import numpy as np

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
sys.path.insert(0, os.path.join(root, "tests"))
import splat_renderer_amd as sr
from helpers import make_case, oracle_pipeline
from oracle import oracle as O

TOL, TOL_NEAR = 2e-5, 0.0101
cases = int(sys.argv[1]) if len(sys.argv) > 1 else 150
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
dev = sr.Device(0)
t0, worst, worst_near, pixels, grazing_literal, off16, skipped = time.time(), 0.0, 0.0, 0, 0, 0, 0
for case in range(cases):
    n = int(rng.choice([rng.integers(1, 200), rng.integers(200, 4000), rng.integers(4000, 25000)]))
    w, h = int(rng.integers(1, 420)), int(rng.integers(1, 300))
    tile = 16 if rng.random() < 0.25 else int(np.exp(rng.uniform(0.0, np.log(4097.0))))  # 1..4096, log-uniform
    # (these screens hold at most 420 x 300 tiles; below T = 16 the splats shrink with the tile to keep the pairs in budget)
    rs = float(rng.choice([0.3, 1.0, 2.5, 6.0])) * (4.0 if n < 200 else 1.0) * min(1.0, np.sqrt(tile / 16))
    cam = dict(distance=float(rng.uniform(1.3, 5.0)), azimuth=float(rng.uniform(0, 6.28)), elevation=float(rng.uniform(-1.2, 1.2)))
    props, normals, u = make_case(n, w, h, 9000 + case, rs, camera=cam)
    ref = oracle_pipeline(props, normals, u, w, h, tile=tile)
    if ref["indices"].shape[0] > 3_000_000:
        skipped += 1
        continue
    mode = int(rng.integers(0, 2))
    eo = bool(rng.integers(0, 4))  # mostly on
    records = str(rng.choice(["lit", "projected"]))
    layout = str(rng.choice(["interleaved", "planes", "prelit"]))
    want, want8, _, _, near = O.composite(O.MODE_FRONT_TO_BACK if mode == 0 else O.MODE_REFERENCE_LITERAL, eo, props[:, 4:], normals,
                                          ref["proj"], ref["indices"], ref["counts"], ref["offsets"], w, h, tile=tile, want_stops=True)
    pm = sr.SplatPropertyManager(dev, n)
    pm.setFromArrays(props)
    nbuf = dev.createBufferFrom(normals)
    pbuf = {"interleaved": pm.getPropertyBuffer, "planes": pm.getPropertyPlanes, "prelit": lambda: pm.getLitPlanes(nbuf)}[layout]()
    r = sr.Renderer(dev, None, "rgba8unorm", n, tile, mode=sr.MODE_FRONT_TO_BACK if mode == 0 else sr.MODE_REFERENCE_LITERAL, earlyOut=eo,
                    records=records)
    # which kernel composites at T = 16 (these screens are below the 2048 tiles from which k_composite_px is the library's choice; other
    # tile sizes composite with k_composite_tile whatever is chosen): a third
    # of the cases each with the default, with k_composite_px one chunk ahead, and two chunks ahead with lanes running ahead —
    # and half of the forced ones as the THIRD launch over the same lists (its look-ahead bounded by the second's costs, its
    # tiles in the order the first's costs gave)
    kernel = str(rng.choice(["default", "px1", "px2"]))
    warm = bool(rng.integers(0, 2))
    dev.compositeOptions(None if kernel == "default" else "pixel", ahead={"default": 0, "px1": 1, "px2": 2}[kernel])
    for _ in range(2 if (warm and kernel != "default") else 0):
        r.render(u, pbuf, nbuf, None, w, h, wantFloat=True)
    r.render(u, pbuf, nbuf, None, w, h, wantFloat=True)
    got, got8 = r.readPixelsFloat(), r.readPixels()
    tag = (case, n, w, h, tile, rs, mode, eo, records, layout, kernel, warm)
    err = np.abs(got - want).max(axis=2)
    err8 = np.abs(got8.astype(int) - want8.astype(int)).max(axis=2)
    strict = (near == 0) if eo else np.ones_like(err, bool)
    assert err[strict].max(initial=0) <= TOL and err8[strict].max(initial=0) <= 1, tag
    if mode == 0:
        assert err.max() <= TOL_NEAR and err8.max() <= 3, tag
    else:
        grazing_literal += int((~strict).sum())
    worst = max(worst, float(err[strict].max(initial=0)))
    if mode == 0:
        worst_near = max(worst_near, float(err.max()))
    pixels += w * h
    off16 += int(tile != 16)
    for o in (r, pm, nbuf):
        o.destroy()
    if case % 25 == 24:
        print(f"{case + 1} cases, {pixels} pixels, worst off-threshold error {worst:.2e}, {time.time() - t0:.0f} s", flush=True)
dev.compositeOptions()
status = dev.rankStatus()
assert status["orderFaults"] == 0, f"a frame of this sweep was re-rendered after a failed order check: {status}"
print(f"ok: {cases - skipped} random frames ({off16} at tile sizes other than 16; {skipped} drawn over the pair budget skipped), {pixels} pixels: largest error off the threshold {worst:.2e} (tolerance {TOL}), "
      f"largest at threshold-grazing pixels, nearest-on-top blending, {worst_near:.2e} (bound {TOL_NEAR}); {grazing_literal} threshold-grazing "
      f"pixels in frames blended as the reference writes it (not bounded, not compared)" + f"; ranking {status}")
