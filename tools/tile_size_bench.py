#!/usr/bin/env python3
"""Whole frames of one scene at several tile sizes (GPU box only): python tools/tile_size_bench.py [C2] [K] [sizes, e.g. 8,16,24,32,64]

One JSON line per tile size: device ms per frame (K frames, no events), the per-stage times of 10 frames with every stage's
event pair on (setTiming), the pair total, and the composite's staged / consumed list entries per frame.  Tile size 16 runs
k_composite_px (composite_px.hip; or k_composite, composite.hip, on small screens); every other size runs k_composite_tile
(composite_tile.hip)."""
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import splat_renderer_amd as sr
from splat_renderer_amd import _lib

name = sys.argv[1] if len(sys.argv) > 1 else "C2"
k = int(sys.argv[2]) if len(sys.argv) > 2 else 20
sizes = [int(s) for s in sys.argv[3].split(",")] if len(sys.argv) > 3 else [8, 16, 24, 32, 64]
n, w, h = sr.scene.CONFIGS[name]
props, normals = sr.scene.make_scene(n)
cam = sr.Camera()
cam.setAspect(w / h)
u = cam.uniforms(w, h)
dev = sr.Device(0)
lib, ctx = dev.lib, dev.ctx
pm = sr.SplatPropertyManager(dev, n)
pm.setFromArrays(props)
pbuf, nbuf = pm.getPropertyBuffer(), dev.createBufferFrom(normals)
for tile in sizes:
    r = sr.Renderer(dev, None, "rgba8unorm", n, tile)
    frame = lambda: r.render(u, pbuf, nbuf, None, w, h)
    for _ in range(10):  # warm-up (and the sync-free frames' learnt pair limit)
        frame()
    r.finish()
    dev.sync()
    t0 = time.perf_counter()
    for _ in range(k):
        frame()
    dev.sync()
    ms = (time.perf_counter() - t0) / k * 1e3
    # per-stage times and the composite's entries, from 10 more frames with every stage timed and the entries counted
    _lib.check(lib.splat_set_timing_stages(ctx, 0xFFFFFFFF), ctx)
    dev.setTiming(True)
    for _ in range(10):
        frame()
    dev.sync()
    stage_ms = {}
    for sid, sname in enumerate(_lib.STAGE_NAMES):
        cnt, tot = C.c_uint32(), C.c_double()
        _lib.check(lib.splat_stage_time_stats(ctx, sid, C.byref(cnt), C.byref(tot)), ctx)
        if cnt.value:
            stage_ms[sname] = round(tot.value / cnt.value, 4)
    staged, consumed = C.c_uint64(), C.c_uint64()
    _lib.check(lib.splat_timing_consumed(ctx, C.byref(staged), C.byref(consumed)), ctx)
    dev.setTiming(False)
    pairs = r.finish()
    print(json.dumps({"config": name, "tile": tile, "tiles": -(-w // tile) * -(-h // tile), "ms_per_frame": round(ms, 4),
                      "stage_ms": stage_ms, "pairs": pairs, "composite_staged": staged.value // 10,
                      "composite_consumed": consumed.value // 10}), flush=True)
    r.destroy()
nbuf.destroy()
pm.destroy()
dev.destroy()
