#!/usr/bin/env python3
"""main.ts's whole frame with the reference's own render call: SdfSplatSource.step() (fresh cloud, five projection steps
onto the surface, curvature: one launch) then PointRenderer.render(uniforms, positions, gradients, scales, W, H) — the
opaque depth-tested quads src/Renderer.ts draws — on the demo scene of src/main.ts:55-81 (tools/attic/working_point.py
builds the same).  Prints ms per frame, generation + render and render alone, at 1920x1080 and 3840x2160, and writes the
1080p image as a PNG.
    python tools/point_frame.py [out.png] [frames=200]"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402

import splat_renderer_amd as sr  # noqa: E402
from splat_renderer_amd import sdf  # noqa: E402

png = sys.argv[1] if len(sys.argv) > 1 else "point_frame.png"
frames = int(sys.argv[2]) if len(sys.argv) > 2 else 200
scene = sdf.SDFScene()
s1 = sdf.Sphere(id="sphere1", position=(0, 0, 0), radius=0.5)
b1 = sdf.Box(id="box1", position=(0.6, 0, 0), size=(0.3, 0.3, 0.3))
s2 = sdf.Sphere(id="sphere2", position=(0, 0.6, 0), radius=0.25)
scene.setRoot(sdf.smoothUnion(0.1, sdf.smoothUnion(0.15, s1, b1), s2))
dev = sr.Device(0)
src = sr.SdfSplatSource(dev, scene, seed=1)
n = src.numPoints
renderer = sr.PointRenderer(dev, None, "rgba8unorm", n)


def timed(fn, k):
    for _ in range(5):
        fn()
    dev.sync()
    t0 = time.perf_counter()
    for _ in range(k):
        fn()
    dev.sync()
    return (time.perf_counter() - t0) / k * 1e3


src.step()
for w, h in ((1920, 1080), (3840, 2160)):
    cam = sr.Camera()
    cam.setAspect(w / h)
    u = cam.uniforms(w, h)

    def frame():
        src.step()  # main.ts:146-180
        pos, grad, scales, stride = src.getPointBuffers()
        renderer.render(u, pos, grad, scales, w, h, scaleStride=stride)  # main.ts:183-190

    both = timed(frame, frames)
    pos, grad, scales, stride = src.getPointBuffers()
    alone = timed(lambda: renderer.render(u, pos, grad, scales, w, h, scaleStride=stride), frames)
    ids = renderer.readIds()
    covered = float((ids != sr.PointRenderer.EMPTY).mean())
    print(f"demo scene, {n} points @{w}x{h}: generation + render {both:.3f} ms per frame ({1e3 / both:.0f} frames/s), "
          f"render alone {alone:.3f} ms; {covered * 100:.1f} % of the pixels covered, {len(np.unique(ids[ids != sr.PointRenderer.EMPTY]))} points visible")
    if w == 1920:
        sr.write_png(png, renderer.readPixels())
renderer.destroy()
src.destroy()
dev.destroy()
