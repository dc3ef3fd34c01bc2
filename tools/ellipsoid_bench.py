#!/usr/bin/env python3
"""Anisotropic Gaussians against the other footprints (GPU box only): python tools/ellipsoid_bench.py [C1,C2] [K] [R] [--antialiased]

Per config one JSON line: device ms of splat_project_ellipsoid (with the fused keys), of splat_sh_colors at degree 3, and of
whole ellipsoid, disc and isotropic frames (Renderer, default settings) on the same positions — the scene's, with sigma =
radius / 2 per axis times a random factor in [e^-0.3, e^0.3], random rotations and the scene's colours — R rounds of K calls
each, the kinds alternating round by round in one process, timed with device events after a warm-up.  The frames' tile-list
pair totals are printed beside them: the composite's cost follows the pairs, so frames compare by pairs.
--antialiased: also splat_project_ellipsoid_aa with every output ("project_aa") and the antialiased whole frame ("ellipsoid_aa",
splat_render_frame_ellipsoids_aa), in the same rounds as their classic twins."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import splat_renderer_amd as sr

antialiased = "--antialiased" in sys.argv[1:]
argv = [a for a in sys.argv if not a.startswith("--")]
names = argv[1].split(",") if len(argv) > 1 else ["C1", "C2"]
k = int(argv[2]) if len(argv) > 2 else 50
rounds = int(argv[3]) if len(argv) > 3 else 7
stream = torch.cuda.current_stream()
dev = sr.Device(0, stream=stream.cuda_stream)
for name in names:
    n, w, h = sr.scene.CONFIGS[name]
    props, normals = sr.scene.make_scene(n)
    rng = np.random.default_rng(0)
    scl = (props[:, 3:4] * 0.5 * np.exp(rng.uniform(-0.3, 0.3, (n, 3)))).astype(np.float32)
    rot = rng.normal(size=(n, 4)).astype(np.float32)
    sh = rng.normal(0, 0.3, (n, 16, 3)).astype(np.float32)
    cam = sr.Camera()
    cam.setAspect(w / h)
    u = cam.uniforms(w, h)
    cloud = sr.GaussianCloud.fromArrays(dev, props[:, :3], scl, rot, colors=props[:, 4:8])
    shcloud = sr.GaussianCloud.fromArrays(dev, props[:, :3], scl, rot, opacity=props[:, 7], sh=sh)
    pm = sr.SplatPropertyManager(dev, n)
    pm.setFromArrays(props)
    pbuf, nbuf = pm.getPropertyBuffer(), dev.createBufferFrom(normals)
    proj = sr.SplatProjector(dev, n, footprint="ellipsoid")
    sorter = sr.RadixSorter(dev, n)
    rs = {fp: sr.Renderer(dev, None, "rgba8unorm", n, footprint=fp) for fp in ("ellipsoid", "disc", "isotropic")}
    work = {
        "project": lambda: proj.project(None, u, None, sorter.getKeysBuffer(), sorter.getPayloadBuffer(), sorter.paddedSize, cloud=cloud),
        "sh3": lambda: shcloud.updateColors(u[16:19]),
        "ellipsoid": lambda: rs["ellipsoid"].render(u, cloud, None, None, w, h),
        "disc": lambda: rs["disc"].render(u, pbuf, nbuf, None, w, h),
        "isotropic": lambda: rs["isotropic"].render(u, pbuf, nbuf, None, w, h),
    }

    extra = []
    if antialiased:
        proj_aa = sr.SplatProjector(dev, n, footprint="ellipsoid", antialiased=True)
        rs["ellipsoid_aa"] = sr.Renderer(dev, None, "rgba8unorm", n, footprint="ellipsoid", antialiased=True)
        comp = dev.createBuffer(n * 16)
        lib = dev.lib

        def project_aa():  # every output: records, ProjectedSplats, keys, rho and the compensated colour plane
            import ctypes as C
            sr._lib.check(lib.splat_project_ellipsoid_aa(dev.ctx, u.ctypes.data_as(C.POINTER(C.c_float)), cloud.positions.ptr, 1, cloud.scales.ptr, 1,
                                                         cloud.rotations.ptr, 1, n, proj_aa.projectedBuffer.ptr, proj_aa.discBuffer.ptr,
                                                         sorter.getKeysBuffer().ptr, sorter.getPayloadBuffer().ptr, sorter.paddedSize,
                                                         proj_aa.compensationBuffer.ptr, cloud.colorOpacity.ptr, 1, comp.ptr), dev.ctx)
        work["project_aa"] = project_aa
        work["ellipsoid_aa"] = lambda: rs["ellipsoid_aa"].render(u, cloud, None, None, w, h)
        extra = [proj_aa, comp]

    def run(kind, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            work[kind]()
        e1.record(stream)
        if kind in rs:
            rs[kind].finish()
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    for kind in list(work) * 2:
        run(kind, 10)
    t = {kind: [] for kind in work}
    for _ in range(rounds):
        for kind in work:
            t[kind].append(run(kind, k))
    pairs = {fp: int(r.binner.getTotalIndices()) for fp, r in rs.items()}
    med = {kind: sorted(v)[len(v) // 2] for kind, v in t.items()}
    print(json.dumps({"config": name, "n": n, "calls_per_round": k, "rounds": rounds,
                      **{f"{kind}_ms": round(v, 4) for kind, v in med.items()},
                      **{f"{kind}_ms_min_max": [round(min(v), 4), round(max(v), 4)] for kind, v in t.items()},
                      "pairs": pairs}), flush=True)
    for o in [proj, sorter, pm, nbuf, cloud, shcloud] + extra:
        o.destroy()
dev.destroy()
