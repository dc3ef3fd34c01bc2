#!/usr/bin/env python3
"""Whole frames with and without the auxiliary outputs (GPU box only): python tools/aov_bench.py [C1,C2] [K] [R]

Per config one JSON line: device ms per frame of the plain frame and of the same frame with wantAov=True (depth, alpha and
splat-id buffers), R rounds of K frames each, the two kinds alternating round by round in one process, timed with device
events (torch.cuda.Event on the stream the library enqueues on) after a warm-up of both.  The per-kernel cost comes from a
separate `rocprofv3 --kernel-trace --stats` run of this script (profiles/)."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

import splat_renderer_amd as sr

names = sys.argv[1].split(",") if len(sys.argv) > 1 else ["C1", "C2"]
k = int(sys.argv[2]) if len(sys.argv) > 2 else 100
rounds = int(sys.argv[3]) if len(sys.argv) > 3 else 10
stream = torch.cuda.current_stream()
dev = sr.Device(0, stream=stream.cuda_stream)
for name in names:
    n, w, h = sr.scene.CONFIGS[name]
    props, normals = sr.scene.make_scene(n)
    cam = sr.Camera()
    cam.setAspect(w / h)
    u = cam.uniforms(w, h)
    pm = sr.SplatPropertyManager(dev, n)
    pm.setFromArrays(props)
    pbuf, nbuf = pm.getPropertyBuffer(), dev.createBufferFrom(normals)
    r = sr.Renderer(dev, None, "rgba8unorm", n)

    def run(aov, frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(frames):
            r.render(u, pbuf, nbuf, None, w, h, wantAov=aov)
        e1.record(stream)
        r.finish()
        e1.synchronize()
        return e0.elapsed_time(e1) / frames

    for aov in (False, True, False, True):  # warm-up (and the sync-free frames' learnt pair limit)
        run(aov, 20)
    plain, withaov = [], []
    for _ in range(rounds):
        plain.append(run(False, k))
        withaov.append(run(True, k))
    plain.sort()
    withaov.sort()
    med = lambda a: a[len(a) // 2]
    print(json.dumps({"config": name, "frames_per_round": k, "rounds": rounds, "plain_ms": round(med(plain), 4),
                      "aov_ms": round(med(withaov), 4), "delta_us": round((med(withaov) - med(plain)) * 1e3, 1),
                      "plain_ms_min_max": [round(plain[0], 4), round(plain[-1], 4)],
                      "aov_ms_min_max": [round(withaov[0], 4), round(withaov[-1], 4)]}), flush=True)
    for o in (r, pm, nbuf):
        o.destroy()
dev.destroy()
