#!/usr/bin/env python3
"""Gradients of ellipsoid frames (GPU box only): python tools/grad_bench.py [--depth] [C1,C2] [K] [R]

tools/ellipsoid_bench.py's scenes and method (the scene's positions, sigma = radius / 2 per axis times a random factor in
[e^-0.3, e^0.3], random rotations, SH of degree 3 with the scene's opacity; R rounds of K calls per kind, kinds alternating
round by round, device events after a warm-up, the median round).  Per config one JSON line: the staged forward
(splat_renderer_amd.autograd: project, SH colour, sort, bin, composite with alpha) and its backward (loss = sum of
rgb * a fixed random image, through torch.autograd), each backward kernel alone (splat_composite_backward,
splat_project_ellipsoid_backward, splat_sh_colors_backward), the (tile, entry) pairs the forward consumed (the composite's
own counters), and the bytes of float atomic adds those pairs bound (36 per pair: five record and four colour sums) with
the time they take at 1.3 TB/s.

--depth adds, beside the colour-only figures: the forward with the depth map (rasterize(..., depths=)), its backward with a
depth loss as well (loss += sum of depth * a fixed random image where depth is finite), the depth variant of the composite
backward alone (splat_composite_backward_depth) and of the projector's (splat_project_ellipsoid_backward_depth); the atomic
bytes then count 40 per consumed pair (the tenth sum, dL/dz)."""
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import splat_renderer_amd as sr
from splat_renderer_amd import _lib
from splat_renderer_amd import autograd as AG

ATOMIC_RATE = 1.3e12  # bytes / s of global float atomic adds, chip-wide

argv = [a for a in sys.argv[1:] if a != "--depth"]
depth_too = len(argv) != len(sys.argv) - 1
names = argv[0].split(",") if len(argv) > 0 else ["C1", "C2"]
k = int(argv[1]) if len(argv) > 1 else 20
rounds = int(argv[2]) if len(argv) > 2 else 7
stream = torch.cuda.current_stream()
for name in names:
    n, w, h = sr.scene.CONFIGS[name]
    props, _ = sr.scene.make_scene(n)
    rng = np.random.default_rng(0)
    scl = (props[:, 3:4] * 0.5 * np.exp(rng.uniform(-0.3, 0.3, (n, 3)))).astype(np.float32)
    rot = rng.normal(size=(n, 4)).astype(np.float32)
    sh = rng.normal(0, 0.3, (n, 16, 3)).astype(np.float32)
    cam = sr.Camera()
    cam.setAspect(w / h)
    u = cam.uniforms(w, h)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda", requires_grad=True)  # noqa: E731
    means, scales, rots, ops, shs = t(props[:, :3]), t(scl), t(rot), t(props[:, 7]), t(sh)
    gimg = torch.rand((h, w, 3), device="cuda") * 2 - 1
    state = {}

    def forward():
        rec, aux = AG.project_ellipsoids(u, means, scales, rots)
        col = AG.sh_colors(u[16:19], means, shs, 3, ops)
        rgb, _ = AG.rasterize(rec, col, aux, w, h)
        state.update(rec=rec, col=col, aux=aux, loss=(rgb * gimg).sum())

    def backward():
        state["loss"].backward()

    gdimg = torch.rand((h, w), device="cuda") * 2 - 1

    def forward_depth():
        rec, depths, aux = AG.project_ellipsoids(u, means, scales, rots, return_depth=True)
        col = AG.sh_colors(u[16:19], means, shs, 3, ops)
        rgb, _, depth = AG.rasterize(rec, col, aux, w, h, depths=depths)
        dz = torch.where(torch.isfinite(depth), depth, torch.zeros_like(depth))
        state.update(rec=rec, col=col, aux=aux, depths=depths, loss=(rgb * gimg).sum() + (dz * gdimg).sum())

    forward()
    backward()
    cx = state["aux"].ctx
    rec, col = state["rec"].detach().contiguous(), state["col"].detach().contiguous()
    zs = state["aux"].projected[:, 4].contiguous()
    gz = torch.zeros(n, device="cuda")
    gzp = torch.rand(n, device="cuda")
    m4 = torch.cat([means.detach(), torch.ones((n, 1), device="cuda")], 1).contiguous()
    s4 = torch.cat([scales.detach(), torch.zeros((n, 1), device="cuda")], 1).contiguous()
    g4 = torch.zeros((h, w, 4), device="cuda")
    g4[..., :3] = gimg
    grec, gcol = torch.zeros((n, 8), device="cuda"), torch.zeros((n, 4), device="cuda")
    gp, gs, gq = (torch.empty((n, 4), device="cuda") for _ in range(3))
    gsh, gop = torch.empty_like(shs).reshape(n, -1), torch.empty(n, device="cuda")
    cfg = _lib.CompositeCfg(_lib.MODE_FRONT_TO_BACK, 1, 16, 0, _lib.U32_MAX, _lib.RECORDS_PROJECTED, 1, _lib.FOOTPRINT_ELLIPSOID)
    uf = u.ctypes.data_as(C.POINTER(C.c_float))
    eye = np.ascontiguousarray(u[16:19])
    lib = cx.lib
    cx.bin(state["aux"], w, h)
    idx, cnt, off = cx.lists()
    tiles = -(-w // 16) * -(-h // 16)
    consumed = torch.zeros(2 * tiles, dtype=torch.int64, device="cuda")
    out = torch.empty((h, w, 4), device="cuda")
    _lib.check(lib.splat_composite(cx.ctx, C.byref(cfg), col.data_ptr(), 1, None, 1, rec.data_ptr(), idx, cnt, off, w, h, None,
                                   out.data_ptr(), consumed.data_ptr()), cx.ctx)
    torch.cuda.synchronize()
    tot = C.c_uint64()
    _lib.check(lib.splat_bin_total(cx.binner, C.byref(tot)), cx.ctx)
    pairs = int(tot.value)
    staged_pairs, consumed_pairs = int(consumed[0::2].sum()), int(consumed[1::2].sum())
    work = {
        "forward": forward,
        "backward": None,  # (a forward, then its backward; the forward's time is taken off)
        "composite_backward": lambda: lib.splat_composite_backward(cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), idx, cnt, off, w, h,
                                                                   g4.data_ptr(), n, grec.data_ptr(), gcol.data_ptr()),
        "project_backward": lambda: lib.splat_project_ellipsoid_backward(cx.ctx, uf, m4.data_ptr(), 1, s4.data_ptr(), 1, rots.data_ptr(), 1, n,
                                                                          grec.data_ptr(), gp.data_ptr(), gs.data_ptr(), gq.data_ptr()),
        "sh3_backward": lambda: lib.splat_sh_colors_backward(cx.ctx, eye.ctypes.data_as(C.POINTER(C.c_float)), m4.data_ptr(), 1, shs.data_ptr(),
                                                             48, 3, ops.data_ptr(), gcol.data_ptr(), n, gsh.data_ptr(), gp.data_ptr(),
                                                             gop.data_ptr()),
    }
    if depth_too:
        work.update({
            "forward_depth": forward_depth,
            "backward_depth": None,
            "composite_backward_depth": lambda: lib.splat_composite_backward_depth(cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), idx, cnt,
                                                                               off, w, h, g4.data_ptr(), n, grec.data_ptr(), gcol.data_ptr(),
                                                                               zs.data_ptr(), 1, gdimg.data_ptr(), gz.data_ptr()),
            "project_backward_depth": lambda: lib.splat_project_ellipsoid_backward_depth(cx.ctx, uf, m4.data_ptr(), 1, s4.data_ptr(), 1,
                                                                                         rots.data_ptr(), 1, n, grec.data_ptr(), gp.data_ptr(),
                                                                                         gs.data_ptr(), gq.data_ptr(), gzp.data_ptr()),
        })

    def run(kind, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if kind in ("backward", "backward_depth"):
            tot = 0.0
            for _ in range(calls):
                (forward if kind == "backward" else forward_depth)()
                e0.record(stream)
                backward()
                e1.record(stream)
                e1.synchronize()
                tot += e0.elapsed_time(e1)
            return tot / calls
        e0.record(stream)
        for _ in range(calls):
            work[kind]()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    for kind in list(work) * 2:
        run(kind, 3)
    ts = {kind: [] for kind in work}
    for _ in range(rounds):
        for kind in work:
            ts[kind].append(run(kind, k))
    med = {kind: sorted(v)[len(v) // 2] for kind, v in ts.items()}
    atomic_bytes = 36 * consumed_pairs
    extra = {}
    if depth_too:
        extra = {"atomic_bytes_bound_depth": 40 * consumed_pairs, "atomic_floor_ms_depth": round(40 * consumed_pairs / ATOMIC_RATE * 1e3, 4),
                 "composite_backward_depth_over_colour": round(med["composite_backward_depth"] / med["composite_backward"], 3)}
    print(json.dumps({"config": name, "n": n, "calls_per_round": k, "rounds": rounds,
                      **{f"{kind}_ms": round(v, 4) for kind, v in med.items()},
                      **{f"{kind}_ms_min_max": [round(min(v), 4), round(max(v), 4)] for kind, v in ts.items()},
                      "pairs": pairs,
                      "staged_pairs": staged_pairs, "consumed_pairs": consumed_pairs,
                      "atomic_bytes_bound": atomic_bytes, "atomic_floor_ms": round(atomic_bytes / ATOMIC_RATE * 1e3, 4), **extra}), flush=True)
