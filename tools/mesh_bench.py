#!/usr/bin/env python3
"""tools/mesh_bench.py [--sizes 256,512] [--rounds 9] [--out profiles/tsdf_bench.txt]

Time of TSDF fusion and mesh extraction (include/splat.h, "TSDF fusion and mesh extraction") on one GPU.

Integration: one 1920 x 1080 view of a sphere (an analytic distance map, +inf beside it) into a volume of size^3 nodes that
earlier views have already filled, without and with colour, the two alternating round by round: per variant the median (fastest
to slowest) of `rounds` launches between device events after two warm-up launches, the bytes the launch actually moves (per
written node: weight and tsdf read and written, 16 B; with colour 24 B more; the nodes are counted after the run), and the time
as a multiple of the HBM floor, those bytes over the 5.1 TB/s this box copies at (DESIGN.md's figure for floors).  For scale the
same integration written in float32 torch ops at the first size.
Extraction: the sphere's own distance field in the same volumes, splat_tsdf_mesh_count (classification, two scans, the host wait)
and splat_tsdf_mesh_emit timed separately, against the floors 42 B per node (8 read and 10 written by the classification, 12 by
each scan) and 2 B per node plus the mesh written.
No CPU fallback: without a GPU this fails."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COPY_RATE = 5.1e12  # bytes per second: the box's measured copy rate, the figure DESIGN.md uses for floors
W, H = 1920, 1080


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def spread(times):
    return f"{float(np.median(times)):8.3f} ms ({min(times):.3f} to {max(times):.3f})"


def torch_integrate(torch, tsdf, weight, origin, voxel, trunc, vp, eye, depth):
    """The contract's ten steps in float32 torch ops (distance depth, no weight map, no colour), in place."""
    nz, ny, nx = tsdf.shape
    dev = tsdf.device
    x = origin[0] + voxel * torch.arange(nx, device=dev, dtype=torch.float32)[None, None, :]
    y = origin[1] + voxel * torch.arange(ny, device=dev, dtype=torch.float32)[None, :, None]
    z = origin[2] + voxel * torch.arange(nz, device=dev, dtype=torch.float32)[:, None, None]
    row = lambda r: vp[r] * x + vp[4 + r] * y + vp[8 + r] * z + vp[12 + r]  # noqa: E731
    cw = row(3)
    pu, pv = (row(0) / cw * 0.5 + 0.5) * W, (0.5 - 0.5 * row(1) / cw) * H
    ok = (cw > 0) & (pu >= 0) & (pu < W) & (pv >= 0) & (pv < H)
    p = torch.where(ok, pv.floor().long() * W + pu.floor().long(), torch.zeros((), device=dev, dtype=torch.long))
    D = depth.reshape(-1)[p]
    ok &= (D > 0) & torch.isfinite(D)
    s = D - torch.sqrt((x - eye[0]) ** 2 + (y - eye[1]) ** 2 + (z - eye[2]) ** 2)
    ok &= s >= -trunc
    f = torch.clamp(s / trunc, max=1.0)
    w1 = weight + 1.0
    tsdf.copy_(torch.where(ok, (tsdf * weight + f) / w1, tsdf))
    weight.copy_(torch.where(ok, w1, weight))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256,512")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsdf_bench.txt"))
    args = ap.parse_args()
    import torch
    import splat_renderer_amd as sr
    from splat_renderer_amd import _lib
    from splat_renderer_amd import autograd as AG
    if not torch.cuda.is_available():
        raise SystemExit("mesh_bench: no GPU (there is no CPU path to time)")
    sizes = [int(s) for s in args.sizes.split(",")]
    lines = [f"# tools/mesh_bench.py --sizes {args.sizes} --rounds {args.rounds}: {torch.cuda.get_device_name(0)}; median (fastest to slowest) of "
             f"{args.rounds} launches between device events, 2 warm-up launches; floors at {COPY_RATE / 1e12:.1f} TB/s"]
    # a camera at (0.4, 0.3, -3) looking at the origin; the sphere of radius 0.6 around it; the volume spans [-1, 1]^3
    eye = np.array([0.4, 0.3, -3.0])
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, (0.0, 1.0, 0.0))
    right /= np.linalg.norm(right)
    R = np.stack([right, np.cross(fwd, right), fwd])
    focal = 1500.0
    u = AG.pinhole_uniforms(torch.as_tensor(R), torch.as_tensor(-R @ eye), focal, focal, W / 2, H / 2, W, H).numpy().astype(np.float32)
    ys, xs = np.mgrid[0:H, 0:W]
    d = (((xs + 0.5 - W / 2) / focal)[..., None] * R[0] + ((ys + 0.5 - H / 2) / focal)[..., None] * R[1] + R[2])
    d /= np.linalg.norm(d, axis=2, keepdims=True)
    b = d @ eye
    disc = b * b - (eye @ eye - 0.36)
    depth = torch.from_numpy(np.where(disc > 0, -b - np.sqrt(np.maximum(disc, 0)), np.inf).astype(np.float32)).cuda()
    image = torch.rand((H, W, 3), device="cuda")
    for size in sizes:
        voxel = 2.0 / (size - 1)
        trunc = 4 * voxel
        results = {}
        vols = {c: sr.TsdfVolume((-1.0, -1.0, -1.0), voxel, (size,) * 3, trunc, color=c) for c in (False, True)}
        times = {False: [], True: []}
        for c, vol in vols.items():
            for _ in range(2):
                vol.integrate(depth, u, image=image if c else None)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for c, vol in vols.items():
                times[c].append(timed(torch, lambda: vol.integrate(depth, u, image=image if c else None)))
        for c, vol in vols.items():
            written = int((vol.weight > 0).sum())
            moved = written * (40 if c else 16)
            floor = moved / COPY_RATE * 1e3
            med = float(np.median(times[c]))
            results[c] = med
            line = (f"integrate {size}^3 {'colour' if c else 'plain '} | {spread(times[c])} | {written} of {size ** 3} nodes written, {moved / 1e6:.1f} MB: "
                    f"floor {floor:.3f} ms, {med / floor:.2f} x floor | {size ** 3 / med / 1e6:.0f} Gnodes/s visited")
            print(line, flush=True)
            lines.append(line)
        if size == sizes[0]:
            vol = vols[False]
            tt, tw = vol.tsdf.clone(), vol.weight.clone()
            vp, e = torch.from_numpy(u[:16]).cuda(), torch.from_numpy(u[16:19]).cuda()
            args_t = (torch, tt, tw, (-1.0, -1.0, -1.0), voxel, trunc, vp, e, depth)
            torch_integrate(*args_t)
            torch.cuda.synchronize()
            t_times = [timed(torch, lambda: torch_integrate(*args_t)) for _ in range(5)]
            line = f"integrate {size}^3 plain, float32 torch ops (a baseline, not a target) | {spread(t_times)} | {float(np.median(t_times)) / results[False]:.1f} x the kernel"
            print(line, flush=True)
            lines.append(line)
            del tt, tw
        del vols
        torch.cuda.empty_cache()
        # extraction of the sphere's own distance field
        vol = sr.TsdfVolume((-1.0, -1.0, -1.0), voxel, (size,) * 3, trunc, color=False)
        ax = -1.0 + voxel * torch.arange(size, device="cuda", dtype=torch.float32)
        vol.tsdf.copy_(torch.clamp((torch.sqrt(ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2) - 0.6) / trunc, -1.0, 1.0))
        vol.weight.fill_(1.0)
        cx = AG._context(vol.tsdf)
        nbytes = int(cx.lib.splat_tsdf_mesh_workspace_bytes(size, size, size))
        ws = torch.empty(nbytes, device="cuda", dtype=torch.uint8)
        nv, nt = C.c_uint32(), C.c_uint32()

        def count():
            _lib.check(cx.lib.splat_tsdf_mesh_count(cx.ctx, C.byref(vol.grid), vol.tsdf.data_ptr(), vol.weight.data_ptr(), 0.0, ws.data_ptr(), nbytes,
                                                    C.byref(nv), C.byref(nt)), cx.ctx)
        count()
        vertices, triangles = torch.empty((nv.value, 3), device="cuda"), torch.empty((nt.value, 3), device="cuda", dtype=torch.int32)

        def emit():
            _lib.check(cx.lib.splat_tsdf_mesh_emit(cx.ctx, C.byref(vol.grid), vol.tsdf.data_ptr(), None, ws.data_ptr(), nbytes, vertices.data_ptr(), None,
                                                   triangles.data_ptr()), cx.ctx)
        emit()
        count()
        torch.cuda.synchronize()
        tc, te = [], []
        for _ in range(args.rounds):
            tc.append(timed(torch, count))
            te.append(timed(torch, emit))
        n = size ** 3
        fc, fe = 42 * n / COPY_RATE * 1e3, (2 * n + 12 * (nv.value + nt.value)) / COPY_RATE * 1e3
        for name, t, fl in (("count", tc, fc), ("emit ", te, fe)):
            med = float(np.median(t))
            line = f"mesh {name} {size}^3 | {spread(t)} | floor {fl:.3f} ms, {med / fl:.2f} x floor | {nv.value} vertices, {nt.value} triangles"
            print(line, flush=True)
            lines.append(line)
        del vol, ws, vertices, triangles
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
