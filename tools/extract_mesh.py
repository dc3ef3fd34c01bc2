#!/usr/bin/env python3
"""tools/extract_mesh.py IN.ply OUT.ply --voxel V [--views N --width W --height H --trunc T --alpha-min A --no-color]

The surface of a 3D Gaussian splatting PLY as a triangle mesh PLY: N pinhole cameras (autograd.pinhole_uniforms) orbit the box of
the cloud's means on three rings of elevation, each looking at its centre from 1.6 box diagonals away; GaussianFit.extract_mesh
renders their depth, fuses it into a TSDF volume of spacing V and pulls the mesh out (include/splat.h, "TSDF fusion and mesh
extraction").  Needs a GPU."""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def orbit_cameras(torch, AG, lo, hi, views, width, height):
    centre, diagonal = 0.5 * (lo + hi), float(np.linalg.norm(hi - lo))
    distance = 1.6 * diagonal
    focal = 0.9 * min(width, height) * distance / diagonal  # the box's diagonal fills nine tenths of the shorter side
    cams = []
    for k in range(views):
        azimuth = 2 * math.pi * k / views
        elevation = (-0.5, 0.1, 0.6)[k % 3]
        eye = centre + distance * np.array([math.cos(azimuth) * math.cos(elevation), math.sin(elevation), math.sin(azimuth) * math.cos(elevation)])
        fwd = (centre - eye) / np.linalg.norm(centre - eye)
        right = np.cross(fwd, (0.0, 1.0, 0.0))
        right /= np.linalg.norm(right)
        R = np.stack([right, np.cross(fwd, right), fwd])
        cams.append(AG.pinhole_uniforms(torch.as_tensor(R), torch.as_tensor(-R @ eye), focal, focal, width / 2, height / 2, width, height,
                                        near=0.01 * diagonal, far=10 * diagonal).float())
    return cams


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[1])
    ap.add_argument("input")
    ap.add_argument("output")
    ap.add_argument("--voxel", type=float, required=True)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--height", type=int, default=800)
    ap.add_argument("--trunc", type=float, default=None)
    ap.add_argument("--alpha-min", type=float, default=0.5)
    ap.add_argument("--no-color", action="store_true")
    args = ap.parse_args()
    import torch
    import splat_renderer_amd as sr
    from splat_renderer_amd import autograd as AG
    if not torch.cuda.is_available():
        raise SystemExit("extract_mesh: no GPU (there is no CPU path)")
    cloud = sr.load_gaussian_ply(args.input)
    fit = sr.GaussianFit(cloud["positions"], cloud["scales"], cloud["rotations"], cloud["opacity"], cloud["sh"], exact_activations=True)
    lo, hi = cloud["positions"].min(axis=0).astype(np.float64), cloud["positions"].max(axis=0).astype(np.float64)
    cams = orbit_cameras(torch, AG, lo, hi, args.views, args.width, args.height)
    mesh = fit.extract_mesh(cams, args.width, args.height, args.voxel, trunc=args.trunc, alpha_min=args.alpha_min, color=not args.no_color)
    vertices, triangles = mesh[0].cpu().numpy(), mesh[1].cpu().numpy()
    sr.save_mesh_ply(args.output, vertices, triangles, None if args.no_color else mesh[2].clamp(0.0, 1.0).cpu().numpy())
    print(f"{args.output}: {len(vertices)} vertices, {len(triangles)} triangles from {fit.n} splats, {args.views} views of {args.width} x {args.height}, voxel {args.voxel}")


if __name__ == "__main__":
    main()
