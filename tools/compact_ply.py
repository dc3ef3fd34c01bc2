#!/usr/bin/env python3
"""Prune a 3D Gaussian splatting PLY by what a ring of views sees of every splat (GPU box only):

    python tools/compact_ply.py IN.ply OUT.ply (--threshold 0.01 | --keep 0.5) [--views 24 --width 640 --height 360 --kind max]

The views are tools/turntable.py's: the orbit Camera turned by 2 pi / views after each, here aimed at the cloud's centre from a
distance that holds its bulk.  Every view is scored with GaussianFit.accumulate_importance (one forward walk of the tile lists:
splat_composite_contribution), the cloud is cut with GaussianFit.prune_by_importance - --threshold keeps score >= threshold
(RadSplat prunes at 0.01 of the largest blend weight), --keep the best count (an integer) or fraction (a number with a point, in
(0, 1]) - and saved.  Prints the splat count before and after and the PSNR of the pruned cloud's frames against the unpruned
cloud's over the same views.
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import splat_renderer_amd as sr
from splat_renderer_amd.fit import GaussianFit
from splat_renderer_amd.ply import load_gaussian_ply


def orbit_uniforms(centre, radius, views, width, height):
    """The uniform blocks of `views` cameras of one full orbit around `centre`, as FrameLoop.turntable turns its Camera."""
    cam = sr.Camera()
    cam.setAspect(width / height)
    cam.target = np.asarray(centre, np.float32)
    cam.distance = float(max(2.5 * radius, 4.0 * cam.near))
    cam.far = max(cam.far, 4.0 * cam.distance)
    out = []
    for _ in range(views):
        out.append(cam.uniforms(width, height).copy())
        cam.rotate(2.0 * math.pi / views, 0.0)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("input")
    ap.add_argument("output")
    cut = ap.add_mutually_exclusive_group(required=True)
    cut.add_argument("--threshold", type=float, help="keep splats whose score is at least this")
    cut.add_argument("--keep", help="keep the best splats: a count (integer) or a fraction in (0, 1] (with a point)")
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--kind", default="max", choices=["max", "sum", "hits", "lightgaussian"])
    args = ap.parse_args()
    keep = None
    if args.keep is not None:
        keep = float(args.keep) if any(c in args.keep for c in ".eE") else int(args.keep)

    cloud = load_gaussian_ply(args.input)
    fit = GaussianFit(cloud["positions"], cloud["scales"], cloud["rotations"], cloud["opacity"], cloud["sh"], degree=cloud["degree"],
                      exact_activations=True)
    before = fit.n
    pos = np.asarray(cloud["positions"], np.float64)
    finite = pos[np.isfinite(pos).all(axis=1)]
    centre = np.median(finite, axis=0) if finite.size else np.zeros(3)
    radius = float(np.quantile(np.linalg.norm(finite - centre, axis=1), 0.95)) if finite.size else 1.0
    cams = orbit_uniforms(centre, max(radius, 1e-3), args.views, args.width, args.height)

    def frames():
        with torch.no_grad():
            return [fit.render(u, args.width, args.height)[0].clone() for u in cams]

    full = frames()
    for u in cams:
        fit.accumulate_importance(u, args.width, args.height)
    counts = fit.prune_by_importance(threshold=args.threshold, keep=keep, kind=args.kind)
    pruned = frames()
    mse = torch.stack([((a - b).double() ** 2).mean() for a, b in zip(full, pruned)]).mean().item()
    psnr = math.inf if mse == 0.0 else -10.0 * math.log10(mse)
    fit.save_ply(args.output)
    print(f"{args.input}: {before} splats -> {counts['n']} splats ({counts['pruned']} pruned by {args.kind} over {args.views} views of "
          f"{args.width}x{args.height}); PSNR of pruned against unpruned frames {psnr:.2f} dB -> {args.output}")


if __name__ == "__main__":
    main()
