#!/usr/bin/env python3
"""tools/knn_bench.py [--sizes 100000,1000000,5000000] [--rounds 7] [--out profiles/knn_bench.txt]

Time and work of splat_knn_mean_sq (include/splat.h, "Initialisation from a point cloud") on one GPU: per scene (a uniform cube,
the unit sphere's surface, the cube with eight outliers a thousand extents away) and size, the call's time between two device
events on the stream it runs on (the median of `rounds` calls after two warm-up calls, with the fastest and the slowest), the
distance evaluations per query it counted, and the share of the two radix sort passes, from the context's SPLAT_STAGE_SORT
timing in a separate pass over the same input (stage events cost a few microseconds each, so they are off while the call is
timed).  For scale, torch's brute force (chunks of 2 048 queries against all points, per-axis squares, topk) at the first size.
No CPU fallback: without a GPU this fails."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make(scene, n, seed=3):
    rng = np.random.default_rng(seed)
    if scene == "sphere":
        v = rng.normal(size=(n, 3))
        return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    p = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    if scene == "outliers":
        p[:8] = rng.uniform(-1000, 1000, (8, 3)).astype(np.float32)
    return p


def torch_brute_force(torch, pts, chunk=2048):
    x, y, z = (pts[:, a].contiguous() for a in range(3))
    out = torch.empty(pts.shape[0], device=pts.device)
    for s in range(0, pts.shape[0], chunk):
        e = min(s + chunk, pts.shape[0])
        d = (x[s:e, None] - x[None, :]) ** 2
        d += (y[s:e, None] - y[None, :]) ** 2
        d += (z[s:e, None] - z[None, :]) ** 2
        d[torch.arange(e - s, device=pts.device), torch.arange(s, e, device=pts.device)] = float("inf")
        out[s:e] = d.topk(3, dim=1, largest=False).values.sum(dim=1) / 3.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="100000,1000000,5000000")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_bench.txt"))
    args = ap.parse_args()
    import torch
    from splat_renderer_amd import _lib
    from splat_renderer_amd import autograd as AG
    if not torch.cuda.is_available():
        raise SystemExit("knn_bench: no GPU (there is no CPU path to time)")
    sizes = [int(s) for s in args.sizes.split(",")]
    lines = [f"# tools/knn_bench.py --sizes {args.sizes} --rounds {args.rounds}: {torch.cuda.get_device_name(0)}; median (min to max) of {args.rounds} calls "
             "between device events, 2 warm-up calls; sort share from SPLAT_STAGE_SORT in a separate timed pass",
             "# scene n | ms per call | Mpoints/s | evaluations per query (brute force n - 1) | sort ms (share of that pass's call)"]
    cx = AG._context(torch.empty(4, device="cuda"))
    lib, ctx = cx.lib, cx.ctx
    for n in sizes:
        cx.ensure_sorter(n)
        nbytes = int(lib.splat_knn_workspace_bytes(n))
        ws = torch.empty(nbytes // 4, device="cuda", dtype=torch.int32)
        out = torch.empty(n, device="cuda")
        ev = torch.zeros((), device="cuda", dtype=torch.int64)
        for scene in ("cube", "sphere", "outliers"):
            pts = torch.from_numpy(make(scene, n)).cuda()

            def call():
                _lib.check(lib.splat_knn_mean_sq(ctx, cx.sorter, pts.data_ptr(), 3, n, ws.data_ptr(), nbytes, out.data_ptr(), ev.data_ptr()), ctx)
            for _ in range(2):
                call()
            torch.cuda.synchronize()
            times = []
            for _ in range(args.rounds):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                call()
                b.record()
                b.synchronize()
                times.append(a.elapsed_time(b))
            evals = int(ev)
            assert bool(torch.isfinite(out).all())
            # the sort's share: the same call with the context's stage events on, SORT only
            _lib.check(lib.splat_set_timing_stages(ctx, 1 << _lib.STAGE_SORT), ctx)
            _lib.check(lib.splat_set_timing(ctx, 1), ctx)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            call()
            b.record()
            b.synchronize()
            samples, total = C.c_uint32(), C.c_double()
            _lib.check(lib.splat_stage_time_stats(ctx, _lib.STAGE_SORT, C.byref(samples), C.byref(total)), ctx)
            _lib.check(lib.splat_set_timing(ctx, 0), ctx)
            _lib.check(lib.splat_set_timing_stages(ctx, 0xFFFFFFFF), ctx)
            whole = a.elapsed_time(b)
            med = float(np.median(times))
            line = (f"{scene:9s} {n:8d} | {med:8.3f} ms ({min(times):.3f} to {max(times):.3f}) | {n / med / 1e3:8.1f} | {evals / n:8.1f} ({n - 1}) | "
                    f"{total.value:.3f} ms in {samples.value} passes ({100.0 * total.value / whole:.0f} % of {whole:.3f} ms)")
            print(line, flush=True)
            lines.append(line)
            del pts
    n = sizes[0]
    pts = torch.from_numpy(make("cube", n)).cuda()
    want = AG.knn_mean_sq_distance(pts)
    torch_brute_force(torch, pts)
    torch.cuda.synchronize()
    times = []
    for _ in range(3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        got = torch_brute_force(torch, pts)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    rel = float(((got - want).abs() / want).max())
    line = (f"torch brute force, cube {n}: {float(np.median(times)):.1f} ms ({min(times):.1f} to {max(times):.1f}; chunks of 2 048 queries, 3 calls); "
            f"max relative difference from splat_knn_mean_sq {rel:.2g}")
    print(line, flush=True)
    lines.append(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
