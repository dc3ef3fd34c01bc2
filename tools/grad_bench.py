#!/usr/bin/env python3
"""Gradients of ellipsoid frames (GPU box only): python tools/grad_bench.py [--depth] [--deterministic] [--antialiased] [--importance] [--absgrad] [--features K[,K]] [--surfel [--distortion]] [--camera | --loss | --optimizer] [C1,C2] [K] [R]

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
bytes then count 40 per consumed pair (the tenth sum, dL/dz).

--deterministic adds the fixed-order composite backward beside the atomic one, alternating in the same rounds:
splat_composite_backward_det alone (composite_backward_det; with --depth also its depth variant) - all of its launches: the
rectangle count, its scan, the tile kernel storing to the slots, the gather - and the whole frame's backward with
rasterize(..., deterministic=True) (backward_det); their ratios to the atomic path; the workspace bytes; the slots the tile
kernel wrote (the sum of the tile table's largest L, read back from the workspace) and the time the gather's bytes - every
written slot once out and once in, 36 or 40 B each, plus the 16 B table rows - take at the 5.1 TB/s copy rate.

--antialiased adds the antialiased mode beside the classic one, alternating in the same rounds: the staged forward with
project_ellipsoids(antialiased=True) and the opacity column times rho (forward_aa), its backward (backward_aa), and
splat_project_ellipsoid_backward_aa alone with a random grad_rho and no camera sums (project_backward_aa) beside
splat_project_ellipsoid_backward; their ratios to the classic path.

--importance adds the per-splat contribution pass beside the composite backward, alternating in the same rounds:
splat_composite_contribution alone with all three outputs and no mask (composite_contribution: hit count, largest and summed
blend weight per splat, integer atomics), and the one thing the library offered for the summed weight before it,
splat_composite_backward with an upstream of ones in (r, g, b) and zero in alpha, whose colour column is that sum
(composite_backward_ones: two walks, nine float sums per entry, float atomics); their ratio.

--absgrad adds AbsGS's absolute screen-space gradient beside the plain backward, alternating in the same rounds:
splat_composite_backward_abs alone, colour only (composite_backward_abs: the two extra wave sums per entry and their atomics
into the n x 2 plane), with --depth also its depth variant (composite_backward_abs_depth), with --deterministic also
splat_composite_backward_det_abs over its own, larger workspace (composite_backward_det_abs, and _depth with both), and the
whole frame's backward with rasterize(..., absgrad=True) (backward_abs; with --deterministic backward_det_abs); each one's
ratio to the entry point without the absolute sums, timed in the same rounds; the det workspaces' bytes.

--features K[,K...] (3,8 is what profiles/features_bench.txt holds) adds the feature channels beside the kernels they are walks
of, alternating in the same rounds, per K: splat_composite_features alone on K random floats per splat
(composite_features_K) beside its one-walk peer splat_composite_contribution with all three outputs
(composite_contribution), and splat_composite_features_backward alone with a random upstream map
(composite_features_backward_K: two walks, 6 + K float sums per entry, float atomics) beside its two-walk peer
splat_composite_backward (composite_backward: 9 sums); their ratios.

--surfel adds 2D Gaussian surfels beside the ellipsoid, alternating in the same rounds, on the same planes read as surfels (scales
x and y, the same quaternions): the staged forward with render_surfels' calls (forward_surfel: project_surfels, SH colour, sort,
bin, composite) and its backward (backward_surfel); with --depth the forward with the intersection depth map
(forward_surfel_depth: one more walk, splat_composite_surfel_depth) and its backward; splat_composite_backward(_depth) alone with
cfg.footprint = SURFEL over the surfel frame's own lists (composite_backward_surfel(_depth): 12 or 13 wave sums per entry against
9 or 10, and one rcp per pair), splat_composite_surfel_depth alone (surfel_depth_forward) and splat_project_surfel_backward alone
with a random grad_clip_w (project_backward_surfel); each one's ratio to its ellipsoid peer, and the surfel frame's own pairs.
--surfel --distortion (implies --depth) adds the depth-distortion map in the same rounds: the staged forward with the map
(forward_surfel_distortion: splat_composite_surfel_distortion in place of splat_composite_surfel_depth) beside
forward_surfel_depth and its backward (backward_surfel_distortion); the two entry points alone (surfel_distortion_forward beside
surfel_depth_forward; composite_backward_surfel_distortion, the one fused launch with all three upstreams, beside
composite_backward_surfel_depth); and, for context, what the centre-depth recipe costs on the same lists: splat_composite_features
and its backward with K = 3 under the surfel footprint (surfel_features_3, surfel_features_backward_3), whose sum with
composite_backward_surfel_depth is centre_recipe_backward_ms.  fused_backward_over_depth_ms is what the map adds to the depth
backward; a second replay of the lists would add surfel_features_backward_3_ms.

--camera adds the camera gradients: splat_project_ellipsoid_backward_camera without and with grad_depth (all of its launches:
the per-splat kernel with the per-wave sums, then k_camera_sum_slices above 1024 partials, then k_camera_sum) beside
splat_project_ellipsoid_backward(_depth), whose kernels are the parent commit's instruction for instruction;
splat_sh_colors_backward_camera beside splat_sh_colors_backward; the alternative the fused sums replace, twice, each once per
round: project_backward plus the twelve per-splat terms written out as plain float32 torch ops without autograd and summed
(project_backward_plus_torch_terms: the kernel has no output for gJ, gcx, gcy, gcw, so the expression recomputes J, T, Sigma2
and their gradients per splat), and, as an upper bound, project_backward plus a torch restatement of the whole record function
differentiated by torch.autograd (project_backward_plus_torch_sum); and the whole frame's forward and backward with the
uniform block as a CUDA tensor that requires grad (forward_camera, backward_camera) beside the
NumPy block's (forward, backward).  Ratios camera / plain are printed per pair.

--loss measures the image loss instead (one JSON line per config, nothing of the above): splat_image_loss and
splat_image_loss_backward alone on the frame's own rgb (the stride-4 view rasterize returns) and a packed target
(fused_loss_forward, fused_loss_backward); the route they replace on the same tensors, written out below (torch_loss: float32
conv2d with the 11 x 11 window over three groups, five maps, and the .contiguous() conv2d needs of that view; forward, and
its torch.autograd backward); the whole frame's forward + backward with each of the two losses (frame_fused, frame_torch);
and the bytes each fused kernel must move (forward: x at 16 B and y at 12 B per pixel read, 36 B of derivative maps written;
backward: the same reads, the maps read, 12 B of gradient written) with the time they take at 5.1 TB/s, the copy rate
DESIGN.md uses.

--optimizer measures the optimiser step and density control instead (one JSON line per config, nothing of the above), on the
raw parameters of a fit (means, log-scales, rotations, opacity logits, SH of degree 3: 59 floats per splat) with the gradients
and the visibility mask of one real frame: torch.optim.Adam(foreach=True) and torch.optim.Adam(fused=True) over the five
tensors (one rate per tensor: torch cannot give the SH plane two without splitting it), five splat_adam_step launches dense
and the same five masked with the frame's visibility, alternating in one process; per contender the bytes it moves by the
28 B-per-parameter count (the masked step: that count over the visible rows, plus the mask) and the share of the 5.1 TB/s copy
rate that is; and splat_density_accumulate, splat_densify_plan (with its one synchronisation: a host clock around it) and the
apply pass (splat_densify_geometry, three COPY and ten ZERO_NEW splat_densify_rows) at 3DGS's default thresholds; and the three
MCMC kernels on the same cloud: splat_mcmc_noise (the per-step one: 56 B per splat, its GB/s beside a device-to-device copy of the
same planes timed in the same rounds, the line's measured copy ceiling), splat_mcmc_sample in relocate mode (host clock: it
synchronises) and splat_mcmc_apply of that sample, on logits drawn N(-1, 2.5), 4 % of them below min_opacity = 0.005 (the bench
scene itself is opaque).

--surfel --optimizer measures the three surfel entry points of density control instead (one JSON line per config, nothing of the
above): a GaussianFit and a SurfelFit of the same cloud (the surfel takes the first two scales) each render one frame and take its
backward, and then splat_density_accumulate_surfel, splat_densify_plan_surfel (host clock: it synchronises) and
splat_densify_geometry_surfel run beside their ellipsoid peers on the same n, alternating in the same rounds, as do the two
fits' whole step() (the statistics and the five Adam launches on the frame's gradients, restored before every call) and each of
its five masked splat_adam_step launches alone (adam_<plane>_<kind>: which plane a difference between the two steps comes from).

--normal-loss measures the normal-consistency term instead (one JSON line per config, nothing of the above), on the frame's own
depth map, blended normal map (render_gaussians(return_depth=True, features=splat_normals(...)): a packed (H, W, 3) image) and
alpha as the weight: splat_normal_consistency (both launches) and splat_normal_consistency_backward alone (fused_normal_forward,
fused_normal_backward); the same term written in float32 torch ops on the same tensors, below (torch_normal_loss: 2DGS's
depth_to_normal with the ray directions and 1 / |d| precomputed outside the timed region; forward, and its torch.autograd
backward), alternating in the same rounds; and the bytes each fused kernel must move (forward: 4 B of depth, 12 B of map and 4 B
of weight read per pixel; backward: the same reads, 12 B of map gradient and 4 B of depth gradient written) with the time they
take at 5.1 TB/s and the rate each achieves."""
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

def torch_camera_terms(U, pos, scl, rot, g, W, H):
    """dL/dVP's twelve entries (column k = 0..3, rows 0, 1, 3: index 3 k + {0, 1, 2}) for dL/d{c.x, c.y, B00, B01, B11} = g (n, 5):
    k_project_ellipsoid_backward's per-splat terms written out as plain float32 torch ops, without autograd, and summed (no cull)."""
    q = rot / torch.sqrt((rot * rot).sum(dim=1, keepdim=True))
    qr, qx, qy, qz = q.unbind(1)
    R = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qr * qz), 2 * (qx * qz + qr * qy)],
         [2 * (qx * qy + qr * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qr * qx)],
         [2 * (qx * qz - qr * qy), 2 * (qy * qz + qr * qx), 1 - 2 * (qx * qx + qy * qy)]]
    M = [[R[i][j] * scl[:, j] for j in range(3)] for i in range(3)]
    p = [pos[:, 0], pos[:, 1], pos[:, 2]]
    cx, cy, cw = (U[r] * p[0] + U[4 + r] * p[1] + U[8 + r] * p[2] + U[12 + r] for r in (0, 1, 3))
    nx, ny = cx / cw, cy / cw
    ax, ay = 0.5 * W / cw, 0.5 * H / cw
    dj0 = [U[4 * k] - nx * U[4 * k + 3] for k in range(3)]
    dj1 = [ny * U[4 * k + 3] - U[4 * k + 1] for k in range(3)]
    t0 = [sum(ax * dj0[k] * M[k][c] for k in range(3)) for c in range(3)]
    t1 = [sum(ay * dj1[k] * M[k][c] for k in range(3)) for c in range(3)]
    A = t0[0] * t0[0] + t0[1] * t0[1] + t0[2] * t0[2] + 0.3
    B = t0[0] * t1[0] + t0[1] * t1[1] + t0[2] * t1[2]
    Cc = t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2] + 0.3
    det = A * Cc - B * B
    b00, b01, b11 = torch.sqrt(Cc / det) / 3, -B / torch.sqrt(Cc * det) / 3, 1 / torch.sqrt(Cc) / 3
    gdet = -(g[:, 2] * b00 + g[:, 3] * b01) / (2 * det)
    gC = (g[:, 2] * b00 - g[:, 3] * b01 - g[:, 4] * b11) / (2 * Cc) + gdet * A
    gA = gdet * Cc
    gB = g[:, 3] * (-1 / (3 * torch.sqrt(Cc * det))) - 2 * B * gdet
    gt0 = [2 * gA * t0[c] + gB * t1[c] for c in range(3)]
    gt1 = [2 * gC * t1[c] + gB * t0[c] for c in range(3)]
    gj0 = [sum(gt0[c] * M[k][c] for c in range(3)) for k in range(3)]
    gj1 = [sum(gt1[c] * M[k][c] for c in range(3)) for k in range(3)]
    gax = sum(gj0[k] * dj0[k] for k in range(3))
    gay = sum(gj1[k] * dj1[k] for k in range(3))
    gnx = 0.5 * W * g[:, 0] - sum(gj0[k] * ax * U[4 * k + 3] for k in range(3))
    gny = -0.5 * H * g[:, 1] + sum(gj1[k] * ay * U[4 * k + 3] for k in range(3))
    gcx, gcy = gnx / cw, gny / cw
    gcw = -(gax * ax + gay * ay) / cw - (gnx * nx + gny * ny) / cw
    terms = []
    for k in range(3):
        terms += [gcx * p[k] + gj0[k] * ax, gcy * p[k] - gj1[k] * ay, gcw * p[k] + (gj1[k] * ay * ny - gj0[k] * ax * nx)]
    terms += [gcx, gcy, gcw]
    return torch.stack(terms, dim=1).sum(dim=0)


feature_ks = []
if "--features" in sys.argv[1:]:
    at = sys.argv.index("--features")
    feature_ks = [int(v) for v in sys.argv[at + 1].split(",")]
    del sys.argv[at:at + 2]
argv = [a for a in sys.argv[1:] if a not in ("--depth", "--camera", "--loss", "--normal-loss", "--optimizer", "--deterministic", "--antialiased", "--importance", "--absgrad", "--surfel", "--distortion")]
surfel_too = "--surfel" in sys.argv[1:]
abs_too = "--absgrad" in sys.argv[1:]
aa_too = "--antialiased" in sys.argv[1:]
importance_too = "--importance" in sys.argv[1:]
det_too = "--deterministic" in sys.argv[1:]
optimizer_only = "--optimizer" in sys.argv[1:]
dist_too = "--distortion" in sys.argv[1:] and surfel_too
depth_too = "--depth" in sys.argv[1:] or dist_too
DIST_RANGE = (0.2, 100.0)  # near, far of the distortion map's depth mapping
camera_too = "--camera" in sys.argv[1:]
loss_only = "--loss" in sys.argv[1:]
normal_loss_only = "--normal-loss" in sys.argv[1:]
COPY_RATE = 5.1e12  # bytes / s, read + write: the box's device-to-device copy rate


def torch_loss(rgb, target, lam=0.2):
    """(1 - lam) L1 + lam (1 - SSIM) in float32 torch ops: what a user wrote before the fused kernel."""
    import torch.nn.functional as F
    kk = torch.arange(11, device=rgb.device, dtype=torch.float32)
    g = torch.exp(-((kk - 5) ** 2) / (2 * 1.5 ** 2))
    g = g / g.sum()
    k2 = torch.outer(g, g)[None, None].expand(3, 1, -1, -1).contiguous()
    a, b = rgb.contiguous().permute(2, 0, 1)[None], target.permute(2, 0, 1)[None]
    conv = lambda t: F.conv2d(t, k2, padding=5, groups=3)  # noqa: E731
    mx, my = conv(a), conv(b)
    sx, sy, sxy = conv(a * a) - mx * mx, conv(b * b) - my * my, conv(a * b) - mx * my
    m = ((2 * mx * my + 1e-4) * (2 * sxy + 9e-4)) / ((mx * mx + my * my + 1e-4) * (sx + sy + 9e-4))
    return (1 - lam) * (a - b).abs().mean() + lam * (1 - m.mean())


def loss_bench(name, k, rounds, stream):
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

    def frame():
        rec, aux = AG.project_ellipsoids(u, means, scales, rots)
        col = AG.sh_colors(u[16:19], means, shs, 3, ops)
        return AG.rasterize(rec, col, aux, w, h)[0]

    with torch.no_grad():
        rgb = frame()  # (the (H, W, 3) view of an (H, W, 4) buffer)
    target = (rgb + 0.1 * torch.randn_like(rgb)).clamp(0, 1).contiguous()
    x = rgb.detach().requires_grad_()
    cx = AG._context(rgb)
    lib = cx.lib
    nbytes = int(lib.splat_image_loss_workspace_bytes(w, h))
    ws, out4, up = torch.empty(nbytes // 4, device="cuda"), torch.empty(4, device="cuda"), torch.ones(1, device="cuda")
    grad = torch.empty((h, w, 3), device="cuda")
    state = {}

    def frame_with(loss_fn):
        def go():
            state["loss"] = loss_fn(frame(), target)
            state["loss"].backward()
        return go

    def torch_forward():
        state["loss"] = torch_loss(x, target)

    work = {
        "fused_loss_forward": lambda: lib.splat_image_loss(cx.ctx, rgb.data_ptr(), 4, target.data_ptr(), 3, w, h, 0.2, ws.data_ptr(), nbytes,
                                                           out4.data_ptr()),
        "fused_loss_backward": lambda: lib.splat_image_loss_backward(cx.ctx, rgb.data_ptr(), 4, target.data_ptr(), 3, w, h, 0.2, ws.data_ptr(),
                                                                     nbytes, up.data_ptr(), grad.data_ptr(), 3),
        "torch_loss_forward": torch_forward,
        "torch_loss_backward": None,  # (a forward, then its backward alone)
        "frame_fused": frame_with(AG.photometric_loss),
        "frame_torch": frame_with(torch_loss),
    }

    def run(kind, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if kind == "torch_loss_backward":
            tot = 0.0
            for _ in range(calls):
                torch_forward()
                x.grad = None
                e0.record(stream)
                state["loss"].backward()
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
    fwd_bytes, bwd_bytes = (16 + 12 + 36) * w * h, (16 + 12 + 36 + 12) * w * h
    fused, torch_ms = med["fused_loss_forward"] + med["fused_loss_backward"], med["torch_loss_forward"] + med["torch_loss_backward"]
    print(json.dumps({"config": name, "n": n, "width": w, "height": h, "calls_per_round": k, "rounds": rounds,
                      **{f"{kind}_ms": round(v, 4) for kind, v in med.items()},
                      **{f"{kind}_ms_min_max": [round(min(v), 4), round(max(v), 4)] for kind, v in ts.items()},
                      "fused_loss_ms": round(fused, 4), "torch_loss_ms": round(torch_ms, 4), "torch_over_fused": round(torch_ms / fused, 2),
                      "frame_torch_over_frame_fused": round(med["frame_torch"] / med["frame_fused"], 3),
                      "fused_forward_bytes": fwd_bytes, "fused_forward_floor_ms": round(fwd_bytes / COPY_RATE * 1e3, 4),
                      "fused_forward_over_floor": round(med["fused_loss_forward"] / (fwd_bytes / COPY_RATE * 1e3), 2),
                      "fused_backward_bytes": bwd_bytes, "fused_backward_floor_ms": round(bwd_bytes / COPY_RATE * 1e3, 4),
                      "fused_backward_over_floor": round(med["fused_loss_backward"] / (bwd_bytes / COPY_RATE * 1e3), 2)}), flush=True)


def torch_normal_loss(nmap, depth, weight, d, inv_len, sigma):
    """mean(1 - w F . N(depth)) in float32 torch ops: 2DGS's depth_to_normal (points along the rays, central differences, cross
    product, normalise) and its normal_error.mean(), with the validity rule of include/splat.h.  d (H, W, 3) and inv_len (H, W)
    are the camera's rays and 1 / |d|."""
    import torch.nn.functional as F
    ok = torch.isfinite(depth) & (depth > 0)
    pts = (torch.where(ok, depth, torch.ones_like(depth)) * inv_len)[..., None] * d
    ax = pts[1:-1, 2:] - pts[1:-1, :-2]
    ay = pts[2:, 1:-1] - pts[:-2, 1:-1]
    valid = ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1]
    n = sigma * torch.linalg.cross(ay, ax)
    nn = (n * n).sum(dim=2)
    valid = valid & torch.isfinite(nn) & (nn > 0)
    N = torch.where(valid[..., None], n / torch.sqrt(torch.where(valid, nn, torch.ones_like(nn)))[..., None], torch.zeros_like(n))
    N = F.pad(N.permute(2, 0, 1), (1, 1, 1, 1)).permute(1, 2, 0)
    return (1.0 - weight * (nmap * N).sum(dim=2)).mean()


def normal_loss_bench(name, k, rounds, stream):
    n, w, h = sr.scene.CONFIGS[name]
    props, _ = sr.scene.make_scene(n)
    rng = np.random.default_rng(0)
    scl = (props[:, 3:4] * 0.5 * np.exp(rng.uniform(-0.3, 0.3, (n, 3)))).astype(np.float32)
    rot = rng.normal(size=(n, 4)).astype(np.float32)
    cam = sr.Camera()
    cam.setAspect(w / h)
    u = cam.uniforms(w, h)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")  # noqa: E731
    means, scales, rots, ops, cols = t(props[:, :3]), t(scl), t(rot), t(props[:, 7]), t(props[:, 4:7])
    with torch.no_grad():
        _, alpha, depth, nmap = AG.render_gaussians(u, means, scales, rots, ops, colors=cols, width=w, height=h, return_depth=True,
                                                    features=AG.splat_normals(means, scales, rots, u[16:19]))
    depth, nmap, alpha = depth.contiguous(), nmap.contiguous(), alpha.contiguous()
    rays = (C.c_double * 10)()
    _lib.check(_lib.load().splat_camera_rays(AG._fptr(u), rays))
    r = np.array(rays[:])
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    d64 = r[0:3] + xs[..., None] * r[3:6] + ys[..., None] * r[6:9]
    d, inv_len, sigma = t(d64), t(1.0 / np.linalg.norm(d64, axis=2)), float(r[9])
    cx = AG._context(depth)
    lib = cx.lib
    out4, up = torch.empty(4, device="cuda"), torch.ones(1, device="cuda")
    gmap, gz = torch.empty((h, w, 3), device="cuda"), torch.empty((h, w), device="cuda")
    zt, ft = depth.clone().requires_grad_(), nmap.clone().requires_grad_()
    state = {}
    head = (cx.ctx, AG._fptr(u), _lib.DEPTH_DISTANCE, depth.data_ptr(), nmap.data_ptr(), 3, alpha.data_ptr(), w, h)

    def torch_forward():
        state["loss"] = torch_normal_loss(ft, zt, alpha, d, inv_len, sigma)

    work = {
        "fused_normal_forward": lambda: lib.splat_normal_consistency(*head, out4.data_ptr()),
        "fused_normal_backward": lambda: lib.splat_normal_consistency_backward(*head, up.data_ptr(), gmap.data_ptr(), 3, gz.data_ptr()),
        "torch_normal_forward": torch_forward,
        "torch_normal_backward": None,  # (a forward, then its backward alone)
    }

    def run(kind, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if kind == "torch_normal_backward":
            tot = 0.0
            for _ in range(calls):
                torch_forward()
                zt.grad = ft.grad = None
                e0.record(stream)
                state["loss"].backward()
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
    # the two routes compute the same term: the fused loss beside the torch one, and the largest gradient difference
    work["fused_normal_forward"]()
    work["fused_normal_backward"]()
    torch_forward()
    zt.grad = ft.grad = None
    state["loss"].backward()
    agree = {"fused_loss": float(out4[0]), "torch_loss": float(state["loss"].detach()), "valid_fraction": float(out4[1]),
             "max_abs_dmap_difference": float((gmap - ft.grad).abs().max()), "max_abs_dmap": float(gmap.abs().max()),
             "max_abs_ddepth_difference": float((gz - zt.grad).abs().max()), "max_abs_ddepth": float(gz.abs().max())}
    ts = {kind: [] for kind in work}
    for _ in range(rounds):
        for kind in work:
            ts[kind].append(run(kind, k))
    med = {kind: sorted(v)[len(v) // 2] for kind, v in ts.items()}
    fwd_bytes, bwd_bytes = (4 + 12 + 4) * w * h, (4 + 12 + 4 + 12 + 4) * w * h
    fused, torch_ms = med["fused_normal_forward"] + med["fused_normal_backward"], med["torch_normal_forward"] + med["torch_normal_backward"]
    print(json.dumps({"config": name, "n": n, "width": w, "height": h, "calls_per_round": k, "rounds": rounds,
                      **{f"{kind}_ms": round(v, 4) for kind, v in med.items()},
                      **{f"{kind}_ms_min_max": [round(min(v), 4), round(max(v), 4)] for kind, v in ts.items()},
                      "fused_normal_ms": round(fused, 4), "torch_normal_ms": round(torch_ms, 4), "torch_over_fused": round(torch_ms / fused, 2),
                      "fused_forward_bytes": fwd_bytes, "fused_forward_floor_ms": round(fwd_bytes / COPY_RATE * 1e3, 4),
                      "fused_forward_GBps": round(fwd_bytes / med["fused_normal_forward"] * 1e-6, 1),
                      "fused_forward_over_floor": round(med["fused_normal_forward"] / (fwd_bytes / COPY_RATE * 1e3), 2),
                      "fused_backward_bytes": bwd_bytes, "fused_backward_floor_ms": round(bwd_bytes / COPY_RATE * 1e3, 4),
                      "fused_backward_GBps": round(bwd_bytes / med["fused_normal_backward"] * 1e-6, 1),
                      "fused_backward_over_floor": round(med["fused_normal_backward"] / (bwd_bytes / COPY_RATE * 1e3), 2), **agree}), flush=True)


def optimizer_bench(name, k, rounds, stream):
    import time
    from splat_renderer_amd.fit import DEFAULT_LR, PLANES, GaussianFit
    n, w, h = sr.scene.CONFIGS[name]
    props, _ = sr.scene.make_scene(n)
    rng = np.random.default_rng(0)
    scl = (props[:, 3:4] * 0.5 * np.exp(rng.uniform(-0.3, 0.3, (n, 3)))).astype(np.float32)
    rot = rng.normal(size=(n, 4)).astype(np.float32)
    sh = rng.normal(0, 0.3, (n, 16, 3)).astype(np.float32)
    cam = sr.Camera()
    cam.setAspect(w / h)
    u = cam.uniforms(w, h)
    fit = GaussianFit(props[:, :3], scl, rot, np.clip(props[:, 7], 1e-4, 1 - 1e-4), sh)
    target = torch.rand((h, w, 3), device="cuda")
    rgb, _ = fit.render(u, w, h)
    AG.photometric_loss(rgb, target).backward()
    rec, _, _ = fit._frame
    grec = rec.grad.contiguous()
    grads = {p: getattr(fit, p).grad.contiguous() for p in PLANES}
    cx = AG._context(fit.means)
    lib = cx.lib
    ga, dn, mr = (torch.zeros(n, device="cuda") for _ in range(3))
    vis = torch.zeros(n, device="cuda", dtype=torch.uint8)

    def accumulate():
        _lib.check(lib.splat_density_accumulate(cx.ctx, rec.data_ptr(), grec.data_ptr(), n, w, h, ga.data_ptr(), dn.data_ptr(), mr.data_ptr(),
                                                vis.data_ptr()), cx.ctx)
    accumulate()
    visible = float(vis.float().mean())
    params = sum(g.numel() for g in grads.values())
    visible_params = int(visible * n + 0.5) * 59

    def copies():
        return {p: getattr(fit, p).detach().clone() for p in PLANES}
    sets = {}
    for kind, kw in (("torch_foreach", dict(foreach=True)), ("torch_fused", dict(fused=True))):
        ps = copies()
        for p in PLANES:
            ps[p].requires_grad_()
            ps[p].grad = grads[p]
        sets[kind] = torch.optim.Adam([{"params": [ps[p]], "lr": DEFAULT_LR[p]} for p in PLANES], eps=1e-15, **kw)
    ours = copies()
    m, v = {p: torch.zeros_like(ours[p]) for p in PLANES}, {p: torch.zeros_like(ours[p]) for p in PLANES}
    t = {"step": 0}

    def splat_step(mask):
        t["step"] += 1
        bc1, isbc2 = 1.0 - 0.9 ** t["step"], 1.0 / (1.0 - 0.999 ** t["step"]) ** 0.5
        for p in PLANES:
            fpr = ours[p].shape[1] if ours[p].dim() == 2 else 1
            _lib.check(lib.splat_adam_step(cx.ctx, ours[p].data_ptr(), grads[p].data_ptr(), m[p].data_ptr(), v[p].data_ptr(), n, fpr,
                                           3 if p == "sh" else fpr, DEFAULT_LR[p] / bc1, DEFAULT_LR["sh_rest" if p == "sh" else p] / bc1, 0.9, 0.999,
                                           isbc2, 1e-15, mask), cx.ctx)

    cfg = _lib.DensifyCfg(2e-4, 0.01 * fit.extent, 0.005, 0.0, 0.0, 0, 1)
    nbytes = int(lib.splat_densify_plan_workspace_bytes(n))
    ws = torch.empty(nbytes // 4, device="cuda", dtype=torch.int32)
    rows = torch.empty(2 * n, device="cuda", dtype=torch.int32)
    n_out, counts = C.c_uint32(), (C.c_uint32 * 4)()

    def plan():
        _lib.check(lib.splat_densify_plan(cx.ctx, fit.log_scales.data_ptr(), fit.opacity_logits.data_ptr(), ga.data_ptr(), dn.data_ptr(),
                                          mr.data_ptr(), n, C.byref(cfg), ws.data_ptr(), nbytes, rows.data_ptr(), C.byref(n_out), counts), cx.ctx)
    plan()
    kout = int(n_out.value)
    outs = {p: torch.empty((kout,) + tuple(ours[p].shape[1:]), device="cuda") for p in PLANES}

    def apply():
        _lib.check(lib.splat_densify_geometry(cx.ctx, rows.data_ptr(), kout, ours["means"].data_ptr(), ours["log_scales"].data_ptr(),
                                              ours["rotations"].data_ptr(), C.byref(cfg), outs["means"].data_ptr(), outs["log_scales"].data_ptr()),
                   cx.ctx)
        for p in PLANES:
            fpr = ours[p].shape[1] if ours[p].dim() == 2 else 1
            if p in PLANES[2:]:
                _lib.check(lib.splat_densify_rows(cx.ctx, rows.data_ptr(), kout, ours[p].data_ptr(), outs[p].data_ptr(), fpr, 0), cx.ctx)
            for mom in (m, v):
                _lib.check(lib.splat_densify_rows(cx.ctx, rows.data_ptr(), kout, mom[p].data_ptr(), outs[p].data_ptr(), fpr, 1), cx.ctx)

    # MCMC: the per-step noise, a relocation of the 3 % most transparent splats, and a plain copy of the noise's planes as the ceiling
    # (the bench scene is opaque: the MCMC kernels get logits of their own, N(-1, 2.5), of which 4 % are below min_opacity = 0.005)
    mcmc_min_opacity = 0.005
    mlogits = torch.randn(n, device="cuda", generator=torch.Generator(device="cuda").manual_seed(2)) * 2.5 - 1.0
    alogits = mlogits.clone()  # (the apply's own: it rewrites the drawn sources' logits at every call)
    mws_bytes = int(lib.splat_mcmc_sample_workspace_bytes(n))
    mws = torch.empty(mws_bytes // 4, device="cuda", dtype=torch.int32)
    mt, ms, mc = (torch.empty(n, device="cuda", dtype=torch.int32) for _ in range(3))
    mwords = (C.c_uint32 * 3)()
    mpl = _lib.McmcPlanes()
    for i, p in enumerate(PLANES):
        mpl.param[i], mpl.m[i], mpl.v[i] = (alogits if p == "opacity_logits" else ours[p]).data_ptr(), m[p].data_ptr(), v[p].data_ptr()
    mpl.sh_floats = ours["sh"].shape[1]
    noise_step = {"t": 0}

    def mcmc_sample():
        _lib.check(lib.splat_mcmc_sample(cx.ctx, mlogits.data_ptr(), n, _lib.MCMC_RELOCATE, 0, mcmc_min_opacity, 1, mws.data_ptr(),
                                         mws_bytes, mt.data_ptr(), ms.data_ptr(), mc.data_ptr(), mwords), cx.ctx)
    mcmc_sample()
    mcmc_draws, mcmc_counts = int(mwords[2]), {"dead": int(mwords[0]), "alive": int(mwords[1]), "draws": int(mwords[2])}

    def mcmc_apply():  # (in place on the bench's own copies: the same rows every call)
        _lib.check(lib.splat_mcmc_apply(cx.ctx, mt.data_ptr(), ms.data_ptr(), mc.data_ptr(), n, mcmc_draws, n, mcmc_min_opacity, C.byref(mpl)), cx.ctx)

    def mcmc_noise():
        noise_step["t"] += 1
        _lib.check(lib.splat_mcmc_noise(cx.ctx, ours["means"].data_ptr(), ours["log_scales"].data_ptr(), ours["rotations"].data_ptr(),
                                        mlogits.data_ptr(), n, 5e5 * DEFAULT_LR["means"], noise_step["t"], 1), cx.ctx)
    copy_src = torch.empty(14 * n, device="cuda")  # 56 B per splat: as much read and written as the noise reads and writes
    copy_dst = torch.empty_like(copy_src)

    def copy_planes():
        copy_dst[:7 * n].copy_(copy_src[:7 * n])  # 28 B read + 28 B written per splat

    work = {"mcmc_noise": mcmc_noise, "copy56": copy_planes, "mcmc_apply": mcmc_apply, "torch_foreach": sets["torch_foreach"].step, "torch_fused": sets["torch_fused"].step, "splat_dense": lambda: splat_step(None),
            "splat_masked": lambda: splat_step(vis.data_ptr()), "accumulate": accumulate, "apply": apply}

    def run(kind, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            work[kind]()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    def run_host(fn, calls):  # (it synchronises: a host clock, the stream idle before and after)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        return (time.perf_counter() - t0) * 1e3 / calls

    def run_plan(calls):
        return run_host(plan, calls)

    for kind in list(work) * 2:
        run(kind, 3)
    run_plan(3)
    run_host(mcmc_sample, 3)
    ts = {kind: [] for kind in list(work) + ["plan", "mcmc_sample"]}
    for _ in range(rounds):
        for kind in work:
            ts[kind].append(run(kind, k))
        ts["plan"].append(run_plan(max(k // 4, 1)))
        ts["mcmc_sample"].append(run_host(mcmc_sample, max(k // 4, 1)))
    med = {kind: sorted(x)[len(x) // 2] for kind, x in ts.items()}
    moved = {"torch_foreach": 28 * params, "torch_fused": 28 * params, "splat_dense": 28 * params, "splat_masked": 28 * visible_params + 5 * n}
    print(json.dumps({"config": name, "n": n, "width": w, "height": h, "calls_per_round": k, "rounds": rounds, "parameters": params,
                      "visible_fraction": round(visible, 4),
                      **{f"{kind}_ms": round(x, 4) for kind, x in med.items()},
                      **{f"{kind}_ms_min_max": [round(min(x), 4), round(max(x), 4)] for kind, x in ts.items()},
                      **{f"{kind}_bytes": b for kind, b in moved.items()},
                      **{f"{kind}_share_of_copy_rate": round(b / (med[kind] * 1e-3) / COPY_RATE, 3) for kind, b in moved.items()},
                      "dense_floor_ms": round(28 * params / COPY_RATE * 1e3, 4),
                      "torch_fused_over_splat_dense": round(med["torch_fused"] / med["splat_dense"], 3),
                      "torch_foreach_over_splat_dense": round(med["torch_foreach"] / med["splat_dense"], 3),
                      "splat_dense_over_splat_masked": round(med["splat_dense"] / med["splat_masked"], 3),
                      "mcmc_noise_us": round(med["mcmc_noise"] * 1e3, 2), "mcmc_noise_GBps": round(56 * n / (med["mcmc_noise"] * 1e-3) / 1e9, 1),
                      "copy56_us": round(med["copy56"] * 1e3, 2), "copy56_GBps": round(56 * n / (med["copy56"] * 1e-3) / 1e9, 1),
                      "mcmc_noise_share_of_measured_copy": round(med["copy56"] / med["mcmc_noise"], 3),
                      "splat_dense_GBps": round(28 * params / (med["splat_dense"] * 1e-3) / 1e9, 1),
                      "mcmc_min_opacity": mcmc_min_opacity, "mcmc_counts": mcmc_counts,
                      "mcmc_sample_us": round(med["mcmc_sample"] * 1e3, 1), "mcmc_apply_us": round(med["mcmc_apply"] * 1e3, 2),
                      "plan_counts": {"pruned": counts[0], "kept": counts[1], "cloned": counts[2], "split": counts[3], "rows": kout}}), flush=True)


def surfel_optimizer_bench(name, k, rounds, stream):
    import time
    from splat_renderer_amd.fit import PLANES, GaussianFit, SurfelFit
    n, w, h = sr.scene.CONFIGS[name]
    props, _ = sr.scene.make_scene(n)
    rng = np.random.default_rng(0)
    scl = (props[:, 3:4] * 0.5 * np.exp(rng.uniform(-0.3, 0.3, (n, 3)))).astype(np.float32)
    rot = rng.normal(size=(n, 4)).astype(np.float32)
    sh = rng.normal(0, 0.3, (n, 16, 3)).astype(np.float32)
    cam = sr.Camera()
    cam.setAspect(w / h)
    u = cam.uniforms(w, h)
    opacity = np.clip(props[:, 7], 1e-4, 1 - 1e-4)
    target = torch.rand((h, w, 3), device="cuda")
    fits = {"ellipsoid": GaussianFit(props[:, :3], scl, rot, opacity, sh), "surfel": SurfelFit(props[:, :3], scl[:, :2], rot, opacity, sh)}
    entry = {"ellipsoid": ("splat_density_accumulate", "splat_densify_plan", "splat_densify_geometry"),
             "surfel": ("splat_density_accumulate_surfel", "splat_densify_plan_surfel", "splat_densify_geometry_surfel")}
    cx = AG._context(fits["ellipsoid"].means)
    lib = cx.lib
    work, host, info = {}, {}, {}
    for kind, fit in fits.items():
        rgb, _ = fit.render(u, w, h)
        AG.photometric_loss(rgb, target).backward()
        frame = fit._frame
        rec = frame[0]
        grec = rec.grad.contiguous()
        grads = {p: getattr(fit, p).grad.contiguous() for p in PLANES}
        ga, dn, mr = (torch.zeros(n, device="cuda") for _ in range(3))
        vis = torch.zeros(n, device="cuda", dtype=torch.uint8)
        acc_fn, plan_fn, geo_fn = (getattr(lib, e) for e in entry[kind])

        def accumulate(acc_fn=acc_fn, rec=rec, grec=grec, ga=ga, dn=dn, mr=mr, vis=vis):
            _lib.check(acc_fn(cx.ctx, rec.data_ptr(), grec.data_ptr(), n, w, h, ga.data_ptr(), dn.data_ptr(), mr.data_ptr(), vis.data_ptr()), cx.ctx)
        accumulate()
        cfg = _lib.DensifyCfg(2e-4, 0.01 * fit.extent, 0.005, 0.0, 0.0, 0, 1)
        nbytes = int(lib.splat_densify_plan_workspace_bytes(n))
        ws = torch.empty(nbytes // 4, device="cuda", dtype=torch.int32)
        rows = torch.empty(2 * n, device="cuda", dtype=torch.int32)
        n_out, counts = C.c_uint32(), (C.c_uint32 * 4)()

        def plan(plan_fn=plan_fn, fit=fit, ga=ga, dn=dn, mr=mr, cfg=cfg, ws=ws, nbytes=nbytes, rows=rows, n_out=n_out, counts=counts):
            _lib.check(plan_fn(cx.ctx, fit.log_scales.data_ptr(), fit.opacity_logits.data_ptr(), ga.data_ptr(), dn.data_ptr(), mr.data_ptr(), n,
                               C.byref(cfg), ws.data_ptr(), nbytes, rows.data_ptr(), C.byref(n_out), counts), cx.ctx)
        plan()
        kout = int(n_out.value)
        mu_out = torch.empty((kout, 3), device="cuda")
        ls_out = torch.empty((kout, fit.SCALES), device="cuda")

        def geometry(geo_fn=geo_fn, fit=fit, rows=rows, kout=kout, cfg=cfg, mu_out=mu_out, ls_out=ls_out):
            _lib.check(geo_fn(cx.ctx, rows.data_ptr(), kout, fit.means.data_ptr(), fit.log_scales.data_ptr(), fit.rotations.data_ptr(),
                              C.byref(cfg), mu_out.data_ptr(), ls_out.data_ptr()), cx.ctx)

        def step(fit=fit, frame=frame, grads=grads):  # (the frame and its gradients put back: step() consumes them)
            fit._frame = frame
            for p in PLANES:
                getattr(fit, p).grad = grads[p]
            fit.step()
        work.update({f"accumulate_{kind}": accumulate, f"geometry_{kind}": geometry, f"step_{kind}": step})

        def adam(p, fit=fit, grads=grads, vis=vis):  # (one plane of the step, masked by the frame's visibility, at a fixed step count)
            x = getattr(fit, p)
            fpr = x.shape[1] if x.dim() == 2 else 1
            _lib.check(lib.splat_adam_step(cx.ctx, x.data_ptr(), grads[p].data_ptr(), fit.m[p].data_ptr(), fit.v[p].data_ptr(), n, fpr,
                                           3 if p == "sh" else fpr, fit.lr[p] / 0.1, fit.lr["sh_rest" if p == "sh" else p] / 0.1, 0.9, 0.999,
                                           1.0 / 0.001 ** 0.5, 1e-15, vis.data_ptr()), cx.ctx)
        for p in PLANES:
            work[f"adam_{p}_{kind}"] = lambda p=p, adam=adam: adam(p)
        host[f"plan_{kind}"] = plan
        info[kind] = {"visible_fraction": round(float(vis.float().mean()), 4), "rows": kout,
                      "plan_counts": {"pruned": counts[0], "kept": counts[1], "cloned": counts[2], "split": counts[3]}}

    def run(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for _ in range(calls):
            fn()
        e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / calls

    def run_host(fn, calls):  # (it synchronises: a host clock, the stream idle before and after)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        return (time.perf_counter() - t0) * 1e3 / calls

    for fn in list(work.values()) * 2:
        run(fn, 3)
    for fn in host.values():
        run_host(fn, 3)
    ts = {kind: [] for kind in list(work) + list(host)}
    for _ in range(rounds):
        for kind, fn in work.items():
            ts[kind].append(run(fn, k))
        for kind, fn in host.items():
            ts[kind].append(run_host(fn, max(k // 4, 1)))
    med = {kind: sorted(x)[len(x) // 2] for kind, x in ts.items()}
    print(json.dumps({"config": name, "n": n, "width": w, "height": h, "calls_per_round": k, "rounds": rounds, **info,
                      **{f"{kind}_us": round(x * 1e3, 2) for kind, x in med.items()},
                      **{f"{kind}_us_min_max": [round(min(x) * 1e3, 2), round(max(x) * 1e3, 2)] for kind, x in ts.items()},
                      **{f"{what}_surfel_over_ellipsoid": round(med[f"{what}_surfel"] / med[f"{what}_ellipsoid"], 3)
                         for what in ("accumulate", "plan", "geometry", "step")}}), flush=True)


def torch_records(U, pos, scl, rot, W, H):
    """The records {c.x, c.y, B00, B01, B11} (n, 5) as plain float32 torch ops of the uniform block U (include/splat.h; no cull)."""
    q = rot / torch.sqrt((rot * rot).sum(dim=1, keepdim=True))
    qr, qx, qy, qz = q.unbind(1)
    R = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qr * qz), 2 * (qx * qz + qr * qy)],
         [2 * (qx * qy + qr * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qr * qx)],
         [2 * (qx * qz - qr * qy), 2 * (qy * qz + qr * qx), 1 - 2 * (qx * qx + qy * qy)]]
    M = [[R[i][j] * scl[:, j] for j in range(3)] for i in range(3)]
    cx, cy, cw = (U[r] * pos[:, 0] + U[4 + r] * pos[:, 1] + U[8 + r] * pos[:, 2] + U[12 + r] for r in (0, 1, 3))
    nx, ny = cx / cw, cy / cw
    ax, ay = 0.5 * W / cw, 0.5 * H / cw
    j0 = [ax * (U[4 * k] - nx * U[4 * k + 3]) for k in range(3)]
    j1 = [ay * (ny * U[4 * k + 3] - U[4 * k + 1]) for k in range(3)]
    t0 = [j0[0] * M[0][c] + j0[1] * M[1][c] + j0[2] * M[2][c] for c in range(3)]
    t1 = [j1[0] * M[0][c] + j1[1] * M[1][c] + j1[2] * M[2][c] for c in range(3)]
    a = t0[0] * t0[0] + t0[1] * t0[1] + t0[2] * t0[2] + 0.3
    b = t0[0] * t1[0] + t0[1] * t1[1] + t0[2] * t1[2]
    c = t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2] + 0.3
    det = a * c - b * b
    return torch.stack([(nx + 1) * 0.5 * W, (1 - ny) * 0.5 * H, torch.sqrt(c / det) / 3, -b / torch.sqrt(c * det) / 3, 1 / torch.sqrt(c) / 3], dim=1)


names = argv[0].split(",") if len(argv) > 0 else ["C1", "C2"]
k = int(argv[1]) if len(argv) > 1 else 20
rounds = int(argv[2]) if len(argv) > 2 else 7
stream = torch.cuda.current_stream()
if loss_only:
    for name in names:
        loss_bench(name, k, rounds, stream)
    names = []
if normal_loss_only:
    for name in names:
        normal_loss_bench(name, k, rounds, stream)
    names = []
if optimizer_only:
    for name in names:
        (surfel_optimizer_bench if surfel_too else optimizer_bench)(name, k, rounds, stream)
    names = []
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

    if det_too:
        det_bytes = {d: int(lib.splat_composite_backward_det_workspace_bytes(pairs, tiles, n, d)) for d in (0, 1)}
        det_ws = torch.empty(det_bytes[1] // 4 + 4, dtype=torch.int32, device="cuda")
        projected = state["aux"].projected

        def forward_det():
            rec, aux = AG.project_ellipsoids(u, means, scales, rots)
            col = AG.sh_colors(u[16:19], means, shs, 3, ops)
            rgb, _ = AG.rasterize(rec, col, aux, w, h, deterministic=True)
            state.update(rec=rec, col=col, aux=aux, loss=(rgb * gimg).sum())

        def det_entry(depth):
            tail = (zs.data_ptr(), 1, gdimg.data_ptr(), gz.data_ptr()) if depth else (None, 0, None, None)
            return lambda: lib.splat_composite_backward_det(cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), projected.data_ptr(), idx, cnt,
                                                            off, pairs, w, h, g4.data_ptr(), n, grec.data_ptr(), gcol.data_ptr(), *tail,
                                                            det_ws.data_ptr(), det_bytes[int(depth)])
        work.update({"forward_det": forward_det, "backward_det": None, "composite_backward_det": det_entry(False)})
        if depth_too:
            work["composite_backward_det_depth"] = det_entry(True)

    if abs_too:
        gabs = torch.zeros((n, 2), device="cuda")

        def forward_abs(deterministic=False):
            def go():
                rec, aux = AG.project_ellipsoids(u, means, scales, rots)
                col = AG.sh_colors(u[16:19], means, shs, 3, ops)
                rgb, _ = AG.rasterize(rec, col, aux, w, h, deterministic=deterministic, absgrad=True)
                state.update(rec=rec, col=col, aux=aux, loss=(rgb * gimg).sum())
            return go

        def abs_entry(depth):
            tail = (zs.data_ptr(), 1, gdimg.data_ptr(), gz.data_ptr()) if depth else (None, 0, None, None)
            return lambda: lib.splat_composite_backward_abs(cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), idx, cnt, off, w, h,
                                                            g4.data_ptr(), n, grec.data_ptr(), gcol.data_ptr(), *tail, gabs.data_ptr())
        work.update({"forward_abs": forward_abs(), "backward_abs": None, "composite_backward_abs": abs_entry(False)})
        if depth_too:
            work["composite_backward_abs_depth"] = abs_entry(True)
        if det_too:
            det_abs_bytes = {d: int(lib.splat_composite_backward_det_abs_workspace_bytes(pairs, tiles, n, d)) for d in (0, 1)}
            det_abs_ws = torch.empty(det_abs_bytes[1] // 4 + 4, dtype=torch.int32, device="cuda")

            def det_abs_entry(depth):
                tail = (zs.data_ptr(), 1, gdimg.data_ptr(), gz.data_ptr()) if depth else (None, 0, None, None)
                return lambda: lib.splat_composite_backward_det_abs(cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(),
                                                                    state["aux"].projected.data_ptr(), idx, cnt, off, pairs, w, h, g4.data_ptr(), n,
                                                                    grec.data_ptr(), gcol.data_ptr(), *tail, det_abs_ws.data_ptr(),
                                                                    det_abs_bytes[int(depth)], gabs.data_ptr())
            work.update({"forward_det_abs": forward_abs(True), "backward_det_abs": None, "composite_backward_det_abs": det_abs_entry(False)})
            if depth_too:
                work["composite_backward_det_abs_depth"] = det_abs_entry(True)

    if importance_too:
        ones4 = torch.zeros((h, w, 4), device="cuda")
        ones4[..., :3] = 1.0
        hits, wmax = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, device="cuda")
        wsum = torch.zeros(n, dtype=torch.int64, device="cuda")
        work.update({
            "composite_contribution": lambda: lib.splat_composite_contribution(cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), idx, cnt, off,
                                                                               w, h, None, 0.0, n, hits.data_ptr(), wmax.data_ptr(),
                                                                               wsum.data_ptr()),
            "composite_backward_ones": lambda: lib.splat_composite_backward(cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), idx, cnt, off, w,
                                                                            h, ones4.data_ptr(), n, grec.data_ptr(), gcol.data_ptr()),
        })

    if feature_ks:
        hits_f, wmax_f = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, device="cuda")
        wsum_f = torch.zeros(n, dtype=torch.int64, device="cuda")
        work["composite_contribution"] = lambda: lib.splat_composite_contribution(cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), idx, cnt,
                                                                                  off, w, h, None, 0.0, n, hits_f.data_ptr(), wmax_f.data_ptr(),
                                                                                  wsum_f.data_ptr())
        feature_bufs = {}
        for fk in feature_ks:
            fb = dict(f=torch.rand((n, fk), device="cuda") * 4 - 2, out=torch.empty((h, w, fk), device="cuda"),
                      g=torch.rand((h, w, fk), device="cuda") * 2 - 1, gf=torch.zeros((n, fk), device="cuda"))
            feature_bufs[fk] = fb
            work[f"composite_features_{fk}"] = lambda fb=fb, fk=fk: lib.splat_composite_features(
                cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), idx, cnt, off, w, h, fb["f"].data_ptr(), fk, fk, n, fb["out"].data_ptr())
            work[f"composite_features_backward_{fk}"] = lambda fb=fb, fk=fk: lib.splat_composite_features_backward(
                cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), idx, cnt, off, w, h, fb["f"].data_ptr(), fk, fk, fb["g"].data_ptr(), n,
                grec.data_ptr(), gcol.data_ptr(), fb["gf"].data_ptr(), fk)

    if camera_too:
        ut = torch.tensor(u, device="cuda", requires_grad=True)
        gu, ge = torch.empty(24, device="cuda"), torch.empty(4, device="cuda")
        grec5 = torch.rand((n, 5), device="cuda") * 2 - 1

        def forward_camera():
            rec, depths, aux = AG.project_ellipsoids(ut, means, scales, rots, return_depth=True)
            col = AG.sh_colors(ut[16:19], means, shs, 3, ops)
            rgb, _, depth = AG.rasterize(rec, col, aux, w, h, depths=depths)
            dz = torch.where(torch.isfinite(depth), depth, torch.zeros_like(depth))
            state.update(rec=rec, col=col, aux=aux, depths=depths, loss=(rgb * gimg).sum() + (dz * gdimg).sum())

        def plus_torch_sum():
            work["project_backward"]()
            U = ut.detach().clone().requires_grad_()
            (torch_records(U, means.detach(), scales.detach(), rots.detach(), float(w), float(h)) * grec5).sum().backward()

        def plus_torch_terms():
            work["project_backward"]()
            with torch.no_grad():
                torch_camera_terms(ut.detach(), means.detach(), scales.detach(), rots.detach(), grec5, float(w), float(h))

        def camera_entry(gzp_ptr):
            return lambda: lib.splat_project_ellipsoid_backward_camera(cx.ctx, uf, m4.data_ptr(), 1, s4.data_ptr(), 1, rots.data_ptr(), 1, n,
                                                                       grec.data_ptr(), gp.data_ptr(), gs.data_ptr(), gq.data_ptr(), gzp_ptr,
                                                                       gu.data_ptr())
        work.update({
            "forward_depth": forward_depth,
            "backward_depth": None,
            "forward_camera": forward_camera,
            "backward_camera": None,
            "project_backward_depth": lambda: lib.splat_project_ellipsoid_backward_depth(cx.ctx, uf, m4.data_ptr(), 1, s4.data_ptr(), 1,
                                                                                         rots.data_ptr(), 1, n, grec.data_ptr(), gp.data_ptr(),
                                                                                         gs.data_ptr(), gq.data_ptr(), gzp.data_ptr()),
            "project_backward_camera": camera_entry(None),
            "project_backward_camera_depth": camera_entry(gzp.data_ptr()),
            "sh3_backward_camera": lambda: lib.splat_sh_colors_backward_camera(cx.ctx, eye.ctypes.data_as(C.POINTER(C.c_float)), m4.data_ptr(), 1,
                                                                               shs.data_ptr(), 48, 3, ops.data_ptr(), gcol.data_ptr(), n,
                                                                               gsh.data_ptr(), gp.data_ptr(), gop.data_ptr(), ge.data_ptr()),
            "project_backward_plus_torch_sum": plus_torch_sum,
            "project_backward_plus_torch_terms": plus_torch_terms,
        })
    forwards = {"backward": forward, "backward_depth": forward_depth}
    if surfel_too:
        def forward_surfel():
            rec, aux = AG.project_surfels(u, means, scales, rots)
            col = AG.sh_colors(u[16:19], means, shs, 3, ops)
            rgb, _ = AG.rasterize(rec, col, aux, w, h)
            state.update(srec=rec, scol=col, saux=aux, loss=(rgb * gimg).sum())

        def forward_surfel_depth():
            rec, cw, aux = AG.project_surfels(u, means, scales, rots, return_depth=True)
            col = AG.sh_colors(u[16:19], means, shs, 3, ops)
            rgb, _, depth = AG.rasterize(rec, col, aux, w, h, depths=cw)
            dz = torch.where(torch.isfinite(depth), depth, torch.zeros_like(depth))
            state.update(srec=rec, scol=col, saux=aux, scw=cw, loss=(rgb * gimg).sum() + (dz * gdimg).sum())

        # the surfel frame's own lists, copied out of the binner (the ellipsoid kinds re-bin it between the surfel kinds' calls)
        forward_surfel_depth()
        srec, scw = state["srec"].detach().contiguous(), state["scw"].detach().contiguous()
        saux = state["saux"]
        cx.bin(saux, w, h)
        sidx_p, scnt_p, soff_p = cx.lists()
        _lib.check(lib.splat_bin_total(cx.binner, C.byref(tot)), cx.ctx)
        surfel_pairs = int(tot.value)
        sidx = torch.empty(max(surfel_pairs, 1), dtype=torch.int32, device="cuda")
        scnt, soff = torch.empty(tiles, dtype=torch.int32, device="cuda"), torch.empty(tiles, dtype=torch.int32, device="cuda")
        for dst, src, nb in ((sidx, sidx_p, surfel_pairs * 4), (scnt, scnt_p, tiles * 4), (soff, soff_p, tiles * 4)):
            if nb:
                _lib.check(lib.splat_buf_copy(cx.ctx, dst.data_ptr(), src, nb), cx.ctx)
        torch.cuda.synchronize()
        scfg = _lib.CompositeCfg(_lib.MODE_FRONT_TO_BACK, 1, 16, 0, _lib.U32_MAX, _lib.RECORDS_PROJECTED, 1, _lib.FOOTPRINT_SURFEL)
        sdepth = torch.empty((h, w), device="cuda")
        slists = (sidx.data_ptr(), scnt.data_ptr(), soff.data_ptr())
        work.update({
            "forward_surfel": forward_surfel,
            "backward_surfel": None,
            "composite_backward_surfel": lambda: lib.splat_composite_backward(cx.ctx, C.byref(scfg), col.data_ptr(), 1, srec.data_ptr(), *slists, w, h,
                                                                              g4.data_ptr(), n, grec.data_ptr(), gcol.data_ptr()),
            "surfel_depth_forward": lambda: lib.splat_composite_surfel_depth(cx.ctx, C.byref(scfg), col.data_ptr(), 1, srec.data_ptr(), *slists, w, h,
                                                                             scw.data_ptr(), 1, n, sdepth.data_ptr(), None),
            "project_backward_surfel": lambda: lib.splat_project_surfel_backward(cx.ctx, uf, m4.data_ptr(), 1, s4.data_ptr(), 1, rots.data_ptr(), 1, n,
                                                                                 grec.data_ptr(), gzp.data_ptr(), gp.data_ptr(), gs.data_ptr(),
                                                                                 gq.data_ptr()),
        })
        forwards["backward_surfel"] = forward_surfel
        if depth_too:
            work.update({
                "forward_surfel_depth": forward_surfel_depth,
                "backward_surfel_depth": None,
                "composite_backward_surfel_depth": lambda: lib.splat_composite_backward_depth(cx.ctx, C.byref(scfg), col.data_ptr(), 1, srec.data_ptr(),
                                                                                              *slists, w, h, g4.data_ptr(), n, grec.data_ptr(),
                                                                                              gcol.data_ptr(), scw.data_ptr(), 1, gdimg.data_ptr(),
                                                                                              gz.data_ptr()),
            })
            forwards["backward_surfel_depth"] = forward_surfel_depth
        if dist_too:
            gdist = (torch.rand((h, w), device="cuda") * 2 - 1) * 100.0
            sdist = torch.empty((h, w), device="cuda")
            sfeat = dict(f=torch.rand((n, 3), device="cuda"), out=torch.empty((h, w, 3), device="cuda"),
                         g=torch.rand((h, w, 3), device="cuda") * 2 - 1, gf=torch.zeros((n, 3), device="cuda"))

            def forward_surfel_distortion():
                rec, cw, aux = AG.project_surfels(u, means, scales, rots, return_depth=True)
                col = AG.sh_colors(u[16:19], means, shs, 3, ops)
                rgb, _, depth, dist = AG.rasterize(rec, col, aux, w, h, depths=cw, distortion=DIST_RANGE)
                dz = torch.where(torch.isfinite(depth), depth, torch.zeros_like(depth))
                state.update(srec=rec, scol=col, saux=aux, scw=cw, loss=(rgb * gimg).sum() + (dz * gdimg).sum() + (dist * gdist).sum())
            work.update({
                "forward_surfel_distortion": forward_surfel_distortion,
                "backward_surfel_distortion": None,
                "surfel_distortion_forward": lambda: lib.splat_composite_surfel_distortion(
                    cx.ctx, C.byref(scfg), col.data_ptr(), 1, srec.data_ptr(), *slists, w, h, scw.data_ptr(), 1, n, sdepth.data_ptr(), None,
                    DIST_RANGE[0], DIST_RANGE[1], sdist.data_ptr()),
                "composite_backward_surfel_distortion": lambda: lib.splat_composite_backward_distortion(
                    cx.ctx, C.byref(scfg), col.data_ptr(), 1, srec.data_ptr(), *slists, w, h, g4.data_ptr(), n, grec.data_ptr(), gcol.data_ptr(),
                    scw.data_ptr(), 1, gdimg.data_ptr(), gz.data_ptr(), DIST_RANGE[0], DIST_RANGE[1], gdist.data_ptr()),
                "surfel_features_3": lambda: lib.splat_composite_features(
                    cx.ctx, C.byref(scfg), col.data_ptr(), 1, srec.data_ptr(), *slists, w, h, sfeat["f"].data_ptr(), 3, 3, n, sfeat["out"].data_ptr()),
                "surfel_features_backward_3": lambda: lib.splat_composite_features_backward(
                    cx.ctx, C.byref(scfg), col.data_ptr(), 1, srec.data_ptr(), *slists, w, h, sfeat["f"].data_ptr(), 3, 3, sfeat["g"].data_ptr(), n,
                    grec.data_ptr(), gcol.data_ptr(), sfeat["gf"].data_ptr(), 3),
            })
            forwards["backward_surfel_distortion"] = forward_surfel_distortion
    if aa_too:
        grho = torch.rand(n, device="cuda") * 2 - 1

        def forward_aa():
            rec, rho, aux = AG.project_ellipsoids(u, means, scales, rots, antialiased=True)
            col = AG.compensate_opacity(AG.sh_colors(u[16:19], means, shs, 3, ops), rho)
            rgb, _ = AG.rasterize(rec, col, aux, w, h)
            state.update(rec=rec, col=col, aux=aux, loss=(rgb * gimg).sum())
        work.update({
            "forward_aa": forward_aa,
            "backward_aa": None,
            "project_backward_aa": lambda: lib.splat_project_ellipsoid_backward_aa(cx.ctx, uf, m4.data_ptr(), 1, s4.data_ptr(), 1, rots.data_ptr(), 1,
                                                                                   n, grec.data_ptr(), gp.data_ptr(), gs.data_ptr(), gq.data_ptr(),
                                                                                   None, None, grho.data_ptr()),
        })
        forwards["backward_aa"] = forward_aa
    if camera_too:
        forwards["backward_camera"] = forward_camera
    if det_too:
        forwards["backward_det"] = forward_det
    if abs_too:
        forwards["backward_abs"] = work["forward_abs"]
        if det_too:
            forwards["backward_det_abs"] = work["forward_det_abs"]

    def run(kind, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if kind in ("project_backward_plus_torch_sum", "project_backward_plus_torch_terms"):
            calls = 1  # (about a hundred elementwise launches over n splats and their autograd: once per round is enough)
        if kind in forwards:
            tot = 0.0
            for _ in range(calls):
                forwards[kind]()
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
    if det_too:
        _lib.check(work["composite_backward_det"](), cx.ctx)
        torch.cuda.synchronize()
        written = int(det_ws[:4 * tiles].reshape(tiles, 4)[:, 0].to(torch.int64).sum())  # (the tile table's largest L: the slots stored)
        extra.update({"det_workspace_bytes": det_bytes[0], "det_slots_written": written,
                      "det_gather_floor_ms": round((2 * 36 * written + 16 * tiles) / COPY_RATE * 1e3, 4),
                      "composite_backward_det_over_atomic": round(med["composite_backward_det"] / med["composite_backward"], 3),
                      "backward_det_over_atomic": round(med["backward_det"] / med["backward"], 3)})
        if depth_too:
            extra.update({"det_workspace_bytes_depth": det_bytes[1],
                          "det_gather_floor_ms_depth": round((2 * 40 * written + 16 * tiles) / COPY_RATE * 1e3, 4),
                          "composite_backward_det_depth_over_atomic": round(med["composite_backward_det_depth"] / med["composite_backward_depth"], 3)})
    if abs_too:
        pairs_of = [("composite_backward_abs", "composite_backward"), ("backward_abs", "backward")]
        if depth_too:
            pairs_of.append(("composite_backward_abs_depth", "composite_backward_depth"))
        if det_too:
            pairs_of += [("composite_backward_det_abs", "composite_backward_det"), ("backward_det_abs", "backward_det")]
            extra.update({"det_abs_workspace_bytes": det_abs_bytes[0]})
            if depth_too:
                pairs_of.append(("composite_backward_det_abs_depth", "composite_backward_det_depth"))
                extra.update({"det_abs_workspace_bytes_depth": det_abs_bytes[1]})
        for a, b in pairs_of:
            if a.startswith("composite_"):
                _lib.check(work[a](), cx.ctx)  # (the timed calls' return codes were not looked at)
            extra[f"{a}_over_{b}"] = round(med[a] / med[b], 3)
    if importance_too:
        _lib.check(work["composite_contribution"](), cx.ctx)
        extra.update({"composite_contribution_over_backward_ones": round(med["composite_contribution"] / med["composite_backward_ones"], 3)})
    for fk in feature_ks:
        for kind in (f"composite_features_{fk}", f"composite_features_backward_{fk}"):
            _lib.check(work[kind](), cx.ctx)  # (the timed calls' return codes were not looked at)
        extra[f"composite_features_{fk}_over_contribution"] = round(med[f"composite_features_{fk}"] / med["composite_contribution"], 3)
        extra[f"composite_features_backward_{fk}_over_composite_backward"] = round(med[f"composite_features_backward_{fk}"] / med["composite_backward"], 3)
    if surfel_too:
        peers = [("forward_surfel", "forward"), ("backward_surfel", "backward"), ("composite_backward_surfel", "composite_backward"),
                 ("project_backward_surfel", "project_backward")]
        if depth_too:
            peers += [("forward_surfel_depth", "forward_depth"), ("backward_surfel_depth", "backward_depth"),
                      ("composite_backward_surfel_depth", "composite_backward_depth")]
        for a in ("composite_backward_surfel", "surfel_depth_forward", "project_backward_surfel"):
            _lib.check(work[a](), cx.ctx)  # (the timed calls' return codes were not looked at)
        extra.update({f"{a}_over_{b}": round(med[a] / med[b], 3) for a, b in peers})
        extra["surfel_pairs"] = surfel_pairs
        if dist_too:
            for a in ("surfel_distortion_forward", "composite_backward_surfel_distortion", "surfel_features_3", "surfel_features_backward_3"):
                _lib.check(work[a](), cx.ctx)  # (the timed calls' return codes were not looked at)
            extra.update({f"{a}_over_{b}": round(med[a] / med[b], 3) for a, b in (
                ("forward_surfel_distortion", "forward_surfel_depth"), ("backward_surfel_distortion", "backward_surfel_depth"),
                ("surfel_distortion_forward", "surfel_depth_forward"),
                ("composite_backward_surfel_distortion", "composite_backward_surfel_depth"))})
            extra["fused_backward_over_depth_ms"] = round(med["composite_backward_surfel_distortion"] - med["composite_backward_surfel_depth"], 4)
            extra["centre_recipe_forward_ms"] = round(med["surfel_depth_forward"] + med["surfel_features_3"], 4)
            extra["centre_recipe_backward_ms"] = round(med["composite_backward_surfel_depth"] + med["surfel_features_backward_3"], 4)
    if aa_too:
        extra.update({f"{a}_over_{b}": round(med[a] / med[b], 3) for a, b in (
            ("forward_aa", "forward"), ("backward_aa", "backward"), ("project_backward_aa", "project_backward"))})
    if camera_too:
        extra.update({f"{a}_over_{b}": round(med[a] / med[b], 3) for a, b in (
            ("project_backward_camera", "project_backward"), ("project_backward_camera_depth", "project_backward_depth"),
            ("sh3_backward_camera", "sh3_backward"), ("backward_camera", "backward_depth"), ("forward_camera", "forward_depth"),
            ("project_backward_plus_torch_sum", "project_backward_camera"),
            ("project_backward_plus_torch_terms", "project_backward_camera"))})
    print(json.dumps({"config": name, "n": n, "calls_per_round": k, "rounds": rounds,
                      **{f"{kind}_ms": round(v, 4) for kind, v in med.items()},
                      **{f"{kind}_ms_min_max": [round(min(v), 4), round(max(v), 4)] for kind, v in ts.items()},
                      "pairs": pairs,
                      "staged_pairs": staged_pairs, "consumed_pairs": consumed_pairs,
                      "atomic_bytes_bound": atomic_bytes, "atomic_floor_ms": round(atomic_bytes / ATOMIC_RATE * 1e3, 4), **extra}), flush=True)
