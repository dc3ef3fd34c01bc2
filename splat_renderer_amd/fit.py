"""Fitting a cloud of anisotropic 3D Gaussians to images (footprint="ellipsoid"; an extension, no reference counterpart): the
parameters, their initialisation from a point cloud, a fused Adam step whose state survives a change of the splat count, and
3DGS's adaptive density control.

    xyz, rgb = load_point_ply("sparse/0/points3D.ply")                  # what structure from motion leaves
    fit = GaussianFit.from_points(xyz, rgb)                             # 3DGS's initialisation (below)
    # or, from an existing cloud:
    fit = GaussianFit(means, scales, rotations, opacity, sh)           # activated values, as load_gaussian_ply returns them
    for step in range(steps):
        rgb, alpha = fit.render(camera_or_uniforms, width, height)
        photometric_loss(rgb, target).backward()
        fit.step()                                                      # statistics of this frame, Adam, gradients zeroed
        if step % 100 == 99:
            counts = fit.densify_and_prune(max_splats=...)              # {"pruned", "kept", "cloned", "split", "n"}
    fit.save_ply(path)

GaussianFit holds 3DGS's raw parameters as contiguous float32 CUDA leaves that require grad: means (n, 3), log_scales (n, 3),
rotations (n, 4) as (w, x, y, z), unnormalised, opacity_logits (n,), sh (n, 3 K) basis-major; beside each its two Adam
moments, and the three statistics planes of density control (grad_accum, denom, max_radius).  render() applies the
activations in torch (exp, sigmoid) and calls autograd's project_ellipsoids, sh_colors and rasterize, so everything of
splat_renderer_amd.autograd holds for its results; it keeps the records and retains their gradient, which step() hands to
splat_density_accumulate.  step() is five splat_adam_step launches (include/splat.h, "Density control and optimiser"), with
sparse=True (the default) masked by that frame's visibility: a splat the frame did not see keeps its parameters and moments,
as in the "sparse Adam" of the faster 3DGS trainers (its gradient is exactly zero; a dense Adam would still let its momentum
move it).  densify_and_prune() is splat_densify_plan, splat_densify_geometry and splat_densify_rows: it replaces the tensors
(callers must not hold on to the old ones), moves the moments with them (new splats start at zero) and resets the statistics.
Every kernel runs on torch's current stream; only densify_and_prune waits on the host (once, for the new count).

from_points() is 3DGS's start: every point becomes an isotropic splat whose scale is the root of the mean squared distance to the
point's three nearest neighbours (splat_knn_mean_sq: include/splat.h, "Initialisation from a point cloud"; exact, and not the
n x n distances), floored at sqrt(min_sq_distance); identity rotations, one opacity, the colour as the SH DC term.  It waits on
the host once, to refuse a cloud in which some point has no three usable neighbours.

The other strategy is 3DGS-MCMC (include/splat.h, "MCMC relocation"), for a fit whose splat count is a budget:

    fit = GaussianFit(..., sparse=False)
    for step in range(steps):
        rgb, alpha = fit.render(camera_or_uniforms, width, height)
        (photometric_loss(rgb, target) + fit.regularizer()).backward()
        fit.step()
        fit.inject_noise()                                              # opacity-gated noise on the means, every step
        if step % 100 == 99:
            fit.relocate()                                              # dead splats onto live ones, the image unchanged
            fit.add_new(max_splats=...)                                 # 5 % more, up to exactly max_splats

relocate() and add_new() replace densify_and_prune() and reset_opacity() and are not used beside them.  The regularisers reach
splats the frame did not see, whose gradient a masked Adam step would drop: an MCMC fit wants sparse=False.

GaussianFit(..., deterministic=True) makes a fit repeatable bit for bit: two runs from the same arrays, targets, cameras and
seeds end in the same parameters, the same moments and the same PLY bytes.  Every kernel of a step sums in a fixed order or
not at all, except the composite's backward, whose float atomics arrive in a varying order; the flag replaces it with
autograd.rasterize's deterministic=True (splat_composite_backward_det).  It costs a workspace per backward of 16 bytes per
tile + 4 per splat + 36 per (tile, splat) pair of the frame's lists (40 with a depth gradient), and the time of a second pass
over it.  The default is the atomic path: two runs then drift apart after the first step.

Antialiasing (Mip-Splatting's two filters; both off by default, and a fit that uses neither computes the bytes it always did):

    fit = GaussianFit(..., antialiased=True)                            # the 2D Mip filter: render() draws opacity x rho
    fit.update_filter_3d(train_cameras, width, height)                  # the 3D smoothing filter, from the training cameras
    ...
    fit.densify_and_prune(...); fit.update_filter_3d(train_cameras, width, height)

antialiased=True makes render() call autograd.project_ellipsoids(antialiased=True) and multiply the opacity by its rho
(include/splat.h, "antialiased frames").  update_filter_3d() gives every splat the largest sampling rate focal / depth any of the
cameras sees it at (splat_sampling_rate_max, one launch per camera) and from it the filter's sigma f = sqrt(variance) / rate;
render() then draws s_eff = sqrt(s^2 + f^2) per axis and o_eff = o sqrt(prod s^2 / prod s_eff^2), in torch ops, so the
gradients reach log_scales and opacity_logits through them.  A splat no camera saw gets f = 0, no smoothing (Mip-Splatting
gives such splats the largest filter of the seen ones; a splat outside every training view is not constrained by any of them
either way, and 0 leaves it as the optimiser has it).  The filter belongs to the rows it was computed for:
densify_and_prune(), relocate() and add_new() clear it, and the caller computes it again after them, as Mip-Splatting does
after every densification.  save_ply() writes the fused values (log s_eff, logit o_eff), so that any viewer draws the cloud
the fit drew; without a filter it writes the raw parameters bit for bit, as before.

AbsGS's criterion for where to add splats (include/splat.h, splat_composite_backward_abs; Ye et al. 2024; gsplat's absgrad):

    fit = GaussianFit(..., absgrad=True)

grad_accum is by default the norm of each splat's summed screen-space gradient dL/dc, a signed sum over its pixels: a large
splat that covers two under-fitted regions is pulled in opposite directions, the pulls cancel, the statistic stays under the
threshold and the splat is never split - the blur the 3DGS heuristic is known for.  With absgrad=True render() asks
autograd.rasterize for the absolute sums (sum |term c.x|, sum |term c.y| over the splat's pixels, which cannot cancel) and
step() hands them to splat_density_accumulate_abs: grad_accum += hypot(abs.x W / 2, abs.y H / 2), the same rule on the other
plane, with the same visibility mask.  Adam still gets the signed gradients: only the statistic changes.  The absolute
statistic is several times the signed one (a median of 6 to 12 times on the test clouds), so densify_and_prune()'s default
grad_threshold is then 8e-4, the value gsplat's documentation recommends with absgrad, instead of 2e-4; an explicit value
wins.  It costs two more wave sums per list entry in the composite's backward and, with deterministic=True, 8 more bytes per
pair of its workspace.  Off by default: a fit without it runs the calls it always ran.

Pruning a finished fit by what the training views see of it (include/splat.h, "Contribution of every splat to a frame"):

    for cam in train_cameras:
        fit.accumulate_importance(cam, width, height)                   # one forward walk per view; no gradient, no image
    fit.prune_by_importance(threshold=0.01)                             # RadSplat's rule: {"pruned", "kept", "n"}
    # or: fit.prune_by_importance(keep=0.5, kind="sum")                  # the better half by summed blend weight

accumulate_importance() forms the frame's records and colours exactly as render() does (activations, 3D filter, rho) under
no_grad and hands them to autograd.contribution, which adds into three persistent planes: per splat the hit count, the largest
blend weight T alpha any pixel of any view gave it, and the summed weight in fixed point.  It does not touch the pending
frame, so it may sit between backward() and step().  importance(kind) turns the planes into a score: "max" (RadSplat), "sum"
(Mini-Splatting's summed weights), "hits" (the count) or "lightgaussian" (below); prune_by_importance() keeps the rows the score
selects, in index order, moving all five parameter planes and both Adam moments with splat_densify_rows (every row a kept
original: moments are copied, not zeroed), then resets the statistics, the importance planes, the 3D filter and the pending
frame.  It waits on the host once, for the count.  The planes are integer sums and a maximum: the same views give the same
scores, and so the same pruned cloud, bit for bit, on every run.  densify_and_prune(), relocate() and add_new() clear the planes
too: the rows they were accumulated for are gone.

Geometry and feature terms beside the image (include/splat.h, "Feature channels of a frame"; autograd.composite_features):

    rgb, alpha, feat = fit.render(cam, width, height, features=f)       # feat (H, W, K) = sum w_i f[i, k]; after depth if asked

f is the caller's (n, K) CUDA float32 tensor, K <= 32, one row per splat of the fit as it is now: the fit neither owns nor
optimises it (a learned embedding has its own optimiser, and its rows follow densify_and_prune() only if the caller moves
them).  It is blended with the frame's own weights from the lists render() binned (no second sort), is not compensated by rho,
and its gradients reach means, log_scales, rotations and opacity_logits through the same records and opacities as the image's.
A deterministic fit refuses it (SplatError): the feature gradients are float atomic sums and no fixed-order variant exists.
absgrad's statistic keeps counting the image's terms only.  The two usual regularisers, in torch ops on the fit's parameters:

    # normal consistency (2DGS): the shortest axis of every splat, flipped towards the eye, blended into a normal map and held to
    # the normal of the frame's own depth map by one fused kernel pair (autograd.normal_consistency_loss)
    scales, _ = fit._activated()
    rgb, alpha, depth, nmap = fit.render(cam, width, height, return_depth=True, features=AG.splat_normals(fit.means, scales, fit.rotations, eye))
    loss = AG.photometric_loss(rgb, target) + lam * AG.normal_consistency_loss(nmap, depth, cam, weight=alpha.detach())

    # depth distortion: features (1, z, z^2) give W, M, Q per pixel; sum_{j<i} w_i w_j (z_i - z_j)^2 = W Q - M^2
    z = ((fit.means - eye).norm(dim=1) - near) / (far - near)          # normalised to the scene's depth range: see below
    rgb, alpha, wmq = fit.render(cam, width, height, features=torch.stack([torch.ones_like(z), z, z * z], dim=1))
    distortion = (wmq[..., 0] * wmq[..., 2] - wmq[..., 1] ** 2).mean()

Normalise z before squaring it: W Q - M^2 cancels in binary32 where the depth spread inside a pixel is small against the depth.

The surface of a finished fit (include/splat.h, "TSDF fusion and mesh extraction"; tsdf.TsdfVolume), 2DGS's recipe:

    vertices, triangles, colors = fit.extract_mesh(train_cameras, width, height, voxel=0.01)   # device tensors
    save_mesh_ply(path, vertices.cpu(), triangles.cpu(), colors.cpu())

Under no_grad every camera is rendered with depth, the depth maps are fused into a truncated signed distance volume over the box
of the means (padded by trunc = 4 voxel; bounds= names another box) with the frame's alpha as the weight of the observation
where alpha >= alpha_min, and marching tetrahedra pull the zero surface out: indexed, consistently wound, the same bytes on
every run.  The depth is the blended distance to the splats' centres, so the surface sits where the fit's mass does: a fit
trained with normal_consistency_loss and the distortion term has flat, thin splats and gives the cleaner surface.  One launch
per view on top of the render, one host wait for the mesh's size.

Fitting 2D Gaussian surfels (include/splat.h, "2D Gaussian surfels"; 2DGS, Huang et al. 2024): SurfelFit is GaussianFit with
2DGS's parameters, log_scales (n, 2) along the two tangent axes, and the whole 2DGS objective:

    fit = SurfelFit.from_points(xyz, rgb)                               # or SurfelFit(means, scales (n, 2), rotations, opacity, sh)
    for step in range(steps):
        rgb, alpha, depth, dist, nmap = fit.render(cam, width, height, return_depth=True, normals=True, distortion=(near, far))
        loss = AG.photometric_loss(rgb, target)                         # L1 + D-SSIM
        loss = loss + lam_n * AG.normal_consistency_loss(nmap, depth, cam, weight=alpha.detach(), depth_kind="z")
        loss = loss + lam_d * dist.mean()
        loss.backward()
        fit.step()
        if step % 100 == 99:
            fit.densify_and_prune(max_splats=...)
    fit.save_ply(path)                                                  # 2DGS's file: ply.load_surfel_ply reads it
    mesh = fit.extract_mesh(train_cameras, width, height, voxel=0.01)

render() is autograd.render_surfels: depth is the ray-surfel intersection depth in clip w, dist 2DGS's depth-distortion map, nmap
the blended surfel normals.  step() takes the frame's statistics with splat_density_accumulate_surfel, whose visibility and screen
radius come from the surfel record's own extent (a surfel's record has B10 and q terms the ellipsoid's rule takes for zero), then
runs the same five Adam launches.  densify_and_prune() plans on the larger of the two scales and splits inside the surfel's
plane (splat_densify_plan_surfel, splat_densify_geometry_surfel), min_opacity 2DGS's 0.05.  extract_mesh() fuses the intersection
depth (depth_kind "z"), the reason to fit surfels: a flat surfel's depth is its plane, not the distance to its centre.
from_points() starts from 2DGS's rand((n, 4)) rotations, drawn on the host from rotation_seed.  Not built for surfels (each
raises SplatError): deterministic, antialiased and absgrad fits, update_filter_3d, relocate, add_new, inject_noise and the
importance scores.
"""
import ctypes as C
import math
import numbers

from . import _lib
from . import autograd as AG
from ._lib import SplatError, check

# 3DGS's learning rates: position (its initial rate; callers schedule it through step(lr=...)), scaling, rotation, opacity,
# SH DC, SH rest (DC / 20)
DEFAULT_LR = {"means": 1.6e-4, "log_scales": 5e-3, "rotations": 1e-3, "opacity_logits": 5e-2, "sh": 2.5e-3, "sh_rest": 1.25e-4}
PLANES = ("means", "log_scales", "rotations", "opacity_logits", "sh")


def select_by_importance(score, threshold=None, keep=None):
    """The rows prune_by_importance keeps, as ascending int64 indices into `score` (a 1-D torch tensor, any device).  Exactly one
    of threshold (keep score >= threshold) and keep (the highest scores: an int is a count, clamped to [0, n]; a float in (0, 1]
    a fraction of n rounded down, at least 1) is given.  Equal scores go to the lower index: a stable descending sort."""
    torch = AG._t()
    if (threshold is None) == (keep is None):
        raise SplatError(-1, "prune_by_importance: give exactly one of threshold and keep")
    n = int(score.shape[0])
    if threshold is not None:
        return torch.nonzero(score.double() >= float(threshold)).reshape(-1)  # (in float64: a threshold below binary32's range still cuts at > 0)
    if isinstance(keep, bool) or not isinstance(keep, (numbers.Integral, numbers.Real)):
        raise SplatError(-1, f"prune_by_importance: keep must be an int count or a float fraction, not {keep!r}")
    if not isinstance(keep, numbers.Integral):
        keep = float(keep)
        if not 0.0 < keep <= 1.0:
            raise SplatError(-1, f"prune_by_importance: a fractional keep must lie in (0, 1], not {keep}")
        k = min(n, max(1, int(math.floor(keep * n))))
    else:
        if keep < 0:
            raise SplatError(-1, f"prune_by_importance: keep must be >= 0, not {keep}")
        k = min(n, int(keep))
    order = torch.sort(score, descending=True, stable=True).indices[:k]
    return torch.sort(order).values


class GaussianFit:
    # what a fit of another footprint (SurfelFit) replaces: the scales per splat, the three entry points that read them or the
    # record, and the kind of depth its render() returns
    SCALES = 3
    _ACCUMULATE, _PLAN, _GEOMETRY = "splat_density_accumulate", "splat_densify_plan", "splat_densify_geometry"
    _DEPTH_KIND = "distance"

    def __init__(self, means, scales, rotations, opacity, sh, degree=None, lr=None, betas=(0.9, 0.999), eps=1e-15, sparse=True,
                 device="cuda", exact_activations=False, deterministic=False, antialiased=False, absgrad=False):
        """means (n, 3), scales (n, 3) > 0, rotations (n, 4), opacity (n,) in (0, 1), sh (n, K, 3) or (n, 3 K), K = (degree +
        1)^2: arrays or tensors of activated values.  lr: a dict that overrides entries of DEFAULT_LR.  exact_activations:
        render() forms exp and sigmoid in float64 and rounds once, as load_gaussian_ply does, so the frame the fit renders is the
        frame its saved PLY renders; with the default float32 activations the two differ by an ulp in some scales and opacities,
        which now and then carries one pixel across a splat's 3-sigma cut (a step of up to 0.011 x opacity in that pixel).
        deterministic: render() asks autograd.rasterize for its fixed-order backward, so that the whole fit is bit-reproducible
        (the module's docstring).  antialiased: render() draws every opacity times the 2D Mip filter's rho (the module's
        docstring).  absgrad: the density statistic is AbsGS's absolute screen-space gradient (the module's docstring)."""
        torch = AG._t()
        t = lambda a: torch.as_tensor(a, dtype=torch.float32).to(device).detach()  # noqa: E731
        means, scales, rotations, opacity, sh = t(means), t(scales), t(rotations), t(opacity).reshape(-1), t(sh)
        n = means.shape[0]
        sh = sh.reshape(n, -1)
        k = sh.shape[1] // 3
        self.degree = {1: 0, 4: 1, 9: 2, 16: 3}.get(k) if degree is None else int(degree)
        if self.degree is None or sh.shape[1] != 3 * (self.degree + 1) ** 2:
            raise SplatError(-1, f"sh must hold 3 (degree + 1)^2 floats per splat, degree 0-3, not {sh.shape[1]}")
        if means.shape != (n, 3) or scales.shape != (n, self.SCALES) or rotations.shape != (n, 4) or opacity.shape != (n,):
            raise SplatError(-1, f"means (n, 3), scales (n, {self.SCALES}), rotations (n, 4) and opacity (n,) are expected")
        self.lr = dict(DEFAULT_LR, **(lr or {}))
        self.betas, self.eps, self.sparse = (float(betas[0]), float(betas[1])), float(eps), bool(sparse)
        self.exact_activations = bool(exact_activations)
        self.deterministic = bool(deterministic)
        self.antialiased = bool(antialiased)
        self.absgrad = bool(absgrad)
        self._aux = None  # (absgrad) the pending frame's ProjectedSplats: backward() leaves the absolute sums on it
        self.filter_3d = None  # (n,) sigma of the 3D smoothing filter per splat (update_filter_3d), or None
        self.steps = 0
        self.densifications = 0
        self.relocations = self.additions = self.noises = 0
        self._set(means[:, :3].clone(), torch.log(scales), rotations.clone(), torch.logit(opacity), sh.clone())
        self.m = {k: torch.zeros_like(getattr(self, k)) for k in PLANES}
        self.v = {k: torch.zeros_like(getattr(self, k)) for k in PLANES}
        self._reset_statistics()
        self.reset_importance()
        # 3DGS's percent_dense x scene extent: the default scale_threshold of densify_and_prune
        centre = means.mean(dim=0, keepdim=True) if n else means
        self.extent = float(1.1 * (means - centre).norm(dim=1).max()) if n else 1.0
        self._frame = None

    @classmethod
    def from_points(cls, points, colors, degree=3, opacity=0.1, min_sq_distance=1e-7, **kw):
        """3DGS's initialisation from a coloured point cloud: points (n, 3), colors (n, 3) in [0, 1] (arrays or tensors, as
        load_point_ply returns them).  scales = sqrt(max(mean_sq, min_sq_distance)) on all three axes, mean_sq the mean squared
        distance to the three nearest neighbours (autograd.knn_mean_sq_distance); rotations (1, 0, 0, 0); the given opacity;
        sh[:, 0] = (rgb - 0.5) / 0.28209479177387814 and the higher coefficients zero.  **kw goes to GaussianFit.  SplatError
        when a row of mean_sq is not finite: fewer than four usable points, or a point with a NaN or infinite coordinate."""
        return cls._from_points(points, colors, degree, opacity, min_sq_distance, cls._identity_rotations, kw)

    @staticmethod
    def _identity_rotations(n, device):
        torch = AG._t()
        rotations = torch.zeros((n, 4), device=device, dtype=torch.float32)
        rotations[:, 0] = 1.0
        return rotations

    @classmethod
    def _from_points(cls, points, colors, degree, opacity, min_sq_distance, make_rotations, kw):
        """from_points for a fit of cls.SCALES scales per splat; make_rotations(n, device) gives the (n, 4) start."""
        torch = AG._t()
        device = kw.get("device", "cuda")
        t = lambda a: torch.as_tensor(a, dtype=torch.float32).to(device).detach()  # noqa: E731
        points, colors = t(points), t(colors)
        n = points.shape[0]
        if points.dim() != 2 or points.shape[1] != 3 or tuple(colors.shape) != (n, 3):
            raise SplatError(-1, "from_points: points (n, 3) and colors (n, 3) are expected")
        if not 0 <= int(degree) <= 3:
            raise SplatError(-1, f"from_points: degree must be 0-3, not {degree}")
        mean_sq = AG.knn_mean_sq_distance(points.contiguous())
        bad = int((~torch.isfinite(mean_sq)).sum())  # (the one host sync)
        if bad or n == 0:
            raise SplatError(-1, f"from_points: {bad} of {n} points have no three usable neighbours (fewer than four points, or "
                                 "NaN or infinite coordinates): no scale can be given to them")
        scales = torch.sqrt(torch.clamp(mean_sq, min=float(min_sq_distance)))[:, None].repeat(1, cls.SCALES)
        rotations = make_rotations(n, points.device)
        sh = torch.zeros((n, (int(degree) + 1) ** 2, 3), device=points.device, dtype=torch.float32)
        sh[:, 0] = ((colors.double() - 0.5) / 0.28209479177387814).float()  # (in float64, rounded once)
        return cls(points, scales, rotations, torch.full((n,), float(opacity), device=points.device, dtype=torch.float32), sh,
                   degree=int(degree), **kw)

    def _set(self, *tensors):
        for name, value in zip(PLANES, tensors):
            setattr(self, name, value.contiguous().requires_grad_())

    def _reset_statistics(self):
        torch = AG._t()
        dev = self.means.device
        self.grad_accum, self.denom, self.max_radius = (torch.zeros(self.n, device=dev, dtype=torch.float32) for _ in range(3))
        self.visible = torch.zeros(self.n, device=dev, dtype=torch.uint8)

    @property
    def n(self):
        return self.means.shape[0]

    def parameters(self):
        return [getattr(self, k) for k in PLANES]

    def render(self, camera_or_uniforms, width, height, return_depth=False, features=None):
        """(rgb (H, W, 3), alpha (H, W)), or with return_depth (rgb, alpha, depth): autograd.render_gaussians of the activated
        parameters (with the 3D filter fused into scales and opacity when one is set, and the opacity times rho when the fit is
        antialiased).  The frame's records are kept for the next step().  features ((n, K) or (n,), the caller's tensor: the fit
        neither owns nor optimises it): autograd.rasterize's features, the map (H, W, K) appended to the tuple; not in a
        deterministic fit (SplatError)."""
        torch = AG._t()
        AG._refuse_deterministic_features(self.deterministic, features, "GaussianFit(deterministic=True).render")
        u = AG._uniforms(camera_or_uniforms, width, height)
        scales, opacity = self._activated()
        rho = None
        if self.antialiased and return_depth:
            rec, rho, depths, aux = AG.project_ellipsoids(u, self.means, scales, self.rotations, return_depth=True, antialiased=True)
        elif self.antialiased:
            rec, rho, aux = AG.project_ellipsoids(u, self.means, scales, self.rotations, antialiased=True)
            depths = None
        elif return_depth:
            rec, depths, aux = AG.project_ellipsoids(u, self.means, scales, self.rotations, return_depth=True)
        else:
            rec, aux = AG.project_ellipsoids(u, self.means, scales, self.rotations)
            depths = None
        col = AG.sh_colors(u[16:19], self.means, self.sh, self.degree, opacity)
        if rho is not None:
            col = AG.compensate_opacity(col, rho)
        if rec.requires_grad:
            rec.retain_grad()
        self._frame = (rec, int(width), int(height))
        if self.absgrad:
            self._aux = aux
            return AG.rasterize(rec, col, aux, width, height, depths=depths, deterministic=self.deterministic, absgrad=True, features=features)
        return AG.rasterize(rec, col, aux, width, height, depths=depths, deterministic=self.deterministic, features=features)

    def _activated(self):
        """(scales (n, 3), opacity (n,)) as render() draws them: exp and sigmoid (in float64, rounded once, with
        exact_activations), and with a 3D filter f the fused s_eff = sqrt(s^2 + f^2), o_eff = o sqrt(prod s^2 / prod s_eff^2)
        (formed in the activations' precision)."""
        torch = AG._t()
        if self.exact_activations:
            scales, opacity = torch.exp(self.log_scales.double()), torch.sigmoid(self.opacity_logits.double())
        else:
            scales, opacity = torch.exp(self.log_scales), torch.sigmoid(self.opacity_logits)
        if self.filter_3d is not None:
            s2 = scales * scales
            e2 = s2 + (self.filter_3d.to(scales.dtype) ** 2)[:, None]
            scales, opacity = torch.sqrt(e2), opacity * torch.sqrt(s2.prod(dim=1) / e2.prod(dim=1))
        return (scales.float(), opacity.float()) if self.exact_activations else (scales, opacity)

    def update_filter_3d(self, cameras, width, height, focal_px=None, near=0.2, margin=0.15, variance=0.2):
        """Mip-Splatting's 3D smoothing filter from the training cameras (Cameras or uniform blocks): the rate is reset to zero,
        splat_sampling_rate_max runs once per camera (a splat counts for a camera when its clip w exceeds `near` and its screen
        centre lies inside the screen widened by `margin` of its size on every side), and filter_3d = sqrt(variance) / rate, 0
        (no smoothing) where no camera saw the splat.  focal_px: the focal length in pixels, one value or one per camera; the
        default is 0.5 W |(m0, m4, m8)| of each camera's VP, formed in float64 on the host: exact for a centred pinhole (row 0
        of VP is then (2 fx / W) times a unit row of the rotation), an approximation when the principal point is off centre.
        Returns filter_3d (n,).  densify_and_prune(), relocate() and add_new() clear it: call this again after them."""
        torch = AG._t()
        n = self.n
        cameras = list(cameras)
        focals = list(focal_px) if hasattr(focal_px, "__len__") else [focal_px] * len(cameras)
        if len(focals) != len(cameras):
            raise SplatError(-1, "update_filter_3d: focal_px must be one value or one per camera")
        rate = torch.zeros(n, device=self.means.device, dtype=torch.float32)
        if n:
            cx = AG._context(self.means)
            pos = AG._cuda_f32(AG._vec4(self.means.detach(), "means", 1.0), "means", 4)
            for cam, focal in zip(cameras, focals):
                u = AG._uniforms(cam, width, height)
                if focal is None:
                    focal = 0.5 * float(u[20]) * math.sqrt(float(u[0]) ** 2 + float(u[4]) ** 2 + float(u[8]) ** 2)
                check(cx.lib.splat_sampling_rate_max(cx.ctx, AG._fptr(u), float(focal), float(near), float(margin), pos.data_ptr(), 1, n,
                                                     rate.data_ptr()), cx.ctx)
        self.filter_3d = torch.where(rate > 0, math.sqrt(float(variance)) / rate, torch.zeros_like(rate))
        self._frame = None
        return self.filter_3d

    def step(self, lr=None):
        """One optimiser step after backward(): this frame's density statistics and visibility mask, five Adam launches, the
        gradients zeroed.  lr: a dict that overrides per-plane rates for this step (e.g. {"means": scheduled_rate})."""
        if self._frame is None or self._frame[0].grad is None:
            raise SplatError(-5, f"{type(self).__name__}.step: call render() and backward() first")
        rec, width, height = self._frame
        n = self.n
        cx = AG._context(self.means)
        lib = cx.lib
        if self.absgrad:  # the same statistic of the absolute sums this frame's backward left on its projection
            gabs = self._aux.absgrad if self._aux is not None else None
            if gabs is None:
                raise SplatError(-5, "GaussianFit.step: the frame's backward left no absolute gradient")
            check(lib.splat_density_accumulate_abs(cx.ctx, rec.data_ptr(), gabs.data_ptr(), n, width, height, self.grad_accum.data_ptr(),
                                                   self.denom.data_ptr(), self.max_radius.data_ptr(), self.visible.data_ptr()), cx.ctx)
            self._aux = None
        else:
            grec = AG._cuda_f32(rec.grad, "grad_records", 8)
            check(getattr(lib, self._ACCUMULATE)(cx.ctx, rec.data_ptr(), grec.data_ptr(), n, width, height, self.grad_accum.data_ptr(),
                                                 self.denom.data_ptr(), self.max_radius.data_ptr(), self.visible.data_ptr()), cx.ctx)
        self.steps += 1
        rates = dict(self.lr, **(lr or {}))
        b1, b2 = self.betas
        bc1, isbc2 = 1.0 - b1 ** self.steps, 1.0 / math.sqrt(1.0 - b2 ** self.steps)
        mask = self.visible.data_ptr() if self.sparse and n else None
        for name in PLANES:
            p = getattr(self, name)
            if p.grad is None:  # (a plane the loss does not reach)
                continue
            g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
            fpr = p.shape[1] if p.dim() == 2 else 1
            head, tail = rates[name] / bc1, rates["sh_rest" if name == "sh" else name] / bc1
            check(lib.splat_adam_step(cx.ctx, p.data_ptr(), g.data_ptr(), self.m[name].data_ptr(), self.v[name].data_ptr(), n, fpr,
                                      3 if name == "sh" else fpr, head, tail, b1, b2, isbc2, self.eps, mask), cx.ctx)
            p.grad = None
        self._frame = None

    def densify_and_prune(self, grad_threshold=None, scale_threshold=None, min_opacity=0.005, max_screen_radius=0.0, max_world_scale=0.0,
                          max_splats=0, seed=None):
        """Clone the under-reconstructed splats, split the over-large ones, prune the transparent ones (the rules: include/splat.h,
        splat_densify_plan), from the statistics accumulated since the last call.  grad_threshold defaults to 3DGS's 2e-4, and
        to 8e-4 in a fit with absgrad=True (the absolute statistic is larger: the module's docstring); scale_threshold to 0.01 x
        the extent of the initial cloud; seed to the number of earlier calls.  Returns {"pruned", "kept", "cloned", "split", "n"}."""
        torch = AG._t()
        n = self.n
        cx = AG._context(self.means)
        lib = cx.lib
        dev = self.means.device
        if grad_threshold is None:
            grad_threshold = 8e-4 if self.absgrad else 2e-4
        cfg = _lib.DensifyCfg(float(grad_threshold), float(0.01 * self.extent if scale_threshold is None else scale_threshold),
                              float(min_opacity), float(max_screen_radius), float(max_world_scale), int(max_splats),
                              int(self.densifications if seed is None else seed) & 0xFFFFFFFFFFFFFFFF)
        self.densifications += 1
        nbytes = int(lib.splat_densify_plan_workspace_bytes(n))
        ws = torch.empty(nbytes // 4, device=dev, dtype=torch.int32)
        rows = torch.empty(max(2 * n, 1), device=dev, dtype=torch.int32)
        n_out, counts = C.c_uint32(), (C.c_uint32 * 4)()
        with torch.no_grad():
            check(getattr(lib, self._PLAN)(cx.ctx, self.log_scales.data_ptr(), self.opacity_logits.data_ptr(), self.grad_accum.data_ptr(),
                                           self.denom.data_ptr(), self.max_radius.data_ptr(), n, C.byref(cfg), ws.data_ptr(), nbytes,
                                           rows.data_ptr(), C.byref(n_out), counts), cx.ctx)
            k = int(n_out.value)
            new = {name: torch.empty((k,) + tuple(getattr(self, name).shape[1:]), device=dev, dtype=torch.float32) for name in PLANES}
            check(getattr(lib, self._GEOMETRY)(cx.ctx, rows.data_ptr(), k, self.means.data_ptr(), self.log_scales.data_ptr(),
                                               self.rotations.data_ptr(), C.byref(cfg), new["means"].data_ptr(),
                                               new["log_scales"].data_ptr()), cx.ctx)

            def move(src, mode):
                out = torch.empty((k,) + tuple(src.shape[1:]), device=dev, dtype=torch.float32)
                check(lib.splat_densify_rows(cx.ctx, rows.data_ptr(), k, src.data_ptr(), out.data_ptr(), src.shape[1] if src.dim() == 2 else 1,
                                             mode), cx.ctx)
                return out
            for name in PLANES[2:]:
                new[name] = move(getattr(self, name), _lib.DENSIFY_COPY)
            self.m = {name: move(self.m[name], _lib.DENSIFY_ZERO_NEW) for name in PLANES}
            self.v = {name: move(self.v[name], _lib.DENSIFY_ZERO_NEW) for name in PLANES}
        self._set(*(new[name] for name in PLANES))
        self._reset_statistics()
        self.reset_importance()
        self._frame = None
        self.filter_3d = None  # (it belonged to the old rows: update_filter_3d() again)
        return {"pruned": int(counts[0]), "kept": int(counts[1]), "cloned": int(counts[2]), "split": int(counts[3]), "n": k}

    def reset_opacity(self, value=0.01):
        """3DGS's opacity reset: no opacity above `value`, and the logits' moments zeroed."""
        torch = AG._t()
        with torch.no_grad():
            self.opacity_logits.clamp_(max=math.log(value / (1.0 - value)))
            self.m["opacity_logits"].zero_()
            self.v["opacity_logits"].zero_()

    # ---- 3DGS-MCMC (include/splat.h, "MCMC relocation") ---------------------------------------------------------------------

    def _mcmc_planes(self, params=None, m=None, v=None):
        params = params or {name: getattr(self, name) for name in PLANES}
        m, v = m or self.m, v or self.v
        pl = _lib.McmcPlanes()
        for k, name in enumerate(PLANES):
            pl.param[k], pl.m[k], pl.v[k] = params[name].data_ptr(), m[name].data_ptr(), v[name].data_ptr()
        pl.sh_floats = self.sh.shape[1]
        return pl

    def _mcmc_sample(self, mode, n_draws, min_opacity, seed):
        """splat_mcmc_sample on the current logits: (targets, sources, counts, (dead, alive, draws made))."""
        torch = AG._t()
        n = self.n
        cx = AG._context(self.means)
        dev = self.means.device
        nbytes = int(cx.lib.splat_mcmc_sample_workspace_bytes(n))
        ws = torch.empty(nbytes // 4, device=dev, dtype=torch.int32)
        room = max(n if mode == _lib.MCMC_RELOCATE else n_draws, 1)
        targets, sources = (torch.empty(room, device=dev, dtype=torch.int32) for _ in range(2))
        counts = torch.empty(max(n, 1), device=dev, dtype=torch.int32)
        words = (C.c_uint32 * 3)()
        check(cx.lib.splat_mcmc_sample(cx.ctx, self.opacity_logits.data_ptr(), n, mode, int(n_draws), float(min_opacity),
                                       int(seed) & 0xFFFFFFFFFFFFFFFF, ws.data_ptr(), nbytes, targets.data_ptr(), sources.data_ptr(),
                                       counts.data_ptr(), words), cx.ctx)
        return targets, sources, counts, tuple(int(x) for x in words)

    def relocate(self, min_opacity=0.005, seed=None):
        """3DGS-MCMC's relocation, in place: every dead splat (opacity below min_opacity, or a NaN logit) becomes a copy of a live
        one drawn in proportion to opacity, and the opacity and scales of the source and its copies are corrected so that the
        rendered image does not change (splat_mcmc_sample, splat_mcmc_apply); the Adam moments of moved rows and of drawn sources
        are zeroed.  seed defaults to the number of earlier calls.  Returns {"dead", "alive", "relocated", "sources"}: "sources"
        is the number of distinct splats drawn.  With densify_and_prune()/reset_opacity() this is not used: it replaces them."""
        torch = AG._t()
        n = self.n
        seed, self.relocations = (self.relocations if seed is None else seed), self.relocations + 1
        with torch.no_grad():
            targets, sources, counts, (dead, alive, draws) = self._mcmc_sample(_lib.MCMC_RELOCATE, 0, min_opacity, seed)
            drawn = 0
            if draws:
                cx = AG._context(self.means)
                pl = self._mcmc_planes()
                check(cx.lib.splat_mcmc_apply(cx.ctx, targets.data_ptr(), sources.data_ptr(), counts.data_ptr(), n, draws, n, float(min_opacity),
                                              C.byref(pl)), cx.ctx)
                drawn = int((counts[:n] > 0).sum())
        self.reset_importance()
        self._frame = None
        self.filter_3d = None  # (moved rows: update_filter_3d() again)
        return {"dead": dead, "alive": alive, "relocated": draws, "sources": drawn}

    def add_new(self, max_splats, growth=0.05, min_opacity=0.005, seed=None):
        """3DGS-MCMC's growth: k = max(0, min(max_splats, floor((1 + growth) n)) - n) new splats, each a copy of a live one drawn
        in proportion to opacity, corrected as relocate() corrects (so the count reaches max_splats exactly and never passes it).
        Like densify_and_prune() it replaces the tensors and moves the moments (new rows and drawn sources start at zero); the
        three statistics planes are resized with zeros for the new rows.  seed defaults to the number of earlier calls.  Returns
        {"added", "n"}.  With densify_and_prune()/reset_opacity() this is not used: it replaces them."""
        torch = AG._t()
        n = self.n
        k = max(0, min(int(max_splats), int(math.floor((1.0 + float(growth)) * n))) - n)
        seed, self.additions = (self.additions if seed is None else seed), self.additions + 1
        if k == 0 or n == 0:
            return {"added": 0, "n": n}
        with torch.no_grad():
            targets, sources, counts, (_, _, draws) = self._mcmc_sample(_lib.MCMC_ADD, k, min_opacity, seed)
            if draws == 0:  # (nobody alive)
                return {"added": 0, "n": n}

            def grown(src, fill_old=True):
                out = torch.zeros((n + k,) + tuple(src.shape[1:]), device=src.device, dtype=src.dtype)
                if fill_old:
                    out[:n].copy_(src.detach())
                return out
            new = {name: grown(getattr(self, name)) for name in PLANES}
            m = {name: grown(self.m[name]) for name in PLANES}
            v = {name: grown(self.v[name]) for name in PLANES}
            cx = AG._context(self.means)
            pl = self._mcmc_planes(new, m, v)
            check(cx.lib.splat_mcmc_apply(cx.ctx, targets.data_ptr(), sources.data_ptr(), counts.data_ptr(), n, k, n + k, float(min_opacity),
                                          C.byref(pl)), cx.ctx)
            self.m, self.v = m, v
            self.grad_accum, self.denom, self.max_radius, self.visible = (grown(x) for x in (self.grad_accum, self.denom, self.max_radius,
                                                                                             self.visible))
        self._set(*(new[name] for name in PLANES))
        self.reset_importance()
        self._frame = None
        self.filter_3d = None  # (new rows: update_filter_3d() again)
        return {"added": k, "n": n + k}

    # ---- importance: what the training views see of every splat (include/splat.h, "Contribution of every splat to a frame") ----

    def reset_importance(self):
        """Forget the views accumulated so far (the planes are allocated by the next accumulate_importance)."""
        self._importance = None
        self.importance_views = 0

    def accumulate_importance(self, camera_or_uniforms, width, height, pixel_weight=None, min_weight=0.0):
        """Score one view: autograd.contribution of the frame render() would draw from this camera, added into the fit's three
        importance planes (hit count, largest blend weight, summed weight in units of 2^-24).  pixel_weight (H, W) in [0, 1]
        masks pixels; a pair counts as a hit when its weight is at least min_weight.  No gradient, no image, and the pending
        frame of render() is left alone.  Returns the number of views accumulated."""
        torch = AG._t()
        with torch.no_grad():
            u = AG._uniforms(camera_or_uniforms, width, height)
            scales, opacity = self._activated()
            if self.antialiased:
                rec, rho, aux = AG.project_ellipsoids(u, self.means, scales, self.rotations, antialiased=True)
            else:
                rec, aux = AG.project_ellipsoids(u, self.means, scales, self.rotations)
                rho = None
            col = AG.sh_colors(u[16:19], self.means, self.sh, self.degree, opacity)
            if rho is not None:
                col = AG.compensate_opacity(col, rho)
            self._importance = AG.contribution(rec, col, aux, width, height, pixel_weight=pixel_weight, min_weight=min_weight,
                                               out=self._importance)
        self.importance_views += 1
        return self.importance_views

    def importance(self, kind="max"):
        """(n,) float32 score from the views accumulated so far; a splat no view scored gets 0.
          "max"            the largest blend weight T alpha over all pixels of all views (RadSplat)
          "sum"            the summed blend weight: weight_sum 2^-24, formed in float64 and rounded once (Mini-Splatting)
          "hits"           the number of (pixel, view) pairs with a weight of at least min_weight
          "lightgaussian"  hits x opacity x clamp(V / V90, 0, 1)^0.1, V the product of the activated scales and V90 its 90th
                           percentile over the cloud (LightGaussian's global significance, with its volume power 0.1)
        SplatError when no view was accumulated."""
        torch = AG._t()
        if self._importance is None or self.importance_views == 0:
            raise SplatError(-5, "GaussianFit.importance: call accumulate_importance() first")
        hits, wmax, wsum = self._importance
        with torch.no_grad():
            if kind == "max":
                return wmax.clone()
            if kind == "sum":
                return (wsum.double() * 2.0 ** -24).float()
            count = (hits.long() & 0xFFFFFFFF).double()  # (the uint32 bits)
            if kind == "hits":
                return count.float()
            if kind == "lightgaussian":
                scales, opacity = self._activated()
                vol = scales.double().prod(dim=1)
                v90 = torch.quantile(vol, 0.9) if self.n else vol.sum()
                vnorm = torch.clamp(vol / v90, 0.0, 1.0) ** 0.1
                return (count * opacity.double() * vnorm).float()
        raise SplatError(-1, f"importance: kind must be max, sum, hits or lightgaussian, not {kind!r}")

    def prune_by_importance(self, threshold=None, keep=None, kind="max"):
        """Keep the splats importance(kind) selects (select_by_importance: score >= threshold, or the `keep` highest scores - an int
        is a count, a float in (0, 1] a fraction of n rounded down, at least 1 - with ties going to the lower index), in index
        order.  All five parameter planes and both Adam moments are compacted with splat_densify_rows (copies: every row is a
        kept original); the density statistics, the importance planes, the 3D filter and the pending frame are reset.  One host
        sync, for the count.  Returns {"pruned", "kept", "n"}.  SplatError when no view was accumulated."""
        torch = AG._t()
        score = self.importance(kind)
        n = self.n
        with torch.no_grad():
            rows = select_by_importance(score, threshold=threshold, keep=keep).to(torch.int32).contiguous()  # (kind 0: the kept index)
            k = int(rows.shape[0])  # (the host sync)
            cx = AG._context(self.means)
            dev = self.means.device

            def move(src):
                out = torch.empty((k,) + tuple(src.shape[1:]), device=dev, dtype=torch.float32)
                if k:
                    check(cx.lib.splat_densify_rows(cx.ctx, rows.data_ptr(), k, src.data_ptr(), out.data_ptr(),
                                                    src.shape[1] if src.dim() == 2 else 1, _lib.DENSIFY_COPY), cx.ctx)
                return out
            new = {name: move(getattr(self, name)) for name in PLANES}
            self.m = {name: move(self.m[name]) for name in PLANES}
            self.v = {name: move(self.v[name]) for name in PLANES}
        self._set(*(new[name] for name in PLANES))
        self._reset_statistics()
        self.reset_importance()
        self._frame = None
        self.filter_3d = None  # (it belonged to the old rows: update_filter_3d() again)
        return {"pruned": n - k, "kept": k, "n": k}

    def inject_noise(self, noise_lr=5e5, lr_means=None, seed=None):
        """3DGS-MCMC's exploration term, after every step(): means += Sigma xi g noise_lr lr_means, xi standard normal, g a gate
        that is ~1 for nearly transparent splats and below 1e-20 from opacity 0.5 on (splat_mcmc_noise).  lr_means defaults to
        this fit's rate for the means; the random stream is counted by fit.steps, seed defaults to the number of earlier calls."""
        n = self.n
        seed, self.noises = (self.noises if seed is None else seed), self.noises + 1
        if n == 0:
            return
        cx = AG._context(self.means)
        scale = float(noise_lr) * float(self.lr["means"] if lr_means is None else lr_means)
        check(cx.lib.splat_mcmc_noise(cx.ctx, self.means.data_ptr(), self.log_scales.data_ptr(), self.rotations.data_ptr(),
                                      self.opacity_logits.data_ptr(), n, scale, int(self.steps) & 0xFFFFFFFF, int(seed) & 0xFFFFFFFFFFFFFFFF), cx.ctx)

    def regularizer(self, opacity_reg=0.01, scale_reg=0.01):
        """3DGS-MCMC's two regularisers as a 0-d tensor to add to the loss: opacity_reg mean(opacity) + scale_reg mean(scale), in
        plain torch.  They reach splats the frame did not see, so a fit that uses them wants sparse=False."""
        torch = AG._t()
        return opacity_reg * torch.sigmoid(self.opacity_logits).mean() + scale_reg * torch.exp(self.log_scales).mean()

    def extract_mesh(self, cameras, width, height, voxel, trunc=None, bounds=None, alpha_min=0.5, color=True, return_volume=False):
        """The surface of the fit as a triangle mesh, the way 2DGS gets one (the module's docstring): every camera (Cameras or
        uniform blocks) is rendered with depth under no_grad, the depth maps are fused into a TsdfVolume of spacing `voxel` with
        the frame's alpha as the observation weight where alpha >= alpha_min (and nothing elsewhere), and the mesh is extracted.
        trunc=None: 4 voxel.  bounds=None: the box of the means padded by trunc; else ((x0, y0, z0), (x1, y1, z1)).  Returns
        (vertices (V, 3) float32, triangles (T, 3) int32[, colors (V, 3)]) on the device (tsdf.TsdfVolume.extract_mesh);
        return_volume=True appends the volume.  The pending frame of render() / step() is not touched."""
        torch = AG._t()
        from .tsdf import TsdfVolume
        voxel = float(voxel)
        trunc = 4.0 * voxel if trunc is None else float(trunc)
        if not (voxel > 0 and trunc > 0):
            raise SplatError(-1, "extract_mesh: voxel and trunc must be > 0")
        frame, aux = self._frame, self._aux
        with torch.no_grad():
            if bounds is None:
                if self.n == 0:
                    raise SplatError(-1, "extract_mesh: the fit has no splats to take bounds from")
                lo, hi = (self.means.min(dim=0).values - trunc).tolist(), (self.means.max(dim=0).values + trunc).tolist()
            else:
                lo, hi = [float(x) for x in bounds[0]], [float(x) for x in bounds[1]]
            dims = [int(math.ceil((b - a) / voxel)) + 1 for a, b in zip(lo, hi)]
            vol = TsdfVolume(lo, voxel, dims, trunc, color=color, device=self.means.device)
            for cam in cameras:
                rgb, alpha, depth = self.render(cam, width, height, return_depth=True)[:3]
                weight = torch.where(alpha >= alpha_min, alpha, torch.zeros_like(alpha))
                vol.integrate(depth, cam, image=rgb if color else None, weight=weight, depth_kind=self._DEPTH_KIND)
            mesh = vol.extract_mesh()
        self._frame, self._aux = frame, aux
        return (*mesh, vol) if return_volume else mesh

    def save_ply(self, path):
        """The cloud as a 3D Gaussian splatting PLY file (ply.save_gaussian_ply): the raw parameters, bit for bit; with a 3D
        filter set, the fused scales and opacities (log s_eff and logit o_eff, formed in float64 and rounded once), so that a
        viewer that knows nothing of the filter draws the cloud render() draws."""
        from .ply import save_gaussian_ply
        c = lambda t: t.detach().cpu().numpy()  # noqa: E731
        if self.filter_3d is not None:
            torch = AG._t()
            with torch.no_grad():
                s2 = torch.exp(self.log_scales.double()) ** 2
                e2 = s2 + (self.filter_3d.double() ** 2)[:, None]
                o = torch.sigmoid(self.opacity_logits.double()) * torch.sqrt(s2.prod(dim=1) / e2.prod(dim=1))
                log_scales, logits = (0.5 * torch.log(e2)).float(), torch.logit(o).float()
            save_gaussian_ply(path, c(self.means), None, c(self.rotations), None, c(self.sh).reshape(self.n, -1, 3), log_scales=c(log_scales),
                              opacity_logits=c(logits))
            return
        save_gaussian_ply(path, c(self.means), None, c(self.rotations), None, c(self.sh).reshape(self.n, -1, 3), log_scales=c(self.log_scales),
                          opacity_logits=c(self.opacity_logits))


class SurfelFit(GaussianFit):
    """GaussianFit for 2D Gaussian surfels (the module's docstring, "Fitting 2D Gaussian surfels"): log_scales is (n, 2), render()
    is autograd.render_surfels, the density statistics, the plan and the split are the surfel entry points, the mesh is fused
    from the intersection depth.  step(), the row moves, the moments and the opacity reset are GaussianFit's own code."""
    SCALES = 2
    _ACCUMULATE, _PLAN, _GEOMETRY = "splat_density_accumulate_surfel", "splat_densify_plan_surfel", "splat_densify_geometry_surfel"
    _DEPTH_KIND = "z"

    def __init__(self, means, scales, rotations, opacity, sh, degree=None, lr=None, betas=(0.9, 0.999), eps=1e-15, sparse=True,
                 device="cuda", exact_activations=False, deterministic=False, antialiased=False, absgrad=False):
        """GaussianFit's arguments with scales (n, 2) > 0, the standard deviations along the two tangent axes (columns 0 and 1 of
        R(rotations); the normal is column 2).  deterministic, antialiased and absgrad are refused when true (SplatError)."""
        for name, flag in (("deterministic", deterministic), ("antialiased", antialiased), ("absgrad", absgrad)):
            if flag:
                raise _not_built_for_surfels(f"SurfelFit({name}=True)")
        super().__init__(means, scales, rotations, opacity, sh, degree=degree, lr=lr, betas=betas, eps=eps, sparse=sparse, device=device,
                         exact_activations=exact_activations)

    @classmethod
    def from_points(cls, points, colors, degree=3, opacity=0.1, min_sq_distance=1e-7, rotation_seed=0, **kw):
        """2DGS's initialisation: GaussianFit.from_points with the k-NN scale on both tangent axes, and the rotations 2DGS starts
        from, rand((n, 4)): uniform in [0, 1), drawn on the host from a torch.Generator seeded with rotation_seed and uploaded,
        so that a seed gives the same start on every machine."""
        def random_rotations(n, device):
            torch = AG._t()
            gen = torch.Generator(device="cpu")
            gen.manual_seed(int(rotation_seed))
            return torch.rand((n, 4), generator=gen, dtype=torch.float32).to(device)
        return cls._from_points(points, colors, degree, opacity, min_sq_distance, random_rotations, kw)

    def render(self, camera_or_uniforms, width, height, return_depth=False, normals=False, distortion=None, features=None):
        """autograd.render_surfels of the activated parameters (exp and sigmoid; in float64 rounded once with exact_activations;
        no 3D filter): (rgb (H, W, 3), alpha (H, W)[, depth][, dist][, feat]).  return_depth: the ray-surfel intersection depth
        map in clip w (depth_kind="z").  distortion=(near, far): 2DGS's depth-distortion map, after the depth it implies.
        normals=True: the blended normal map (H, W, 3) last, features=autograd.surfel_normals(rotations, means, eye) with the eye
        of the uniforms; a caller's own features are then refused (SplatError).  The frame's records are kept for step()."""
        if normals and features is not None:
            raise SplatError(-1, "SurfelFit.render: normals=True blends the surfels' normals as the frame's features; give features= "
                                 "or normals=True, not both")
        scales, opacity = self._activated()
        if normals:
            features = AG.surfel_normals(self.rotations, self.means, AG._uniforms(camera_or_uniforms, width, height)[16:19])
        *out, rec = AG.render_surfels(camera_or_uniforms, self.means, scales, self.rotations, opacity, sh=self.sh, width=width, height=height,
                                      degree=self.degree, return_depth=return_depth, features=features, distortion=distortion,
                                      return_records=True)
        if rec.requires_grad:
            rec.retain_grad()
        self._frame = (rec, int(width), int(height))
        return tuple(out)

    def densify_and_prune(self, grad_threshold=None, scale_threshold=None, min_opacity=0.05, max_screen_radius=0.0, max_world_scale=0.0,
                          max_splats=0, seed=None):
        """GaussianFit.densify_and_prune with the surfel plan and split (include/splat.h, splat_densify_plan_surfel,
        splat_densify_geometry_surfel: the larger of two scales decides, and a split's children stay in the parent's plane);
        min_opacity defaults to 2DGS's 0.05."""
        return super().densify_and_prune(grad_threshold=grad_threshold, scale_threshold=scale_threshold, min_opacity=min_opacity,
                                         max_screen_radius=max_screen_radius, max_world_scale=max_world_scale, max_splats=max_splats,
                                         seed=seed)

    def save_ply(self, path):
        """The cloud as a 2D Gaussian splatting PLY file (ply.save_surfel_ply): the raw parameters, bit for bit."""
        from .ply import save_surfel_ply
        c = lambda t: t.detach().cpu().numpy()  # noqa: E731
        save_surfel_ply(path, c(self.means), None, c(self.rotations), None, c(self.sh).reshape(self.n, -1, 3), log_scales=c(self.log_scales),
                        opacity_logits=c(self.opacity_logits))


def _not_built_for_surfels(who):
    return SplatError(-1, f"{who}: not built for surfels")


def _refusal(name):
    def method(self, *args, **kw):
        raise _not_built_for_surfels(f"SurfelFit.{name}")
    method.__name__ = name
    method.__doc__ = f"Not built for surfels: SplatError.  (GaussianFit.{name} projects its planes as ellipsoids.)"
    return method


for _name in ("update_filter_3d", "relocate", "add_new", "inject_noise", "accumulate_importance", "importance", "prune_by_importance"):
    setattr(SurfelFit, _name, _refusal(_name))
del _name
