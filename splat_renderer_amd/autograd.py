"""torch autograd for frames of anisotropic 3D Gaussians (footprint="ellipsoid"; an extension, no reference counterpart).

    rec, aux   = project_ellipsoids(uniforms, means, scales, rotations)  # rec (n, 8) differentiable; aux: ProjectedSplats, keys
    col        = sh_colors(eye, means, sh, degree, opacities)             # (n, 4) differentiable (or the caller's own (rgb, opacity))
    rgb, alpha = rasterize(rec, col, aux, width, height)                  # (H, W, 3), (H, W)
    rgb, alpha = render_gaussians(camera_or_uniforms, means, scales, rotations, opacities, colors=None, sh=None, width=..., height=...)

With a depth map (every result differentiable):

    rec, depths, aux   = project_ellipsoids(uniforms, means, scales, rotations, return_depth=True)  # depths (n,) = aux.projected[:, 4]
    rgb, alpha, depth  = rasterize(rec, col, aux, width, height, depths=depths)                      # depth (H, W)
    rgb, alpha, depth  = render_gaussians(..., return_depth=True)

depth is the AOV depth of include/splat.h: per pixel sum w_i z_i / sum w_i over the entries it consumed (w_i = T_i alpha_i,
the colour's own weights), +inf where nothing contributed.  z_i is whatever (n,) tensor is passed as `depths`: the default,
project_ellipsoids' depths, is the distance from the eye to each centre (the depth the sort orders by), not view-space z.  A
caller who wants planar z computes it in torch from `means` (e.g. (means - eye) . forward) and passes that instead; its
gradient flows back through torch.  3DGS's accumulated depth sum w_i z_i is depth * alpha where alpha > 0 (sum w_i = alpha up
to rounding) and 0 elsewhere; torch.where(alpha > 0, depth, 0) * alpha computes it with a finite gradient everywhere (a
gradient through depth * alpha at an empty pixel would multiply by its +inf).  The backward of the depth map is
splat_composite_backward_depth and splat_project_ellipsoid_backward_depth; an upstream gradient at pixels where depth is +inf
is not read, so NaN or inf there is harmless.

Every kernel runs on torch's current stream (a Device created on it, cached per device and stream).  Tensors must be CUDA
float32; there is no CPU path (SplatError).  The forward is the staged frame of include/splat.h (splat_project_ellipsoid ->
sort -> splat_bin_run -> splat_composite_aov), so rasterize's image is Renderer(footprint="ellipsoid")'s bit for bit; the
backward is splat_composite_backward, splat_project_ellipsoid_backward and splat_sh_colors_backward, whose contract (the cut
and the early-out stop held fixed; float atomic sums, reproducible to rounding) is stated in include/splat.h.

rasterize(..., deterministic=True) and render_gaussians(..., deterministic=True) make the backward bit-reproducible: the
composite's backward is then splat_composite_backward_det, which stores each tile's share of a splat's sums to a workspace and
adds them per splat in a documented order (the tiles of each tile row of the splat's rectangle left to right, then the rows
top to bottom, then once into the gradient: include/splat.h) with no float atomics.  Every other kernel of the chain already
sums in a fixed order, so with the flag the same inputs give the same .grad bits on every run, the camera's included.  The
price: the workspace, a torch tensor allocated in backward() and freed after it, of 16 bytes per tile + 4 per splat + 36 per
(tile, splat) pair of the frame's lists (40 with a depth gradient) - about 0.5 GB where the lists hold 12.5 M pairs - and the
time of the stores and the second pass (DESIGN.md section 4 has the measurement).  The default, deterministic=False, is the
atomic path, unchanged: no workspace, reproducible to rounding.

AbsGS's absolute screen-space gradient (include/splat.h, splat_composite_backward_abs; Ye et al. 2024; gsplat's absgrad):

    rgb, alpha       = rasterize(rec, col, aux, width, height, absgrad=True)
    loss.backward();   aux.absgrad                                             # (n, 2): sum |term c.x|, sum |term c.y|
    rgb, alpha, aux  = render_gaussians(..., absgrad=True, return_aux=True);  loss.backward();  aux.absgrad

3DGS densifies by the norm of rec.grad[:, :2], a signed sum over a splat's pixels: where a large splat covers two
under-fitted regions its pixels pull the centre in opposite directions, the sum cancels and the splat is never split.  With
absgrad=True the composite's backward is splat_composite_backward_abs (splat_composite_backward_det_abs with
deterministic=True; the depth variant of either when a depth gradient arrives), which sums the absolute values of the very
per-pixel terms beside the signed sums.  backward() leaves them in aux.absgrad on the ProjectedSplats: a fresh (n, 2) float32
tensor holding this backward's values, zeros for splats no pixel consumed; None before any backward.  It is a statistic, not
a gradient: nothing flows through it, and rec.grad, col.grad and the image are what absgrad=False gives (bit for bit under
deterministic=True, where the signed sums are made by the same additions).  render_gaussians builds its ProjectedSplats
itself, so return_aux=True appends it to the tuple it returns; by default it returns what it always did.  The price: two more
wave sums per list entry on top of nine or ten in the backward's second walk, and 44 (48) instead of 36 (40) bytes per pair of
the deterministic workspace (DESIGN.md section 4 has the measurement).  absgrad=False, the default, is the code path
described above, call for call.

Antialiased frames (include/splat.h, "antialiased frames"; Mip-Splatting's 2D filter, gsplat's rasterize_mode="antialiased"):

    rec, rho, aux          = project_ellipsoids(uniforms, means, scales, rotations, antialiased=True)
    rec, rho, depths, aux  = project_ellipsoids(..., return_depth=True, antialiased=True)
    rgb, alpha             = rasterize(rec, compensate_opacity(col, rho), aux, width, height)
    rgb, alpha             = render_gaussians(..., antialiased=True)

rho (n,) = sqrt(det(Sigma2 - 0.3 I) / det Sigma2) in the projector's binary32 arithmetic, 0 for a culled splat and where the
binary32 det(Sigma2 - 0.3 I) is not positive (needle splats: it cancels); it is differentiable (splat_project_ellipsoid_aa
and splat_project_ellipsoid_backward_aa, one autograd Function; the term is zero where rho is 0), honours return_depth and a
uniforms tensor that requires grad, and keeps the camera sums' fixed order.  render_gaussians multiplies the opacity column by
it with a torch op; the composite, its backward, deterministic=True and photometric_loss are untouched.  antialiased=False,
the default, is the code path described above, call for call.

The camera is differentiable too.  `uniforms` may be a torch tensor (CUDA or CPU, float32 or float64, 22 floats, or 20 with
width= and height=) that requires grad: it is then an input of the projection and, through its [16:19] slice, of sh_colors,
and backward() fills its .grad — dL/dVP in [0:16] (row 2, entries 2, 6, 10, 14, is not read by this footprint: exact zeros),
dL/deye in [16:19] (through the depths and the SH direction), zeros in [19:22] (time is not read; W and H are the screen's
integers, not parameters: no gradient is offered).  The sums over the splats are made by splat_project_ellipsoid_backward_camera
and splat_sh_colors_backward_camera in float64 and in a fixed order: unlike the per-splat gradients they are bit-reproducible
for the same upstream.  Each is one sum over every unculled splat: one ill-conditioned splat (Sigma2 of condition number
beyond 1e4, say) or one NaN in the upstream reaches the whole camera gradient, not one splat's row; mask such splats (zero
their opacity or their upstream) when refining a pose.  The forward still reads a host copy of the block (the C ABI takes host uniforms): one 88-byte
device-to-host copy per frame when the tensor lives on the GPU.  A Camera, a NumPy array or a tensor that does not require
grad takes the code path, the kernels and the results described above, unchanged.  A 4 x 4 VP is not what anyone optimises:
pinhole_uniforms(R, t, fx, fy, cx, cy, width, height) builds the block from a pose and intrinsics in plain torch ops, so that
gradients reach whatever parametrises R and t (axis-angle, quaternion: the caller's choice).

The objective (include/splat.h, "Image loss"):

    loss            = photometric_loss(rgb, target, lambda_dssim=0.2)                     # 0-d tensor, differentiable in rgb
    loss, l1, ssim  = photometric_loss(rgb, target, lambda_dssim=0.2, return_terms=True)  # l1, ssim detached

loss = (1 - lambda) mean|rgb - target| + lambda (1 - SSIM), SSIM over 3DGS's 11 x 11 Gaussian window of sigma 1.5 with zero
padding: one fused kernel forward (splat_image_loss), one backward (splat_image_loss_backward), instead of five grouped
convolutions and their transposes.  rgb is (H, W, 3); the view rasterize returns (the first three channels of its (H, W, 4)
buffer) is read in place with pixel stride 4, a contiguous (H, W, 3) tensor with stride 3, and any other layout is made
contiguous first.  target is (H, W, 3) or (H, W, 4) and gets no gradient; rgb is not clamped.  The two means are summed in
float64 in a fixed order and the backward is a gather: both are bit-reproducible.  The upstream gradient is read on the device,
so backward() does not synchronise.  lambda_dssim = 0 is a plain L1: the SSIM part is not launched (unless return_terms asks
for its value).  No masks: multiply both images by one in torch.

The geometry term (include/splat.h, "Normals of a depth map"):

    normals      = depth_normals(depth, camera_or_uniforms, depth_kind="distance")                       # (H, W, 3), differentiable in depth
    loss         = normal_consistency_loss(normal_map, depth, camera_or_uniforms, weight=None)            # 0-d, differentiable in both
    loss, valid  = normal_consistency_loss(..., return_terms=True)                                        # valid: fraction of pixels with a normal
    n            = splat_normals(means, scales, rotations, eye)                                           # (n, 3), torch ops

depth_normals is the unit normal of the surface a depth map describes: the cross product of the central differences of the
points the four neighbours of a pixel see along the camera's rays, facing the eye whether or not the camera mirrors an axis.  It
is 0, and passes no gradient, on the border, next to an empty (+inf), non-positive or NaN depth, and on screens below 3 x 3.
depth_kind says what the map holds: "distance", |P - eye|, which is what rasterize(depths=) gives from project_ellipsoids'
depths, or "z", clip w.  normal_consistency_loss is 2DGS's normal_error.mean(), mean(1 - weight * normal_map . normals), with
an invalid pixel contributing the constant 1: one fused kernel and a small sum forward (splat_normal_consistency), one kernel
backward for both gradients (splat_normal_consistency_backward), instead of some two dozen element-wise ops over (H, W, 3)
temporaries and their transposes.  normal_map is (H, W, 3) or an (H, W, K >= 3) feature map whose first three channels are the
normal, read in place by its pixel stride (its other channels get zero gradient from this term); weight (2DGS: alpha.detach())
is detached.  Every sum is made in a fixed order without atomics and the backward recomputes instead of storing: no workspace,
the same bits on every run, and the upstream is read on the device, so backward() does not synchronise.  The camera gets no
gradient from this term: a uniforms tensor that requires grad is refused with SplatError (pass uniforms.detach()) rather than
its gradient dropped silently.  Only perspective cameras: an orthographic VP is refused.  splat_normals is the per-splat normal
2DGS blends: the axis of the smallest scale, flipped towards the eye.

`rec` is a real intermediate: rec.retain_grad() gives the screen-space gradient rec.grad[:, :2] that 3DGS densification reads.

The background is the composite's fixed bg = (0.05, 0.05, 0.1).  A caller that wants background b uses
rgb + (b - bg) * (1 - alpha)[..., None], which is exact and differentiable.

Where a fit starts (include/splat.h, "Initialisation from a point cloud"):

    mean_sq = knn_mean_sq_distance(points)   # (n,): per point the mean squared distance to its three nearest neighbours

points is (n, 3) or (n, 4) (the fourth column is not read); the result is the header's contract bit for bit, +inf for a point
with fewer than three usable neighbours or a non-finite coordinate.  No gradient: it is an initialisation.  One call of
splat_knn_mean_sq on torch's current stream, with this module's per-device context and sorter; nothing waits on the host.

What a view sees of every splat (include/splat.h, "Contribution of every splat to a frame"):

    hits, weight_max, weight_sum = contribution(rec, col, aux, width, height, pixel_weight=None, min_weight=0.0, out=None)

Per splat, over the (pixel, consumed entry inside the cut) pairs of the frame rasterize would draw from the same arguments: the
number of pairs whose blend weight w = T alpha (times the pixel's mask) is at least min_weight (int32 holding the uint32 bits),
the largest weight (float32: RadSplat's score once taken over views) and the sum of the weights in units of 2^-24 (int64;
weight_sum.double() * 2 ** -24 is the sum).  A named tuple of three (n,) tensors; out= an earlier result to accumulate into
(one call per view builds the statistic over views: sums add, the maximum is kept).  pixel_weight (H, W) float32 in [0, 1]
masks pixels.  One call of splat_composite_contribution on torch's current stream with this module's per-device context, binned
through the same sorter and binner as rasterize (a pending backward of an earlier rasterize re-bins its own lists, as after any
other frame).  Integer sums and a maximum: the same inputs give the same bytes on every run.  Inputs are detached; no gradient.

Anything else blended with the image's own weights (include/splat.h, "Feature channels of a frame"):

    feat             = composite_features(rec, col, aux, features, width, height)     # (H, W, K), K = features.shape[1] <= 32
    rgb, alpha, feat = rasterize(rec, col, aux, width, height, features=features)    # after depth when depths= is given
    rgb, alpha, feat = render_gaussians(..., features=features)

feat[y, x, k] = sum_i w_i features[i, k] over the entries the pixel consumed, with the colour's own weights w_i = T_i alpha_i:
no background term, no division by sum w, 0 where nothing contributed.  features is (n, K) CUDA float32 (or (n,) for K = 1); a
column slice features[:, a:b] of a wider tensor is read where it lies, by its row stride, without a copy.  It is the caller's
tensor: render_gaussians does not compensate it by rho (rho already sits in the opacity).  The map is differentiable in rec,
in col's opacity column (its colour columns get exact zeros) and in features: a torch.autograd.Function of its own
(splat_composite_features, splat_composite_features_backward), whose rec / col gradients torch adds to Rasterize's - the
backward's recurrence is linear in the upstream, so a feature loss contributes its own additive share.  It reuses the context's
tile lists when they are this projection's for this screen: rasterize followed by composite_features on the same aux sorts
and bins once (a backward after another frame re-bins, as Rasterize's does).  The gradients are float atomic sums,
reproducible to rounding; no fixed-order variant exists, so features together with deterministic=True raises SplatError rather
than mixing a reproducible and a non-reproducible sum.  absgrad keeps counting the colour, alpha and depth terms only.  Without
features= every function runs the calls it always ran.  Measured on one MI355X at 5 M splats, 1920 x 1080:
the map 0.35 ms at K = 3 and 0.37 at K = 8; its backward 1.13 and 1.35 ms beside the image's 1.10.  Two recipes:

    # Normal consistency (2DGS): each splat's shortest axis, flipped towards the eye, blended beside the image and held to the
    # normal of the depth map (below, "The geometry term")
    rgb, alpha, depth, nmap = render_gaussians(cam, means, scales, rotations, opacities, sh=sh, width=W, height=H, return_depth=True,
                                               features=splat_normals(means, scales, rotations, eye))
    loss = photometric_loss(rgb, target) + lam * normal_consistency_loss(nmap, depth, cam, weight=alpha.detach())

    # Depth distortion (Mip-NeRF 360, 2DGS): sum over pairs j < i of w_i w_j (z_i - z_j)^2 = W Q - M^2 from one walk
    rec, depths, aux = project_ellipsoids(cam_uniforms, means, scales, rotations, return_depth=True)
    z = (depths - near) / (far - near)                   # NORMALISE to the scene's depth range first (below)
    W_, M, Q = composite_features(rec, col, aux, torch.stack([torch.ones_like(z), z, z * z], dim=1)).unbind(2)
    distortion = (W_ * Q - M * M).mean()

W Q - M^2 is a difference of products of sums: in binary32 it cancels where the spread of depth within a pixel is small against
the depth itself (z = 100 +- 0.01 leaves no digits), so subtract the near plane and divide by the range before squaring.

2D Gaussian surfels (include/splat.h, "2D Gaussian surfels"; 2DGS): the same planes read as a planar Gaussian, scales x and y along
columns 0 and 1 of R(rotations), normal column 2.

    rec, aux           = project_surfels(uniforms, means, scales, rotations)                       # rec (n, 8): all eight columns
    rec, clip_w, aux   = project_surfels(uniforms, means, scales, rotations, return_depth=True)    # clip_w (n,): the centres' clip w
    rgb, alpha, depth  = rasterize(rec, col, aux, width, height, depths=clip_w)                    # aux says the footprint
    rgb, alpha, depth  = render_surfels(camera_or_uniforms, means, scales, rotations, opacities, colors=..., width=W, height=H,
                                        return_depth=True)

The footprint is the exact ray-surfel intersection, (u, v) = B d / (1 - q.d), not the ellipsoid's affine approximation (q = 0), and
the image is drawn by the ellipsoid's composites over these records.  depth is the intersection depth map sum w z rd / sum w with
rd = 1 / (1 - q.d) (splat_composite_surfel_depth): with z = clip_w it is the clip w of the points the pixel's ray meets the surfels
at, so a large flat surfel reports the plane it lies in, not a constant; +inf where nothing contributed.  It is a depth_kind="z"
map.  Every result is differentiable in means, scales (x, y; a third column gets zeros), rotations, opacities and colours
(splat_composite_backward / _depth with the surfel footprint, splat_project_surfel_backward).  features= and composite_features
blend with the surfel image's own weights (the same entry points under the surfel footprint: their kernels evaluate the whole
record), differentiable in all eight record columns.  project_surfels returns (rec, clip_w, aux), aux last as project_ellipsoids
does.  Not built for surfels, and refused with SplatError rather than run with q ignored: deterministic=True, absgrad=True,
contribution(), and a uniforms tensor that requires grad (no camera gradient yet).  The recipe of 2DGS, image + depth + normal map
+ normal consistency:

    eye = uniforms[16:19]
    rgb, alpha, depth, nmap = render_surfels(cam, means, scales, rotations, opacities, sh=sh, width=W, height=H, return_depth=True,
                                             features=surfel_normals(rotations, means, eye))
    loss = photometric_loss(rgb, target) + lam * normal_consistency_loss(nmap, depth, cam, weight=alpha.detach(), depth_kind="z")

Depth distortion for surfels (2DGS's fourth term).  The (1, z, z^2) recipe above blends one constant per splat, so for a surfel it
sees the centre's depth only; 2DGS's term is over the per-pixel intersection depth t_i = z_i rd_i, whose spread across one surfel is
what flattens surfels onto the surface.  distortion=(near, far), 0 < near < far (far = inf allowed), adds the map
dist = sum_{i > j} w_i w_j (m_i - m_j)^2, m = far (t - near) / ((far - near) t) in [0, 1), 0 where nothing contributed, after depth:

    rgb, alpha, depth, dist, nmap = render_surfels(cam, means, scales, rotations, opacities, sh=sh, width=W, height=H,
                                                   distortion=(near, far), features=surfel_normals(rotations, means, eye))
    loss = photometric_loss(rgb, target) + lam_d * dist.mean() \
        + lam_n * normal_consistency_loss(nmap, depth, cam, weight=alpha.detach(), depth_kind="z")

The map comes from the depth map's own walk (splat_composite_surfel_distortion in place of splat_composite_surfel_depth: depth
keeps its bits), summed front to back over m_i - m_first so that nothing cancels in binary32 (relative L2 of 3e-7 of float64
where W Q - M^2 and the unshifted prefix sums sit at 1e-4), and its gradient joins the image's and the depth map's in one launch
(splat_composite_backward_distortion), to all eight record columns, the opacity and z.  Surfel projections only, and with
depths= (render_surfels: implied): anything else raises SplatError.

torch is imported when a function here is first called, so `import splat_renderer_amd` does not need it.
"""
import collections
import ctypes as C
import types

import numpy as np

from . import _lib
from ._lib import CompositeCfg, SplatError, check

BG = (0.05, 0.05, 0.1)
TILE = 16
MAX_FEATURE_CHANNELS = 32  # include/splat.h, SPLAT_MAX_FEATURE_CHANNELS

_torch = None
_devices = {}


def _t():
    global _torch
    if _torch is None:
        import torch
        _torch = torch
    return _torch


class _Ctx:
    """The splat context on one device and stream, with the sorter and binner the staged frames share.  Each binSplats
    bumps `generation`: a backward whose forward's lists have since been replaced rebuilds them."""

    def __init__(self, index, stream):
        from .host import Device
        self.device = Device(index, stream=stream)
        self.lib = self.device.lib
        self.sorter = None
        self.capacity = 0
        self.padded = 0
        b = C.c_void_p()
        check(self.lib.splat_bin_create(self.device.ctx, TILE, C.byref(b)), self.device.ctx)
        self.binner = b
        self.generation = 0
        self.total = 0

    @property
    def ctx(self):
        return self.device.ctx

    def ensure_sorter(self, n):
        if self.sorter is None or n > self.capacity:
            if self.sorter is not None:
                self.lib.splat_sort_destroy(self.sorter)
                self.sorter = None
            s = C.c_void_p()
            cap = max(n, 1)
            check(self.lib.splat_sort_create(self.ctx, cap, C.byref(s)), self.ctx)
            self.sorter, self.capacity = s, cap
            self.padded = int(self.lib.splat_sort_capacity(s))
        return self.padded

    def bin(self, aux, width, height):
        """sort aux's keys, bin with its ProjectedSplats: the lists of one frame; returns this binning's generation."""
        lib, ctx, n = self.lib, self.ctx, aux.n
        self.ensure_sorter(n)
        if aux.keys.numel() > self.padded:
            raise SplatError(-1, "rasterize: the projection's keys outgrew the sorter")
        kb = aux.keys.numel() * 4
        check(lib.splat_buf_copy(ctx, lib.splat_sort_keys(self.sorter), aux.keys.data_ptr(), kb), ctx)
        check(lib.splat_buf_copy(ctx, lib.splat_sort_payload(self.sorter), aux.payload.data_ptr(), kb), ctx)
        check(lib.splat_sort_run(self.sorter, n, 0, 32), ctx)
        args = (self.binner, aux.projected.data_ptr(), n, lib.splat_sort_sorted_payload(self.sorter), n, width, height, 0, _lib.U32_MAX)
        check(lib.splat_bin_run(*args), ctx)
        # the binner is sync-free: lists that outgrew the pair limit it sized from the frame before are reported here (the
        # limit has been raised then), and binned again
        total = C.c_uint64()
        rc = lib.splat_bin_total(self.binner, C.byref(total))
        if rc in _lib.RENDER_AGAIN:
            check(lib.splat_bin_run(*args), ctx)
            rc = lib.splat_bin_total(self.binner, C.byref(total))
        check(rc, ctx)
        self.total = int(total.value)  # (the lists' pairs: what sizes the deterministic backward's workspace)
        self.generation += 1
        aux.binned = (self.generation, int(width), int(height))  # (lists_for: whose lists the binner holds)
        return self.generation

    def lists_for(self, aux, width, height):
        """The lists of aux's frame on this screen: the binner's current ones when they are that frame's (the last bin() was
        this projection's for this screen), else binned now."""
        if aux.binned != (self.generation, int(width), int(height)):
            self.bin(aux, width, height)
        return self.lists()

    def lists(self):
        out = []
        for fn in (self.lib.splat_bin_indices, self.lib.splat_bin_counts, self.lib.splat_bin_offsets):
            p = C.c_void_p()
            check(fn(self.binner, C.byref(p)), self.ctx)
            out.append(p.value)
        return out


def _context(tensor):
    torch = _t()
    index = tensor.device.index if tensor.device.index is not None else torch.cuda.current_device()
    stream = torch.cuda.current_stream(index).cuda_stream
    key = (index, stream)
    c = _devices.get(key)
    if c is None:
        c = _devices[key] = _Ctx(index, stream)
    return c


def _cuda_f32(t, name, cols=None):
    """A contiguous 16-byte-aligned CUDA float32 tensor, or SplatError."""
    torch = _t()
    if not isinstance(t, torch.Tensor):
        raise SplatError(-1, f"{name} must be a torch tensor")
    if not t.is_cuda:
        raise SplatError(-1, f"{name} is on {t.device}: splat_renderer_amd has no CPU path")
    if t.dtype != torch.float32:
        raise SplatError(-1, f"{name} must be float32, not {t.dtype}")
    if cols is not None and (t.dim() != 2 or t.shape[1] != cols):
        raise SplatError(-1, f"{name} must have shape (n, {cols}), not {tuple(t.shape)}")
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone()
    if t.data_ptr() % 16:
        raise SplatError(-1, f"{name} is not 16-byte aligned")
    return t


def _vec4(t, name, fill=0.0):
    """(n, 3) -> (n, 4) with torch ops (outside the Functions, so autograd handles the slice)."""
    _cuda_f32(t, name)
    if t.dim() != 2 or t.shape[1] not in (3, 4):
        raise SplatError(-1, f"{name} must have shape (n, 3) or (n, 4), not {tuple(t.shape)}")
    if t.shape[1] == 3:
        t = _t().cat([t, t.new_full((t.shape[0], 1), fill)], dim=1)
    return t


def _uniforms(camera_or_uniforms, width, height):
    if hasattr(camera_or_uniforms, "uniforms"):
        u = camera_or_uniforms.uniforms(width, height)
    else:
        u = camera_or_uniforms
        if hasattr(u, "detach"):
            u = u.detach().cpu().numpy()
        u = np.asarray(u, np.float32).reshape(-1)
        if u.shape[0] < 20:
            raise SplatError(-1, "uniform block needs 22 floats (VP, eye, time, screenW, screenH)")
        u = u.copy() if u.shape[0] >= 22 else np.concatenate([u[:20], np.zeros(2, np.float32)])
        if width is not None:
            u[20], u[21] = width, height
    return np.ascontiguousarray(u, np.float32)


def _grad_uniforms(u, name="uniforms", sizes=(20, 22)):
    """`u` itself when it is a torch tensor that requires grad (checked: float32 / float64, 20 or 22 floats), else None."""
    if not getattr(u, "requires_grad", False):  # (a Camera, a NumPy array, a tensor that does not: the constant-camera path)
        return None
    torch = _t()
    if u.dtype not in (torch.float32, torch.float64):
        raise SplatError(-1, f"{name} that requires grad must be float32 or float64, not {u.dtype}")
    if u.numel() not in sizes:
        raise SplatError(-1, f"{name} that requires grad must hold {' or '.join(map(str, sizes))} floats, not {u.numel()}")
    return u


def _like(g, t):
    """The first t.numel() floats of the float32 device vector g, as a gradient for t (its shape, dtype and device)."""
    return g[:t.numel()].to(device=t.device, dtype=t.dtype).reshape(t.shape)


def _fptr(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


class ProjectedSplats:
    """What rasterize needs of a projection beside its records: ProjectedSplat records (n, 8), depth keys and payload (padded
    to the sorter's capacity), the uniforms and the inputs (for the projector's backward).  No gradient flows through it.
    absgrad: None, or after the backward of a rasterize(absgrad=True) over this projection the (n, 2) sums of |term c.x|,
    |term c.y| (the module's docstring)."""

    def __init__(self, ctx, u, n, projected, keys, payload, footprint=_lib.FOOTPRINT_ELLIPSOID):
        self.ctx, self.u, self.n = ctx, u, n
        self.footprint = footprint  # (FOOTPRINT_SURFEL: project_surfels' records; rasterize reads it)
        self.absgrad = None
        self.binned = None  # (generation, width, height) of the context's binning of this projection, once there is one
        self.projected, self.keys, self.payload = projected, keys, payload
        self.width, self.height = int(u[20]), int(u[21])


def _ellipsoid_cfg(footprint=_lib.FOOTPRINT_ELLIPSOID):
    """The one composite configuration the ellipsoid footprint's backward and contribution kernels accept (footprint: the
    projection's, ProjectedSplats.footprint; the surfel's kernels take the same configuration under their own footprint)."""
    return CompositeCfg(_lib.MODE_FRONT_TO_BACK, 1, TILE, 0, _lib.U32_MAX, _lib.RECORDS_PROJECTED, 1, footprint)


def _is_surfel(aux):
    return aux.footprint == _lib.FOOTPRINT_SURFEL


# Rasterize.backward's entry point: (deterministic, absgrad, a depth gradient arrived) -> its name.  The _det and _abs entry
# points take the four depth arguments always (all NULL / 0: colour only).
_COMPOSITE_BACKWARD = {
    (False, False, False): "splat_composite_backward", (False, False, True): "splat_composite_backward_depth",
    (False, True, False): "splat_composite_backward_abs", (False, True, True): "splat_composite_backward_abs",
    (True, False, False): "splat_composite_backward_det", (True, False, True): "splat_composite_backward_det",
    (True, True, False): "splat_composite_backward_det_abs", (True, True, True): "splat_composite_backward_det_abs",
}


def _functions():
    """The autograd Functions, by name, built on first use (torch imported then).  Each is applied with its full argument
    list, and each backward returns one entry per argument (None for what is no tensor or needs no gradient)."""
    torch = _t()
    if "_fns" in globals():
        return globals()["_fns"]

    class Project(torch.autograd.Function):
        """splat_project_ellipsoid, or with antialiased splat_project_ellipsoid_aa (the 2D Mip filter's factor rho beside the
        records), and their backwards.  Returns (rec, [rho,] [depths,] aux)."""

        @staticmethod
        def forward(fctx, u, means4, scales4, rots, with_depth, u_t, antialiased):
            # (u_t: the uniforms as the tensor that requires grad, or None; the kernels read the host copy u)
            cx = _context(means4)
            n = means4.shape[0]
            dev = means4.device
            padded = cx.ensure_sorter(n)
            rec = torch.empty((n, 8), device=dev, dtype=torch.float32)
            proj = torch.empty((n, 8), device=dev, dtype=torch.float32)
            rho = torch.empty(n, device=dev, dtype=torch.float32) if antialiased else None
            keys = torch.empty(padded, device=dev, dtype=torch.int32)
            pay = torch.empty(padded, device=dev, dtype=torch.int32)
            args = (cx.ctx, _fptr(u), means4.data_ptr(), 1, scales4.data_ptr(), 1, rots.data_ptr(), 1, n, proj.data_ptr(), rec.data_ptr(),
                    keys.data_ptr(), pay.data_ptr(), padded)
            if n and antialiased:
                check(cx.lib.splat_project_ellipsoid_aa(*args, rho.data_ptr(), None, 1, None), cx.ctx)
            elif n:
                check(cx.lib.splat_project_ellipsoid(*args), cx.ctx)
            fctx.save_for_backward(means4, scales4, rots)
            fctx.u, fctx.u_t, fctx.with_depth, fctx.antialiased = u, u_t, with_depth, antialiased
            fctx.set_materialize_grads(False)  # (an unused rho or depth: None, and the kernel without it)
            out = [rec]
            if antialiased:
                out.append(rho)
            if with_depth:  # (the ProjectedSplat depth, as a tensor of its own: bit for bit aux.projected[:, 4])
                out.append(proj[:, 4].contiguous())
            return (*out, ProjectedSplats(cx, u, n, proj, keys, pay))

        @staticmethod
        def backward(fctx, grad_rec, *grads):
            grads = list(grads[:-1])  # ([rho,] [depths]; the last is aux's)
            grad_rho = grads.pop(0) if fctx.antialiased else None
            grad_depth = grads.pop(0) if fctx.with_depth else None
            means4, scales4, rots = fctx.saved_tensors
            n = means4.shape[0]
            cx = _context(means4)
            dev = means4.device
            cam = fctx.needs_input_grad[5]
            g = _cuda_f32(grad_rec, "grad_records", 8) if grad_rec is not None else torch.zeros((n, 8), device=dev, dtype=torch.float32)
            gz = _cuda_f32(grad_depth.reshape(-1), "grad_depths") if grad_depth is not None else None
            gp, gs, gr = (torch.empty((n, 4), device=dev, dtype=torch.float32) for _ in range(3))
            gu = torch.empty(24, device=dev, dtype=torch.float32) if cam else None  # (22, and a 16-byte multiple)
            args = (cx.ctx, _fptr(fctx.u), means4.data_ptr(), 1, scales4.data_ptr(), 1, rots.data_ptr(), 1, n, g.data_ptr(), gp.data_ptr(),
                    gs.data_ptr(), gr.data_ptr())
            gz_ptr = gz.data_ptr() if gz is not None and n else None
            if fctx.antialiased:
                grho = _cuda_f32(grad_rho.reshape(-1), "grad_rho") if grad_rho is not None else torch.zeros(n, device=dev, dtype=torch.float32)
                if n or cam:
                    check(cx.lib.splat_project_ellipsoid_backward_aa(*args, gz_ptr, gu.data_ptr() if cam else None, grho.data_ptr()), cx.ctx)
            elif cam:
                check(cx.lib.splat_project_ellipsoid_backward_camera(*args, gz_ptr, gu.data_ptr()), cx.ctx)
            elif n and gz is None:
                check(cx.lib.splat_project_ellipsoid_backward(*args), cx.ctx)
            elif n:
                check(cx.lib.splat_project_ellipsoid_backward_depth(*args, gz_ptr), cx.ctx)
            return None, gp, gs, gr, None, (_like(gu, fctx.u_t) if cam else None), None

    class ProjectSurfel(torch.autograd.Function):
        """splat_project_surfel and splat_project_surfel_backward.  Returns (rec, [clip_w,] aux)."""

        @staticmethod
        def forward(fctx, u, means4, scales4, rots, with_depth):
            cx = _context(means4)
            n = means4.shape[0]
            dev = means4.device
            padded = cx.ensure_sorter(n)
            rec = torch.empty((n, 8), device=dev, dtype=torch.float32)
            proj = torch.empty((n, 8), device=dev, dtype=torch.float32)
            cw = torch.empty(n, device=dev, dtype=torch.float32) if with_depth else None
            keys = torch.empty(padded, device=dev, dtype=torch.int32)
            pay = torch.empty(padded, device=dev, dtype=torch.int32)
            if n:
                check(cx.lib.splat_project_surfel(cx.ctx, _fptr(u), means4.data_ptr(), 1, scales4.data_ptr(), 1, rots.data_ptr(), 1, n,
                                                  proj.data_ptr(), rec.data_ptr(), keys.data_ptr(), pay.data_ptr(), padded,
                                                  cw.data_ptr() if with_depth else None), cx.ctx)
            fctx.save_for_backward(means4, scales4, rots)
            fctx.u, fctx.with_depth = u, with_depth
            fctx.set_materialize_grads(False)
            aux = ProjectedSplats(cx, u, n, proj, keys, pay, _lib.FOOTPRINT_SURFEL)
            return (rec, cw, aux) if with_depth else (rec, aux)

        @staticmethod
        def backward(fctx, grad_rec, *grads):
            grad_cw = grads[0] if fctx.with_depth else None
            means4, scales4, rots = fctx.saved_tensors
            n = means4.shape[0]
            cx = _context(means4)
            dev = means4.device
            g = _cuda_f32(grad_rec, "grad_records", 8) if grad_rec is not None else torch.zeros((n, 8), device=dev, dtype=torch.float32)
            gw = _cuda_f32(grad_cw.reshape(-1), "grad_clip_w") if grad_cw is not None else None
            gp, gs, gr = (torch.empty((n, 4), device=dev, dtype=torch.float32) for _ in range(3))
            if n:
                check(cx.lib.splat_project_surfel_backward(cx.ctx, _fptr(fctx.u), means4.data_ptr(), 1, scales4.data_ptr(), 1, rots.data_ptr(), 1,
                                                           n, g.data_ptr(), gw.data_ptr() if gw is not None else None, gp.data_ptr(),
                                                           gs.data_ptr(), gr.data_ptr()), cx.ctx)
            return None, gp, gs, gr, None

    class ShColors(torch.autograd.Function):
        @staticmethod
        def forward(fctx, eye, means4, sh, degree, opacities, eye_t):
            # (eye_t: the eye as the tensor that requires grad, or None; the kernels read the host copy eye)
            cx = _context(means4)
            n = means4.shape[0]
            out = torch.empty((n, 4), device=means4.device, dtype=torch.float32)
            if n:
                check(cx.lib.splat_sh_colors(cx.ctx, _fptr(eye), means4.data_ptr(), 1, sh.data_ptr(), sh.shape[1], degree, opacities.data_ptr(), n,
                                             out.data_ptr()), cx.ctx)
            fctx.save_for_backward(means4, sh, opacities)
            fctx.eye, fctx.degree, fctx.eye_t = eye, degree, eye_t
            return out

        @staticmethod
        def backward(fctx, grad_col):
            means4, sh, opacities = fctx.saved_tensors
            n = means4.shape[0]
            cx = _context(means4)
            cam = fctx.needs_input_grad[5]
            g = _cuda_f32(grad_col, "grad_color_opacity", 4)
            gsh = torch.zeros_like(sh)
            gp = torch.empty((n, 4), device=means4.device, dtype=torch.float32)
            gop = torch.empty(n, device=means4.device, dtype=torch.float32)
            ge = torch.empty(4, device=means4.device, dtype=torch.float32) if cam else None
            args = (cx.ctx, _fptr(fctx.eye), means4.data_ptr(), 1, sh.data_ptr(), sh.shape[1], fctx.degree, opacities.data_ptr(), g.data_ptr(), n,
                    gsh.data_ptr(), gp.data_ptr(), gop.data_ptr())
            if cam:
                check(cx.lib.splat_sh_colors_backward_camera(*args, ge.data_ptr()), cx.ctx)
            elif n:
                check(cx.lib.splat_sh_colors_backward(*args), cx.ctx)
            return None, gp, gsh, None, gop, (_like(ge, fctx.eye_t) if cam else None)

    class Rasterize(torch.autograd.Function):
        @staticmethod
        def forward(fctx, rec, col, aux, width, height, depths, deterministic, absgrad, distortion=None):
            cx = aux.ctx
            out = torch.empty((height, width, 4), device=rec.device, dtype=torch.float32)
            alpha = torch.empty((height, width), device=rec.device, dtype=torch.float32)
            gen = cx.bin(aux, width, height)
            idx, cnt, off = cx.lists()
            cfg = _ellipsoid_cfg(aux.footprint)
            surfel = _is_surfel(aux)
            depth = torch.empty((height, width), device=rec.device, dtype=torch.float32) if depths is not None else None
            aov = _lib.Aov(depth.data_ptr() if depth is not None and not surfel else None, alpha.data_ptr(), None)
            args = (cx.ctx, C.byref(cfg), col.data_ptr(), 1, None, 1, rec.data_ptr(), idx, cnt, off, width, height, None, out.data_ptr(), None,
                    C.byref(aov))
            if depths is None or surfel:
                check(cx.lib.splat_composite_aov(*args), cx.ctx)
            else:
                check(cx.lib.splat_composite_aov_depth(*args, depths.data_ptr(), 1), cx.ctx)
            dist = None
            if depths is not None and surfel and distortion is not None:  # the same walk writes the distortion map beside it
                dist = torch.empty((height, width), device=rec.device, dtype=torch.float32)
                check(cx.lib.splat_composite_surfel_distortion(cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), idx, cnt, off, width,
                                                               height, depths.data_ptr(), 1, aux.n, depth.data_ptr(), None, distortion[0],
                                                               distortion[1], dist.data_ptr()), cx.ctx)
            elif depths is not None and surfel:  # the intersection depth sum w z rd / sum w: a walk of its own over the same lists
                check(cx.lib.splat_composite_surfel_depth(cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), idx, cnt, off, width, height,
                                                          depths.data_ptr(), 1, aux.n, depth.data_ptr(), None), cx.ctx)
            fctx.distortion = distortion
            fctx.save_for_backward(rec, col, depths)
            fctx.set_materialize_grads(False)  # (an unused depth map: None, and the colour-only kernel)
            fctx.aux, fctx.gen, fctx.wh = aux, gen, (width, height)
            fctx.deterministic, fctx.absgrad = deterministic, absgrad
            rgb = out[..., :3]
            if dist is not None:
                return rgb, alpha, depth, dist
            return (rgb, alpha) if depths is None else (rgb, alpha, depth)

        @staticmethod
        def backward(fctx, grad_rgb, grad_alpha, grad_depth_map=None, grad_dist_map=None):
            rec, col, depths = fctx.saved_tensors
            aux = fctx.aux
            cx = aux.ctx
            dev = rec.device
            width, height = fctx.wh
            n = aux.n
            if cx.generation != fctx.gen:  # the binner has binned another frame since: rebuild this frame's lists (deterministic)
                fctx.gen = cx.bin(aux, width, height)
            idx, cnt, off = cx.lists()
            g = torch.zeros((height, width, 4), device=dev, dtype=torch.float32)
            if grad_rgb is not None:
                g[..., :3] = grad_rgb
            if grad_alpha is not None:
                g[..., 3] = grad_alpha
            grec = torch.zeros((n, 8), device=dev, dtype=torch.float32)
            gcol = torch.zeros((n, 4), device=dev, dtype=torch.float32)
            det, absgrad = fctx.deterministic, fctx.absgrad
            with_dist = fctx.distortion is not None and grad_dist_map is not None
            with_depth = depths is not None and grad_depth_map is not None
            gd = _cuda_f32(grad_depth_map, "grad_depth") if with_depth else None
            gz = torch.zeros(n, device=dev, dtype=torch.float32) if with_depth or with_dist else None
            # absgrad: beside the signed sums, sum |term c.x| and sum |term c.y|, left on the projection
            gabs = torch.zeros((n, 2), device=dev, dtype=torch.float32) if absgrad else None
            if n and with_dist:  # one launch: the image's, the depth map's (when it has an upstream) and the distortion's gradients
                gdist = _cuda_f32(grad_dist_map, "grad_distortion")
                check(cx.lib.splat_composite_backward_distortion(cx.ctx, C.byref(_ellipsoid_cfg(aux.footprint)), col.data_ptr(), 1, rec.data_ptr(),
                                                                 idx, cnt, off, width, height, g.data_ptr(), n, grec.data_ptr(), gcol.data_ptr(),
                                                                 depths.data_ptr(), 1, gd.data_ptr() if with_depth else None, gz.data_ptr(),
                                                                 fctx.distortion[0], fctx.distortion[1], gdist.data_ptr()), cx.ctx)
            elif n:
                name = _COMPOSITE_BACKWARD[det, absgrad, with_depth]
                cfg = _ellipsoid_cfg(aux.footprint)
                head, lists = [cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr()], [idx, cnt, off]
                frame = [width, height, g.data_ptr(), n, grec.data_ptr(), gcol.data_ptr()]
                if with_depth:
                    frame += [depths.data_ptr(), 1, gd.data_ptr(), gz.data_ptr()]
                elif det or absgrad:
                    frame += [None, 0, None, None]
                if det:  # the fixed-order sums: the ProjectedSplats, the lists' pairs and a workspace sized from them
                    tiles = ((width + TILE - 1) // TILE) * ((height + TILE - 1) // TILE)
                    nbytes = int(getattr(cx.lib, name + "_workspace_bytes")(cx.total, tiles, n, int(with_depth)))
                    ws = torch.empty((nbytes + 15) // 16 * 4, device=dev, dtype=torch.int32)
                    args = head + [aux.projected.data_ptr()] + lists + [cx.total] + frame + [ws.data_ptr(), nbytes]
                else:
                    args = head + lists + frame
                if absgrad:
                    args.append(gabs.data_ptr())
                check(getattr(cx.lib, name)(*args), cx.ctx)
            if absgrad:
                aux.absgrad = gabs
            return grec, gcol, None, None, None, gz, None, None, None

    class CompositeFeatures(torch.autograd.Function):
        """splat_composite_features and splat_composite_features_backward over the projection's lists.  feats: (n, K), its rows
        feats.stride(0) floats apart (a column slice of a wider tensor is read where it lies)."""

        @staticmethod
        def forward(fctx, rec, col, aux, feats, width, height):
            cx = aux.ctx
            n, k = aux.n, feats.shape[1]
            out = torch.empty((height, width, k), device=rec.device, dtype=torch.float32)
            idx, cnt, off = cx.lists_for(aux, width, height)
            cfg = _ellipsoid_cfg(aux.footprint)
            check(cx.lib.splat_composite_features(cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), idx, cnt, off, width, height,
                                                  feats.data_ptr() if n else None, max(int(feats.stride(0)), k), k, n, out.data_ptr()), cx.ctx)
            fctx.save_for_backward(rec, col, feats)
            fctx.aux, fctx.wh = aux, (width, height)
            return out

        @staticmethod
        def backward(fctx, grad_map):
            rec, col, feats = fctx.saved_tensors
            aux = fctx.aux
            cx = aux.ctx
            width, height = fctx.wh
            n, k = aux.n, feats.shape[1]
            idx, cnt, off = cx.lists_for(aux, width, height)  # (another frame binned since: this frame's lists again)
            g = grad_map.to(torch.float32).contiguous()
            grec = torch.zeros((n, 8), device=rec.device, dtype=torch.float32)
            gcol = torch.zeros((n, 4), device=rec.device, dtype=torch.float32)
            gfeat = torch.zeros((n, k), device=rec.device, dtype=torch.float32)
            if n:
                cfg = _ellipsoid_cfg(aux.footprint)
                check(cx.lib.splat_composite_features_backward(cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), idx, cnt, off, width,
                                                               height, feats.data_ptr(), max(int(feats.stride(0)), k), k, g.data_ptr(), n,
                                                               grec.data_ptr(), gcol.data_ptr(), gfeat.data_ptr(), k), cx.ctx)
            return grec, gcol, None, gfeat, None, None

    class PhotometricLoss(torch.autograd.Function):
        @staticmethod
        def forward(fctx, x, xs, y, ys, lam, want_ssim):
            # (x, y: tensors whose data_ptr() is an image of pixel stride xs, ys floats; x (H, W, 3), perhaps a view)
            cx = _context(x)
            h, w = x.shape[0], x.shape[1]
            out = torch.empty(4, device=x.device, dtype=torch.float32)
            nbytes = int(cx.lib.splat_image_loss_workspace_bytes(w, h)) if (lam > 0.0 or want_ssim) else 0
            ws = torch.empty(nbytes // 4, device=x.device, dtype=torch.float32) if nbytes else None
            check(cx.lib.splat_image_loss(cx.ctx, x.data_ptr(), xs, y.data_ptr(), ys, w, h, lam, ws.data_ptr() if nbytes else None, nbytes,
                                          out.data_ptr()), cx.ctx)
            fctx.save_for_backward(x, y, ws)
            fctx.args = (xs, ys, lam, nbytes)
            fctx.set_materialize_grads(False)
            loss, l1, ssim = out[0], out[1], out[2]
            fctx.mark_non_differentiable(l1, ssim)
            return loss, l1, ssim

        @staticmethod
        def backward(fctx, grad_loss, *_):
            if grad_loss is None:
                return (None,) * 6
            x, y, ws = fctx.saved_tensors
            xs, ys, lam, nbytes = fctx.args
            cx = _context(x)
            h, w = x.shape[0], x.shape[1]
            up = grad_loss.to(torch.float32).reshape(1).contiguous()
            g = torch.empty((h, w, 3), device=x.device, dtype=torch.float32)
            check(cx.lib.splat_image_loss_backward(cx.ctx, x.data_ptr(), xs, y.data_ptr(), ys, w, h, lam,
                                                   ws.data_ptr() if nbytes and lam > 0.0 else None, nbytes, up.data_ptr(), g.data_ptr(), 3), cx.ctx)
            return g, None, None, None, None, None

    class DepthNormals(torch.autograd.Function):
        @staticmethod
        def forward(fctx, depth, u, kind):
            cx = _context(depth)
            h, w = depth.shape
            out = torch.empty((h, w, 3), device=depth.device, dtype=torch.float32)
            check(cx.lib.splat_depth_normals(cx.ctx, _fptr(u), kind, depth.data_ptr(), w, h, out.data_ptr(), 3), cx.ctx)
            fctx.save_for_backward(depth)
            fctx.args = (u, kind)
            return out

        @staticmethod
        def backward(fctx, grad_normals):
            depth, = fctx.saved_tensors
            u, kind = fctx.args
            cx = _context(depth)
            h, w = depth.shape
            g, gs = _image(grad_normals, "the gradient of the normals", (3,))
            gz = torch.empty((h, w), device=depth.device, dtype=torch.float32)
            check(cx.lib.splat_depth_normals_backward(cx.ctx, _fptr(u), kind, depth.data_ptr(), w, h, g.data_ptr(), gs, gz.data_ptr()), cx.ctx)
            return gz, None, None

    class NormalConsistency(torch.autograd.Function):
        @staticmethod
        def forward(fctx, nmap, ms, depth, weight, u, kind):
            # (nmap: a tensor whose data_ptr() is an image of pixel stride ms floats, (H, W, K >= 3), perhaps a view)
            cx = _context(depth)
            h, w = depth.shape
            out = torch.empty(4, device=depth.device, dtype=torch.float32)
            check(cx.lib.splat_normal_consistency(cx.ctx, _fptr(u), kind, depth.data_ptr(), nmap.data_ptr(), ms,
                                                  weight.data_ptr() if weight is not None else None, w, h, out.data_ptr()), cx.ctx)
            fctx.save_for_backward(nmap, depth, weight)
            fctx.args = (ms, u, kind)
            fctx.set_materialize_grads(False)
            loss, valid = out[0], out[1]
            fctx.mark_non_differentiable(valid)
            return loss, valid

        @staticmethod
        def backward(fctx, grad_loss, *_):
            if grad_loss is None:
                return (None,) * 6
            nmap, depth, weight = fctx.saved_tensors
            ms, u, kind = fctx.args
            cx = _context(depth)
            h, w = depth.shape
            up = grad_loss.to(torch.float32).reshape(1).contiguous()
            k = nmap.shape[2]
            gmap = torch.empty((h, w, 3), device=depth.device, dtype=torch.float32) if k == 3 else \
                torch.zeros((h, w, k), device=depth.device, dtype=torch.float32)  # (channels past the normal: no gradient from this term)
            gz = torch.empty((h, w), device=depth.device, dtype=torch.float32)
            check(cx.lib.splat_normal_consistency_backward(cx.ctx, _fptr(u), kind, depth.data_ptr(), nmap.data_ptr(), ms,
                                                           weight.data_ptr() if weight is not None else None, w, h, up.data_ptr(),
                                                           gmap.data_ptr(), k, gz.data_ptr()), cx.ctx)
            return gmap, None, gz, None, None, None

    fns = globals()["_fns"] = types.SimpleNamespace(Project=Project, ProjectSurfel=ProjectSurfel, ShColors=ShColors, Rasterize=Rasterize, CompositeFeatures=CompositeFeatures,
                                                  PhotometricLoss=PhotometricLoss, DepthNormals=DepthNormals, NormalConsistency=NormalConsistency)
    return fns


def project_ellipsoids(uniforms, means, scales, rotations, width=None, height=None, return_depth=False, antialiased=False):
    """(rec (n, 8) differentiable records {c.x, c.y, B00, B01, 0, B11, 0, 0}, aux: ProjectedSplats).  uniforms: a Camera (then
    width and height are required) or the 22-float block.  return_depth=True: (rec, depths, aux), depths (n,) the
    differentiable ProjectedSplat depth |mean - eye| (aux.projected[:, 4] bit for bit; rasterize's `depths`).  A uniforms
    tensor that requires grad receives its gradient (the module's docstring).  antialiased=True: (rec, rho, aux) or (rec, rho,
    depths, aux), rho (n,) the differentiable 2D Mip filter factor (splat_project_ellipsoid_aa; rec, depths and aux are the
    same bits either way)."""
    u = _uniforms(uniforms, width, height)
    u_t = _grad_uniforms(uniforms)
    means4 = _cuda_f32(_vec4(means, "means", 1.0), "means", 4)
    scales4 = _cuda_f32(_vec4(scales, "scales"), "scales", 4)
    rots = _cuda_f32(rotations, "rotations", 4)
    if not (means4.shape[0] == scales4.shape[0] == rots.shape[0]):
        raise SplatError(-1, "means, scales and rotations must hold the same number of splats")
    return _functions().Project.apply(u, means4, scales4, rots, bool(return_depth), u_t, bool(antialiased))


def _refuse_surfel_camera_grad(uniforms, who):
    """No camera gradient exists for surfels yet: a uniforms tensor that requires grad is refused rather than its gradient dropped
    silently (as _ray_uniforms does for the normals of a depth map)."""
    if getattr(uniforms, "requires_grad", False):
        raise SplatError(-1, f"{who}: the uniforms tensor requires grad, and surfels offer no camera gradient yet; pass uniforms.detach()")


def project_surfels(uniforms, means, scales, rotations, width=None, height=None, return_depth=False):
    """(rec (n, 8) differentiable surfel records {c.x, c.y, B00, B01, B10, B11, q0, q1}, aux: ProjectedSplats of
    footprint SURFEL).  A surfel is the ellipsoid's planes read as a 2D Gaussian (the module's docstring): scales x and y along
    columns 0 and 1 of R(rotations), normal column 2; a third scale column is ignored and gets a zero gradient.
    return_depth=True: (rec, clip_w, aux), aux last as in project_ellipsoids' (rec, depths, aux); clip_w (n,) the differentiable
    clip w of each centre (0 for a culled surfel): the z_i of rasterize's intersection depth map.  uniforms: a Camera (then width and height are required) or the 22-float block; one
    that requires grad is refused (SplatError)."""
    _refuse_surfel_camera_grad(uniforms, "project_surfels")
    u = _uniforms(uniforms, width, height)
    means4 = _cuda_f32(_vec4(means, "means", 1.0), "means", 4)
    if isinstance(scales, _t().Tensor) and scales.dim() == 2 and scales.shape[1] == 2:
        scales = _t().cat([scales, scales.new_zeros((scales.shape[0], 2))], dim=1)
    scales4 = _cuda_f32(_vec4(scales, "scales"), "scales", 4)
    rots = _cuda_f32(rotations, "rotations", 4)
    if not (means4.shape[0] == scales4.shape[0] == rots.shape[0]):
        raise SplatError(-1, "means, scales and rotations must hold the same number of splats")
    return _functions().ProjectSurfel.apply(u, means4, scales4, rots, bool(return_depth))


def surfel_normals(rotations, means, eye):
    """(n, 3): each surfel's normal, column 2 of R(q) of the normalised quaternion (w, x, y, z), flipped so that it faces the eye;
    torch ops, any device, differentiable in rotations (the sign held fixed).  Pass it as render_surfels' features for 2DGS's
    normal map."""
    torch = _t()
    q = rotations / rotations.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    axis = torch.stack([2 * (x * z + r * y), 2 * (y * z - r * x), 1 - 2 * (x * x + y * y)], dim=1)
    eye = torch.as_tensor(eye, dtype=means.dtype, device=means.device).reshape(3)
    return torch.where(((means[:, :3] - eye) * axis).sum(dim=1, keepdim=True) > 0, -axis, axis)


def render_surfels(camera_or_uniforms, means, scales, rotations, opacities, colors=None, sh=None, width=None, height=None, degree=None,
                   return_depth=False, features=None, return_aux=False, distortion=None, return_records=False):
    """render_gaussians' surfel twin: project_surfels, the colour (sh_colors when `sh` is given, else cat(colors, opacities)),
    rasterize.  Returns (rgb (H, W, 3), alpha (H, W)); return_depth=True: (rgb, alpha, depth (H, W)), the ray-surfel
    intersection depth map sum w z rd / sum w in clip w (depth_kind="z" for depth_normals and normal_consistency_loss), +inf where
    nothing contributed; features ((n, K) or (n,)): rasterize's, blended with the surfel image's own weights, the map after depth:
    (rgb, alpha[, depth], feat[, aux]); return_aux=True appends the frame's ProjectedSplats.  distortion=(near, far) implies
    return_depth=True and adds rasterize's depth-distortion map after depth: (rgb, alpha, depth, dist[, feat][, aux]).
    return_records=True appends, last of all, the frame's differentiable records (n, 8): what SurfelFit keeps for its density
    statistics."""
    if width is None or height is None:
        raise SplatError(-1, "render_surfels needs width and height")
    if distortion is not None:
        distortion = _distortion_range(distortion, "render_surfels")
        return_depth = True
    _refuse_surfel_camera_grad(camera_or_uniforms, "render_surfels")
    for name, t in (("means", means), ("scales", scales), ("rotations", rotations), ("opacities", opacities)):
        _cuda_f32(t, name)
    u = _uniforms(camera_or_uniforms, width, height)
    out = project_surfels(u, means, scales, rotations, return_depth=return_depth)  # (rec, [clip_w,] aux)
    rec, aux = out[0], out[-1]
    depths = out[1] if return_depth else None
    n = aux.n
    if sh is not None:
        k = sh.reshape(n, -1).shape[1] // 3
        deg = {1: 0, 4: 1, 9: 2, 16: 3}.get(k) if degree is None else degree
        if deg is None:
            raise SplatError(-1, f"sh must hold 3 (degree + 1)^2 floats per splat, not {3 * k}")
        col = sh_colors(u[16:19], means, sh, deg, opacities)
    elif colors is not None:
        _cuda_f32(colors, "colors", 3)
        col = _t().cat([colors, opacities.reshape(-1, 1)], dim=1)
    else:
        raise SplatError(-1, "render_surfels needs colors or sh")
    out = rasterize(rec, col, aux, width, height, depths=depths, features=features, distortion=distortion)
    out = (*out, aux) if return_aux else out
    return (*out, rec) if return_records else out


def sh_colors(eye, means, sh, degree, opacities):
    """(n, 4): rgb = max(0.5 + sum_k Y_k(normalize(p - eye)) sh_k, 0) and the opacity; sh (n, (degree + 1)^2, 3) or (n, 3K).
    An eye tensor (3 floats, float32 / float64, any device) that requires grad receives its gradient."""
    e_t = _grad_uniforms(eye, "eye", (3,))
    e = np.ascontiguousarray(np.asarray(eye.detach().cpu() if hasattr(eye, "detach") else eye, np.float32).reshape(-1)[:3])
    means4 = _cuda_f32(_vec4(means, "means", 1.0), "means", 4)
    n = means4.shape[0]
    if not 0 <= int(degree) <= 3:
        raise SplatError(-1, "degree must be 0-3")
    _cuda_f32(sh, "sh")
    sh2 = _cuda_f32(sh.reshape(n, -1) if n else sh.reshape(0, int(np.prod(sh.shape[1:]))), "sh")  # (no -1 for an empty tensor)
    if sh2.shape[1] < 3 * (int(degree) + 1) ** 2:
        raise SplatError(-1, f"sh holds {sh2.shape[1]} floats per splat; degree {degree} needs {3 * (int(degree) + 1) ** 2}")
    op = _cuda_f32(opacities.reshape(-1), "opacities")
    if op.shape[0] != n:
        raise SplatError(-1, "opacities must hold one value per splat")
    return _functions().ShColors.apply(e, means4, sh2, int(degree), op, e_t)


def _distortion_range(distortion, who):
    """(near, far) as floats, 0 < near < far (far = inf allowed), or SplatError."""
    try:
        near, far = (float(x) for x in distortion)
    except (TypeError, ValueError):
        raise SplatError(-1, f"{who}: distortion must be (near, far)") from None
    near, far = float(np.float32(near)), float(np.float32(far))
    if not (0.0 < near < far and near < float("inf")):
        raise SplatError(-1, f"{who}: distortion=(near, far) needs 0 < near < far, not ({near}, {far})")
    return near, far


def rasterize(rec, col, aux, width=None, height=None, depths=None, deterministic=False, absgrad=False, features=None, distortion=None):
    """(rgb (H, W, 3), alpha (H, W)) of the records and colours over the projection's lists; both differentiable.  With
    depths ((n,) per-splat z, differentiable): (rgb, alpha, depth), depth (H, W) = sum w z / sum w per pixel, +inf where
    nothing contributed.  deterministic=True: the backward sums in a fixed order (the module's docstring).  absgrad=True: the
    backward also leaves the (n, 2) absolute sums of the centre's terms in aux.absgrad (the module's docstring): the colour,
    alpha and depth terms only, never a feature map's.  features ((n, K) or (n,), 1 <= K <= 32): composite_features' map
    (H, W, K) is appended to the tuple, (rgb, alpha[, depth], feat), from the lists this call binned; not with deterministic=True
    (SplatError: no fixed-order feature backward exists).  distortion=(near, far), on a surfel projection with depths= only
    (SplatError otherwise, and unless 0 < near < far): (rgb, alpha, depth, dist[, feat]), dist (H, W) 2DGS's depth-distortion
    map of the intersection depths (the module's docstring), written by the depth map's own walk and differentiated by the one
    fused backward launch."""
    width = aux.width if width is None else int(width)
    height = aux.height if height is None else int(height)
    _refuse_deterministic_features(deterministic, features, "rasterize")
    if _is_surfel(aux) and (deterministic or absgrad):
        raise SplatError(-1, "rasterize: deterministic=True and absgrad=True are not built for surfels (their fixed-order and absolute "
                             "sums take q = 0 of every record)")
    rec_c = _cuda_f32(rec, "rec", 8)
    col_c = _cuda_f32(col, "col", 4)
    if rec_c.shape[0] != aux.n or col_c.shape[0] != aux.n:
        raise SplatError(-1, "rec, col and the projection must hold the same number of splats")
    z = None
    if depths is not None:
        z = _cuda_f32(depths, "depths")
        if z.dim() != 1 or z.shape[0] != aux.n:
            raise SplatError(-1, f"depths must have shape ({aux.n},), not {tuple(z.shape)}")
    if distortion is not None:
        if not _is_surfel(aux):
            raise SplatError(-1, "rasterize: distortion= is built for surfel projections only (project_surfels); an ellipsoid has one "
                                 "depth per splat: the (1, z, z^2) feature recipe of the module's docstring")
        if z is None:
            raise SplatError(-1, "rasterize: distortion= needs depths= (project_surfels(..., return_depth=True)'s clip_w)")
        distortion = _distortion_range(distortion, "rasterize")
    out = _functions().Rasterize.apply(rec_c, col_c, aux, width, height, z, bool(deterministic), bool(absgrad), distortion)
    if features is None:
        return out
    return (*out, composite_features(rec_c, col_c, aux, features, width, height))


def _refuse_deterministic_features(deterministic, features, who):
    if deterministic and features is not None:
        raise SplatError(-1, f"{who}: deterministic=True with features: no fixed-order feature backward exists (the feature gradients are "
                             "float atomic sums), and a reproducible and a non-reproducible sum are not mixed silently")


def composite_features(rec, col, aux, features, width=None, height=None):
    """(H, W, K) float32: per pixel F[k] = sum_i w_i features[i, k] over the entries the pixel consumed, with the weights
    w_i = T_i alpha_i of the frame rasterize(rec, col, aux, width, height) draws (the module's docstring;
    splat_composite_features).  No background, no division by sum w, 0 where nothing contributed.  Differentiable in rec, col
    (the opacity column only: its colour columns get exact zeros) and features.  features: (n, K) CUDA float32, 1 <= K <= 32, or
    (n,) for K = 1; a view whose last dimension has stride 1 and whose rows are at least K floats apart (features[:, a:b] of a
    wider tensor) is read where it lies, anything else is made contiguous.  The context's current lists are used when they are
    this projection's for this screen (after rasterize on the same aux: no second sort and bin); otherwise it bins."""
    torch = _t()
    width = aux.width if width is None else int(width)
    height = aux.height if height is None else int(height)
    rec_c = _cuda_f32(rec, "rec", 8)
    col_c = _cuda_f32(col, "col", 4)
    n = aux.n
    if rec_c.shape[0] != n or col_c.shape[0] != n:
        raise SplatError(-1, "rec, col and the projection must hold the same number of splats")
    f = features
    if not isinstance(f, torch.Tensor):
        raise SplatError(-1, "features must be a torch tensor")
    if not f.is_cuda:
        raise SplatError(-1, f"features is on {f.device}: splat_renderer_amd has no CPU path")
    if f.dtype != torch.float32:
        raise SplatError(-1, f"features must be float32, not {f.dtype}")
    if f.dim() == 1:
        f = f.reshape(-1, 1)
    if f.dim() != 2 or f.shape[0] != n or not 1 <= f.shape[1] <= MAX_FEATURE_CHANNELS:
        raise SplatError(-1, f"features must have shape ({n}, K) with 1 <= K <= {MAX_FEATURE_CHANNELS} (or ({n},)), not {tuple(features.shape)}")
    k = f.shape[1]
    if n > 1 and not ((k == 1 or f.stride(1) == 1) and f.stride(0) >= k):
        f = f.contiguous()
    elif n <= 1 and not f.is_contiguous():
        f = f.contiguous()
    return _functions().CompositeFeatures.apply(rec_c, col_c, aux, f, width, height)


def render_gaussians(camera_or_uniforms, means, scales, rotations, opacities, colors=None, sh=None, width=None, height=None, degree=None,
                     return_depth=False, deterministic=False, antialiased=False, absgrad=False, return_aux=False, features=None):
    """The whole differentiable frame: project_ellipsoids, the colour (sh_colors when `sh` is given, else cat(colors,
    opacities)), rasterize.  Returns (rgb (H, W, 3), alpha (H, W)); return_depth=True: (rgb, alpha, depth (H, W)), the depth
    map of the ProjectedSplat depths (the distance from the eye to each centre).  deterministic=True: every gradient is the
    same bits on every run (rasterize's fixed-order backward; the module's docstring).  antialiased=True: the opacity column is
    multiplied by project_ellipsoids' rho (a torch op) before rasterize: the 2D Mip filter.  absgrad=True: rasterize's
    absgrad; return_aux=True appends the frame's ProjectedSplats to the returned tuple, whose .absgrad backward() fills (the
    module's docstring).  features ((n, K) or (n,)): rasterize's features, the caller's tensor blended as it is (not
    compensated by rho: rho already sits in the opacity); the map comes after depth: (rgb, alpha[, depth], feat[, aux])."""
    if width is None or height is None:
        raise SplatError(-1, "render_gaussians needs width and height")
    _refuse_deterministic_features(deterministic, features, "render_gaussians")
    for name, t in (("means", means), ("scales", scales), ("rotations", rotations), ("opacities", opacities)):
        _cuda_f32(t, name)
    u = _uniforms(camera_or_uniforms, width, height)
    u_t = _grad_uniforms(camera_or_uniforms)
    pu = (camera_or_uniforms, means, scales, rotations, width, height) if u_t is not None else (u, means, scales, rotations)
    out = project_ellipsoids(*pu, return_depth=return_depth, antialiased=antialiased)  # (rec, [rho,] [depths,] aux)
    rec, aux = out[0], out[-1]
    rho = out[1] if antialiased else None
    depths = out[-2] if return_depth else None
    n = aux.n
    if sh is not None:
        k = sh.reshape(n, -1).shape[1] // 3
        deg = {1: 0, 4: 1, 9: 2, 16: 3}.get(k) if degree is None else degree
        if deg is None:
            raise SplatError(-1, f"sh must hold 3 (degree + 1)^2 floats per splat, not {3 * k}")
        col = sh_colors(u[16:19] if u_t is None else u_t.reshape(-1)[16:19], means, sh, deg, opacities)
    elif colors is not None:
        _cuda_f32(colors, "colors", 3)
        col = _t().cat([colors, opacities.reshape(-1, 1)], dim=1)
    else:
        raise SplatError(-1, "render_gaussians needs colors or sh")
    if rho is not None:
        col = compensate_opacity(col, rho)
    out = rasterize(rec, col, aux, width, height, depths=depths, deterministic=deterministic, absgrad=absgrad, features=features)
    return (*out, aux) if return_aux else out


def compensate_opacity(col, rho):
    """(n, 4) (r, g, b, opacity * rho): the antialiased mode's colour plane, in torch ops (one binary32 product per splat, as
    splat_project_ellipsoid_aa's color_opacity_out)."""
    return _t().cat([col[:, :3], col[:, 3:] * rho.reshape(-1, 1)], dim=1)


Contribution = collections.namedtuple("Contribution", ("hits", "weight_max", "weight_sum"))


def contribution(rec, col, aux, width=None, height=None, pixel_weight=None, min_weight=0.0, out=None):
    """Contribution(hits (n,) int32, weight_max (n,) float32, weight_sum (n,) int64 in units of 2^-24) of the frame
    rasterize(rec, col, aux, width, height) draws (the module's docstring; splat_composite_contribution).  pixel_weight: (H, W)
    CUDA float32 or None; out: an earlier Contribution to accumulate into (returned), else fresh zeros.  No gradient."""
    torch = _t()
    width = aux.width if width is None else int(width)
    height = aux.height if height is None else int(height)
    rec_c = _cuda_f32(rec.detach(), "rec", 8)
    col_c = _cuda_f32(col.detach(), "col", 4)
    n = aux.n
    if rec_c.shape[0] != n or col_c.shape[0] != n:
        raise SplatError(-1, "rec, col and the projection must hold the same number of splats")
    if not float(min_weight) >= 0.0:
        raise SplatError(-1, f"min_weight must be >= 0, not {min_weight}")
    pw = None
    if pixel_weight is not None:
        pw = _cuda_f32(pixel_weight.detach(), "pixel_weight")
        if tuple(pw.shape) != (height, width):
            raise SplatError(-1, f"pixel_weight must have shape ({height}, {width}), not {tuple(pw.shape)}")
    if out is None:
        out = Contribution(torch.zeros(n, device=rec_c.device, dtype=torch.int32), torch.zeros(n, device=rec_c.device, dtype=torch.float32),
                           torch.zeros(n, device=rec_c.device, dtype=torch.int64))
    else:
        out = Contribution(*out)
        for t, dt, name in zip(out, (torch.int32, torch.float32, torch.int64), Contribution._fields):
            if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dt or tuple(t.shape) != (n,) or not t.is_contiguous():
                raise SplatError(-1, f"out.{name} must be a contiguous CUDA {dt} tensor of shape ({n},)")
    if n:
        cx = aux.ctx
        cx.bin(aux, width, height)
        idx, cnt, off = cx.lists()
        cfg = _ellipsoid_cfg(aux.footprint)
        check(cx.lib.splat_composite_contribution(cx.ctx, C.byref(cfg), col_c.data_ptr(), 1, rec_c.data_ptr(), idx, cnt, off, width, height,
                                                  pw.data_ptr() if pw is not None else None, float(min_weight), n, out.hits.data_ptr(),
                                                  out.weight_max.data_ptr(), out.weight_sum.data_ptr()), cx.ctx)
    return out


def _image(t, name, channels):
    """(tensor, pixel stride in floats) of an (H, W, 3 | 4) CUDA float32 image, without a copy where its layout is one the
    kernels address: packed pixels of 3 floats, or of 4 (an (H, W, 4) tensor or its [..., :3] view)."""
    torch = _t()
    if not isinstance(t, torch.Tensor):
        raise SplatError(-1, f"{name} must be a torch tensor")
    if not t.is_cuda:
        raise SplatError(-1, f"{name} is on {t.device}: splat_renderer_amd has no CPU path")
    if t.dtype != torch.float32:
        raise SplatError(-1, f"{name} must be float32, not {t.dtype}")
    if t.dim() != 3 or t.shape[2] not in channels or t.shape[0] < 1 or t.shape[1] < 1:
        raise SplatError(-1, f"{name} must have shape (H, W, {' or '.join(map(str, channels))}), not {tuple(t.shape)}")
    h, w, c = t.shape
    for s in ((3, 4) if c == 3 else (4,)):
        if t.stride(2) == 1 and (w == 1 or t.stride(1) == s) and (h == 1 or t.stride(0) == w * s):
            return t, s
    return t.contiguous(), c


def photometric_loss(rgb, target, lambda_dssim=0.2, return_terms=False):
    """3DGS's objective (1 - lambda) L1 + lambda (1 - SSIM) between rgb (H, W, 3) and target (H, W, 3 or 4): a 0-d tensor,
    differentiable in rgb; return_terms=True: (loss, l1, ssim), the two terms detached.  The module's docstring has the rest."""
    x, xs = _image(rgb, "rgb", (3,))
    y, ys = _image(target, "target", (3, 4))
    if x.shape[:2] != y.shape[:2]:
        raise SplatError(-1, f"rgb is {tuple(x.shape[:2])} pixels and target {tuple(y.shape[:2])}")
    if x.device != y.device:
        raise SplatError(-1, f"rgb is on {x.device} and target on {y.device}")
    lam = float(lambda_dssim)
    loss, l1, ssim = _functions().PhotometricLoss.apply(x, xs, y.detach(), ys, lam, bool(return_terms))
    return (loss, l1, ssim) if return_terms else loss


def _ray_uniforms(camera_or_uniforms, width, height, who):
    """The host block of a camera whose rays a depth map's normals are taken along.  No camera gradient exists for them: a
    uniforms tensor that requires grad is refused rather than its gradient dropped silently."""
    if getattr(camera_or_uniforms, "requires_grad", False):
        raise SplatError(-1, f"{who}: the uniforms tensor requires grad, and the normals of a depth map offer no camera gradient; pass "
                             "uniforms.detach() to hold the camera fixed in this term")
    return _uniforms(camera_or_uniforms, width, height)


def _depth_kind(depth_kind, who):
    kinds = {"distance": _lib.DEPTH_DISTANCE, "z": _lib.DEPTH_Z}
    if depth_kind not in kinds:
        raise SplatError(-1, f"{who}: depth_kind must be 'distance' or 'z', not {depth_kind!r}")
    return kinds[depth_kind]


def _depth_map(depth, width, height, who):
    _cuda_f32(depth, "depth")
    if depth.dim() != 2 or depth.shape[0] < 1 or depth.shape[1] < 1:
        raise SplatError(-1, f"{who}: depth must have shape (H, W), not {tuple(depth.shape)}")
    h, w = depth.shape
    if (width is not None and int(width) != w) or (height is not None and int(height) != h):
        raise SplatError(-1, f"{who}: depth is {w} x {h} pixels, not width x height = {width} x {height}")
    return depth.contiguous(), w, h


def depth_normals(depth, camera_or_uniforms, width=None, height=None, depth_kind="distance"):
    """(H, W, 3): the unit normal of the surface the depth map (H, W) describes, facing the eye; 0 at the border, next to an empty
    (+inf) or non-positive depth (include/splat.h, "Normals of a depth map"; the module's docstring).  Differentiable in depth.
    depth_kind: "distance" (|P - eye|: what rasterize(depths=) and render_gaussians(return_depth=True) give) or "z" (clip w)."""
    d, w, h = _depth_map(depth, width, height, "depth_normals")
    u = _ray_uniforms(camera_or_uniforms, w, h, "depth_normals")
    return _functions().DepthNormals.apply(d, u, _depth_kind(depth_kind, "depth_normals"))


def normal_consistency_loss(normal_map, depth, camera_or_uniforms, weight=None, depth_kind="distance", width=None, height=None,
                            return_terms=False):
    """2DGS's normal consistency mean(1 - weight * normal_map . depth_normals(depth)): a 0-d tensor, differentiable in normal_map
    and depth, from one fused kernel forward and one backward.  normal_map (H, W, K >= 3): its first three channels are read
    where they lie, by the pixel stride, when the tensor (or view) is a packed image of K floats per pixel; weight (H, W) or
    None is detached.  return_terms=True: (loss, fraction of valid pixels), the second detached.  The module's docstring has
    the rest."""
    torch = _t()
    who = "normal_consistency_loss"
    d, w, h = _depth_map(depth, width, height, who)
    u = _ray_uniforms(camera_or_uniforms, w, h, who)
    f = normal_map
    if isinstance(f, torch.Tensor) and f.dim() == 3 and f.shape[2] > 4:
        # (_image's rule for K floats per pixel: read in place when the pixels are packed K apart)
        if not f.is_cuda:
            raise SplatError(-1, f"normal_map is on {f.device}: splat_renderer_amd has no CPU path")
        if f.dtype != torch.float32:
            raise SplatError(-1, f"normal_map must be float32, not {f.dtype}")
        k = f.shape[2]
        packed = f.stride(2) == 1 and (f.shape[1] == 1 or f.stride(1) == k) and (f.shape[0] == 1 or f.stride(0) == f.shape[1] * k)
        f, fs = (f, k) if packed else (f.contiguous(), k)
    else:
        f, fs = _image(f, "normal_map", (3, 4))
    if tuple(f.shape[:2]) != (h, w):
        raise SplatError(-1, f"normal_map is {tuple(f.shape[:2])} pixels and depth {(h, w)}")
    wt = None
    if weight is not None:
        wt = _cuda_f32(weight.detach(), "weight")
        if tuple(wt.shape) != (h, w):
            raise SplatError(-1, f"weight must have shape ({h}, {w}), not {tuple(wt.shape)}")
    if f.device != d.device or (wt is not None and wt.device != d.device):
        raise SplatError(-1, "normal_map, depth and weight must be on one device")
    loss, valid = _functions().NormalConsistency.apply(f, fs, d, wt, u, _depth_kind(depth_kind, who))
    return (loss, valid) if return_terms else loss


def splat_normals(means, scales, rotations, eye):
    """(n, 3): each splat's normal for a normal-consistency term, in torch ops (any device): the axis of its shortest scale, a
    column of R(q) of the normalised quaternion (w, x, y, z), flipped so that it faces the eye.  Differentiable in rotations
    (the choice of the axis and of the sign are held fixed); pass the result as render_gaussians' features."""
    torch = _t()
    q = rotations / rotations.norm(dim=1, keepdim=True)
    r, x, y, z = q.unbind(1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y),
                     2 * (x * y + r * z), 1 - 2 * (x * x + z * z), 2 * (y * z - r * x),
                     2 * (x * z - r * y), 2 * (y * z + r * x), 1 - 2 * (x * x + y * y)], dim=1).reshape(-1, 3, 3)
    axis = R.gather(2, scales[:, :3].argmin(dim=1).reshape(-1, 1, 1).expand(-1, 3, 1)).squeeze(2)  # (n, 3): column argmin of R
    eye = torch.as_tensor(eye, dtype=means.dtype, device=means.device).reshape(3)
    return torch.where(((means[:, :3] - eye) * axis).sum(dim=1, keepdim=True) > 0, -axis, axis)


def pinhole_uniforms(R, t, fx, fy, cx, cy, width, height, near=0.01, far=1000.0):
    """The 22-float uniform block of a pinhole camera, in plain torch ops (any device; float64 allowed), differentiable in R
    (3, 3), t (3,) and the intrinsics.  OpenCV / COLMAP convention: Xc = R X + t, x right, y down, z forward; a world point
    lands at pixel (fx Xc.x / Xc.z + cx, fy Xc.y / Xc.z + cy) in the projector's continuous screen coordinates (those of a
    record's c.x, c.y: (W / 2)(1 + c.x / c.w), (H / 2)(1 - c.y / c.w)), clip w = Xc.z, eye = -R^T t.  Row 2 of VP maps
    [near, far] to depth [0, 1] and is not read by the ellipsoid footprint.  R is used as given (not re-orthonormalised): how the
    pose is parametrised is the caller's choice.  fx, fy, cx, cy may be floats or 0-d tensors."""
    torch = _t()
    R = torch.as_tensor(R)
    kw = dict(dtype=R.dtype, device=R.device)
    t = torch.as_tensor(t, **kw).reshape(3)
    fx, fy, cx, cy = (torch.as_tensor(v, **kw).reshape(()) for v in (fx, fy, cx, cy))
    W, H = float(width), float(height)
    zero, one = torch.zeros((), **kw), torch.ones((), **kw)
    a, b = far / (far - near), -far * near / (far - near)
    P = torch.stack([torch.stack([2.0 * fx / W, zero, 2.0 * cx / W - 1.0, zero]),
                     torch.stack([zero, -2.0 * fy / H, 1.0 - 2.0 * cy / H, zero]),
                     torch.stack([zero, zero, a * one, b * one]),
                     torch.stack([zero, zero, one, zero])])
    V = torch.cat([torch.cat([R, t.reshape(3, 1)], dim=1), torch.stack([zero, zero, zero, one]).reshape(1, 4)], dim=0)
    VP = P @ V
    eye = -(R.transpose(0, 1) @ t)
    return torch.cat([VP.transpose(0, 1).reshape(16), eye, torch.zeros(1, **kw), torch.tensor([W, H], **kw)])


def knn_mean_sq_distance(points, return_evaluations=False):
    """Per point the mean of the squared distances to its three nearest neighbours (splat_knn_mean_sq; the module's docstring
    has the rest): points (n, 3) or (n, 4) CUDA float32 -> (n,) float32.  return_evaluations=True: (mean_sq, evaluations), the
    second a 0-d int64 tensor on the device with the number of distance evaluations the search performed."""
    torch = _t()
    if not isinstance(points, torch.Tensor) or points.dim() != 2 or points.shape[1] not in (3, 4):
        raise SplatError(-1, "points must be a tensor of shape (n, 3) or (n, 4)")
    pts = _cuda_f32(points.detach(), "points")
    n, stride = int(pts.shape[0]), int(pts.shape[1])
    out = torch.empty(n, device=pts.device, dtype=torch.float32)
    evals = torch.zeros((), device=pts.device, dtype=torch.int64) if return_evaluations else None
    if n:
        cx = _context(pts)
        cx.ensure_sorter(n)
        nbytes = int(cx.lib.splat_knn_workspace_bytes(n))
        ws = torch.empty((nbytes + 15) // 16 * 4, device=pts.device, dtype=torch.int32)
        check(cx.lib.splat_knn_mean_sq(cx.ctx, cx.sorter, pts.data_ptr(), stride, n, ws.data_ptr(), nbytes, out.data_ptr(),
                                       evals.data_ptr() if evals is not None else None), cx.ctx)
    return (out, evals) if return_evaluations else out
