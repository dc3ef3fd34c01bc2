"""From depth maps to a surface: a truncated signed distance volume on the GPU and the triangle mesh in it (include/splat.h,
"TSDF fusion and mesh extraction"; an extension, no reference counterpart).

    vol = TsdfVolume(origin, voxel, dims, trunc, color=True)                      # dims = (nx, ny, nz) nodes; all planes on the GPU
    for cam, target in views:
        rgb, alpha, depth = render_gaussians(cam, ..., return_depth=True)
        vol.integrate(depth, cam, image=rgb, weight=alpha)                        # in place: no copies of the frame's tensors
    vertices, triangles, colors = vol.extract_mesh()                              # (V, 3) float32, (T, 3) int32, (V, 3) float32: device tensors
    save_mesh_ply(path, vertices.cpu(), triangles.cpu(), colors.cpu())

integrate() is one launch of splat_tsdf_integrate on torch's current stream: per node one projection, one depth lookup and a
running weighted mean of min(1, (depth - the node's own depth) / trunc); nodes hidden behind the surface by more than trunc, or
seeing an empty (+inf), non-positive or NaN depth or a weight <= 0, are left alone.  depth is (H, W) float32, what
render_gaussians(return_depth=True) returns, with depth_kind "distance" (|X - eye|, that depth) or "z" (clip w); image (H, W, 3 or
4) is read by its pixel stride, so rasterize's view of its (H, W, 4) buffer is read where it lies; weight (H, W) weights the
observation (2DGS: the frame's alpha).  max_weight > 0 caps a node's weight, so that later views still move it.  The camera gets
no gradient and nothing here is differentiable: a uniforms tensor that requires grad is refused.

extract_mesh(min_weight) is marching tetrahedra on the Kuhn split over the cubes whose eight corners have weight > min_weight:
indexed (a shared vertex is stored once), ordered (vertices by node and edge, triangles by cube and tetrahedron), wound
counter-clockwise seen from outside, and the same bytes on every run.  It waits on the host once, for the two counts, between
splat_tsdf_mesh_count and splat_tsdf_mesh_emit; the workspace (10 bytes per node) is a torch tensor freed on return.

torch is imported when a volume is first made.
"""
import ctypes as C

import numpy as np

from . import _lib
from . import autograd as AG
from ._lib import SplatError, check


class TsdfVolume:
    def __init__(self, origin, voxel, dims, trunc, color=False, device="cuda"):
        torch = AG._t()
        dims = tuple(int(d) for d in dims)
        if len(dims) != 3 or min(dims) < 1 or max(dims) > _lib.TSDF_MAX_DIM or dims[0] * dims[1] * dims[2] > _lib.TSDF_MAX_NODES:
            raise SplatError(-1, f"TsdfVolume: dims must be three sizes of 1 to {_lib.TSDF_MAX_DIM} nodes with at most 2^30 nodes in all, not {dims}")
        origin = [float(x) for x in np.asarray(origin, np.float64).reshape(-1)]
        voxel, trunc = float(voxel), float(trunc)
        if len(origin) != 3 or not all(np.isfinite(origin)) or not (np.isfinite(voxel) and voxel > 0 and np.isfinite(trunc) and trunc > 0):
            raise SplatError(-1, "TsdfVolume: origin must be three finite numbers, voxel and trunc finite and > 0")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise SplatError(-1, f"TsdfVolume: device {self.device}: splat_renderer_amd has no CPU path")
        self.dims, self.voxel, self.trunc = dims, voxel, trunc
        self.grid = _lib.TsdfGrid((C.c_float * 3)(*origin), voxel, (C.c_uint32 * 3)(*dims), trunc)
        self.origin = tuple(self.grid.origin)
        n = dims[0] * dims[1] * dims[2]
        # (z, y, x) tensors: node (i, j, k) is element [k, j, i], linear index i + nx (j + ny k)
        self.tsdf = torch.zeros(dims[::-1], device=self.device, dtype=torch.float32)
        self.weight = torch.zeros(dims[::-1], device=self.device, dtype=torch.float32)
        self.color = torch.zeros((*dims[::-1], 3), device=self.device, dtype=torch.float32) if color else None
        self.n = n

    def reset(self):
        """An empty volume again (weight 0 everywhere; the other planes are zeroed too)."""
        self.weight.zero_()
        self.tsdf.zero_()
        if self.color is not None:
            self.color.zero_()

    def _map(self, t, name, h, w):
        torch = AG._t()
        if not isinstance(t, torch.Tensor):
            raise SplatError(-1, f"TsdfVolume.integrate: {name} must be a torch tensor")
        if not t.is_cuda or t.device != self.tsdf.device:
            raise SplatError(-1, f"TsdfVolume.integrate: {name} is on {t.device} and the volume on {self.tsdf.device}: splat_renderer_amd has no CPU path")
        if t.dtype != torch.float32:
            raise SplatError(-1, f"TsdfVolume.integrate: {name} must be float32, not {t.dtype}")
        if tuple(t.shape) != (h, w):
            raise SplatError(-1, f"TsdfVolume.integrate: {name} must have shape ({h}, {w}), not {tuple(t.shape)}")
        return t.detach().contiguous()

    def integrate(self, depth, camera_or_uniforms, image=None, weight=None, depth_kind="distance", max_weight=0.0):
        """Fuse one view (the module's docstring): depth (H, W), image (H, W, 3 | 4) or None, weight (H, W) or None, CUDA float32,
        read where they lie."""
        torch = AG._t()
        who = "TsdfVolume.integrate"
        if not isinstance(depth, torch.Tensor) or depth.dim() != 2 or depth.shape[0] < 1 or depth.shape[1] < 1:
            raise SplatError(-1, f"{who}: depth must be a torch tensor of shape (H, W), not {tuple(getattr(depth, 'shape', ()))}")
        h, w = depth.shape
        d = self._map(depth, "depth", h, w)
        u = AG._ray_uniforms(camera_or_uniforms, w, h, who)
        kind = AG._depth_kind(depth_kind, who)
        obs = self._map(weight, "weight", h, w) if weight is not None else None
        img, stride = None, 0
        if image is not None and self.color is not None:
            img, stride = AG._image(image.detach() if isinstance(image, torch.Tensor) else image, "image", (3, 4))
            if tuple(img.shape[:2]) != (h, w) or img.device != self.tsdf.device:
                raise SplatError(-1, f"{who}: image must be ({h}, {w}, 3 or 4) on {self.tsdf.device}, not {tuple(img.shape)} on {img.device}")
        max_weight = float(max_weight)
        if not (max_weight >= 0.0 and np.isfinite(max_weight)):
            raise SplatError(-1, f"{who}: max_weight must be finite and >= 0 (0: no cap), not {max_weight}")
        cx = AG._context(self.tsdf)
        check(cx.lib.splat_tsdf_integrate(cx.ctx, C.byref(self.grid), self.tsdf.data_ptr(), self.weight.data_ptr(),
                                          self.color.data_ptr() if self.color is not None else None, AG._fptr(u), kind, d.data_ptr(),
                                          obs.data_ptr() if obs is not None else None, img.data_ptr() if img is not None else None, stride, w, h,
                                          max_weight), cx.ctx)

    def extract_mesh(self, min_weight=0.0):
        """(vertices (V, 3) float32, triangles (T, 3) int32) on the device, and with a colour plane (..., colors (V, 3) float32);
        empty tensors when nothing crosses zero.  Cubes with a corner of weight <= min_weight are not meshed."""
        torch = AG._t()
        min_weight = float(min_weight)
        if not (min_weight >= 0.0 and np.isfinite(min_weight)):
            raise SplatError(-1, f"TsdfVolume.extract_mesh: min_weight must be finite and >= 0, not {min_weight}")
        cx = AG._context(self.tsdf)
        nbytes = int(cx.lib.splat_tsdf_mesh_workspace_bytes(*self.dims))
        ws = torch.empty(nbytes + 16, device=self.device, dtype=torch.uint8)
        wp = (ws.data_ptr() + 15) & ~15
        nv, nt = C.c_uint32(0), C.c_uint32(0)
        check(cx.lib.splat_tsdf_mesh_count(cx.ctx, C.byref(self.grid), self.tsdf.data_ptr(), self.weight.data_ptr(), min_weight, wp, nbytes,
                                           C.byref(nv), C.byref(nt)), cx.ctx)
        vertices = torch.empty((nv.value, 3), device=self.device, dtype=torch.float32)
        triangles = torch.empty((nt.value, 3), device=self.device, dtype=torch.int32)
        colors = torch.empty((nv.value, 3), device=self.device, dtype=torch.float32) if self.color is not None else None
        if nv.value:
            check(cx.lib.splat_tsdf_mesh_emit(cx.ctx, C.byref(self.grid), self.tsdf.data_ptr(), self.color.data_ptr() if colors is not None else None,
                                              wp, nbytes, vertices.data_ptr(), colors.data_ptr() if colors is not None else None,
                                              triangles.data_ptr()), cx.ctx)
        # (ws is freed by torch's caching allocator in stream order: the emit kernels above run before any later reuse on this stream)
        return (vertices, triangles, colors) if colors is not None else (vertices, triangles)
