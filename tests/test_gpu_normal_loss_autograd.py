"""GPU tests of the geometry term in splat_renderer_amd.autograd: depth_normals, normal_consistency_loss and splat_normals on a
frame of flat splats lying on a tilted plane, through render_gaussians(return_depth=True, features=splat_normals(...)).  The
bounds are tests/test_gpu_depth_normals.py's (K_N, K_G over the per-pixel bounds of tests/depth_normals_ref.py)."""
import numpy as np
import pytest
import torch

from splat_renderer_amd import autograd as AG
from tests import cameras
from tests import depth_normals_ref as DR
from tests.test_depth_normals_cpu import splat_normals_ref
from tests.test_gpu_depth_normals import K_G, K_N, cuda, host, ratio

pytestmark = pytest.mark.gpu

W, H, N_SPLATS = 48, 40, 300
EYE = (0.3, 0.2, -3.0)
LAMBDA = 0.05


def camera():
    R, t = cameras.look_at(EYE, (0.0, 0.0, 0.0), roll=0.1)
    return AG.pinhole_uniforms(torch.as_tensor(R), torch.as_tensor(t), 55.0, 60.0, 0.48 * W, 0.53 * H, W, H).numpy().astype(np.float32)


def plane_splats(grad=True, seed=0):
    """About 300 flat splats on the plane through the origin with normal ~ (0.2, 0.3, -1): their shortest axis is the normal."""
    rng = np.random.default_rng(seed)
    nrm = np.array([0.2, 0.3, -1.0]) / np.linalg.norm([0.2, 0.3, -1.0])
    e1 = np.cross(nrm, [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(nrm, e1)
    ab = rng.uniform(-1.0, 1.0, (N_SPLATS, 2))
    means = ab[:, :1] * e1 + ab[:, 1:] * e2 + 0.01 * rng.standard_normal((N_SPLATS, 1)) * nrm
    scales = np.stack([rng.uniform(0.15, 0.3, N_SPLATS), rng.uniform(0.15, 0.3, N_SPLATS), rng.uniform(0.005, 0.02, N_SPLATS)], axis=1)
    # quaternion (w, x, y, z) turning z onto the normal, then a spin about z, then a small wobble
    axis = np.cross([0.0, 0.0, 1.0], nrm)
    ang = np.arccos(nrm[2])
    axis = axis / np.linalg.norm(axis)
    q0 = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * axis])
    spin = rng.uniform(0, 2 * np.pi, N_SPLATS)
    qs = np.stack([np.cos(spin / 2), 0 * spin, 0 * spin, np.sin(spin / 2)], axis=1)

    def mul(a, b):
        aw, ax, ay, az = a.T
        bw, bx, by, bz = b.T
        return np.stack([aw * bw - ax * bx - ay * by - az * bz, aw * bx + ax * bw + ay * bz - az * by,
                         aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw], axis=1)
    rot = mul(np.broadcast_to(q0, (N_SPLATS, 4)), qs) + 0.03 * rng.standard_normal((N_SPLATS, 4))
    leaves = dict(means=means, scales=scales, rotations=rot * 1.3, opacities=rng.uniform(0.4, 0.9, N_SPLATS), colors=rng.random((N_SPLATS, 3)))
    return {k: torch.tensor(np.ascontiguousarray(v, np.float32), device="cuda", requires_grad=grad) for k, v in leaves.items()}


def frame(p, u, **kw):
    feats = AG.splat_normals(p["means"], p["scales"], p["rotations"], EYE)
    return AG.render_gaussians(u, p["means"], p["scales"], p["rotations"], p["opacities"], colors=p["colors"], width=W, height=H,
                               return_depth=True, features=feats, **kw)


def test_fused_loss_is_the_torch_term_and_reaches_the_splats(device):
    u = camera()
    p = plane_splats()
    rgb, alpha, depth, nmap = frame(p, u)
    depth.retain_grad()
    nmap.retain_grad()
    wt = alpha.detach()
    fused = AG.normal_consistency_loss(nmap, depth, u, weight=wt)
    (LAMBDA * fused).backward()
    g_depth, g_nmap = host(depth.grad), host(nmap.grad)
    splat_grads = {k: host(p[k].grad) for k in ("means", "scales", "rotations", "opacities")}
    for k, g in splat_grads.items():
        assert np.isfinite(g).all() and np.abs(g).max() > 0, k
    # the same term in torch ops over depth_normals, on the same tensors
    d2, n2 = depth.detach().clone().requires_grad_(True), nmap.detach().clone().requires_grad_(True)
    chain = (1.0 - wt * (n2 * AG.depth_normals(d2, u)).sum(dim=2)).mean()
    (LAMBDA * chain).backward()
    # both against float64, within the kernels' bounds
    z64, F64, w64 = host(depth).astype(np.float64), host(nmap).astype(np.float64), host(wt).astype(np.float64)
    L, frac, term_bound, r = DR.loss(F64, z64, u, w64)
    assert 0.3 < frac < 1.0, "the plane should cover most of the screen and leave some of it empty"
    assert L < 0.9, "blended normals of splats lying on the plane agree with the plane's normal where it is covered"
    gF, gF_bound, gz, gz_bound = DR.loss_backward(r, F64, w64, LAMBDA)
    tol = K_N * DR.EPS * term_bound.mean() + 4 * DR.EPS * abs(L)
    assert abs(float(fused.detach()) - L) <= tol and abs(float(chain.detach()) - L) <= tol + 4 * DR.EPS  # (the chain's mean is a float32 sum)
    for name, gd, gn in (("fused", g_depth, g_nmap), ("torch ops over depth_normals", host(d2.grad), host(n2.grad))):
        rz, rf = ratio(np.abs(gd - gz), gz_bound), ratio(np.linalg.norm(gn - gF, axis=2), gF_bound)
        print(f"{name}: |error| / (2^-24 bound): dL/ddepth {rz:.3f}, dL/dnmap {rf:.3f}")
        assert rz <= K_G and rf <= K_N, name
    # a wider feature map is read in place, and its other channels get zero gradient
    wide = torch.cat([nmap.detach(), torch.full((H, W, 3), float("nan"), device="cuda")], dim=2).requires_grad_(True)
    d3 = depth.detach().clone().requires_grad_(True)
    (LAMBDA * AG.normal_consistency_loss(wide, d3, u, weight=wt)).backward()
    assert np.array_equal(host(wide.grad)[..., :3], g_nmap) and (host(wide.grad)[..., 3:] == 0).all()
    assert np.array_equal(host(d3.grad), g_depth)
    loss2, valid = AG.normal_consistency_loss(nmap.detach(), depth.detach(), u, weight=wt, return_terms=True)
    assert float(loss2) == float(fused.detach()) and abs(float(valid) - frac) <= 1e-6 and not valid.requires_grad


def test_splat_normals_matches_float64(device):
    p = plane_splats(grad=False, seed=3)
    got = host(AG.splat_normals(p["means"], p["scales"], p["rotations"], EYE))
    want = splat_normals_ref(host(p["means"]), host(p["scales"]), host(p["rotations"]), np.array(EYE))
    assert np.abs(got - want).max() <= 8 * DR.EPS
    nrm = np.array([0.2, 0.3, -1.0]) / np.linalg.norm([0.2, 0.3, -1.0])
    assert (got @ nrm > 0.9).all()  # the flat axis, turned towards the eye (which looks along +z at a plane facing -z)


def test_camera_that_requires_grad_is_refused(device):
    u = torch.tensor(camera(), requires_grad=True)
    z = cuda(np.ones((H, W)))
    with pytest.raises(AG.SplatError, match="requires grad"):
        AG.depth_normals(z, u)
    with pytest.raises(AG.SplatError, match="requires grad"):
        AG.normal_consistency_loss(cuda(np.ones((H, W, 3))), z, u)
    assert AG.depth_normals(z, u.detach()).shape == (H, W, 3)


def test_deterministic_chain_gives_the_same_grad_bytes(device):
    u = camera()
    target = cuda(np.random.default_rng(8).standard_normal((H, W, 3)))
    grads = []
    for _ in range(2):
        p = plane_splats()
        rec, depths, aux = AG.project_ellipsoids(u, p["means"], p["scales"], p["rotations"], return_depth=True)
        col = torch.cat([p["colors"], p["opacities"].reshape(-1, 1)], dim=1)
        rgb, alpha, depth = AG.rasterize(rec, col, aux, W, H, depths=depths, deterministic=True)
        ((AG.depth_normals(depth, u) - target) ** 2).mean().backward()
        grads.append({k: host(p[k].grad).copy() for k in ("means", "scales", "rotations", "opacities")})
    for k in grads[0]:
        assert np.abs(grads[0][k]).max() > 0 and np.array_equal(grads[0][k].view(np.uint32), grads[1][k].view(np.uint32)), k
