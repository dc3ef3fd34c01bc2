"""GPU tests of the camera gradients of ellipsoid frames (splat_project_ellipsoid_backward_camera,
splat_sh_colors_backward_camera, the uniforms tensor of splat_renderer_amd.autograd and pinhole_uniforms) against the float64
restatement differentiated by torch.autograd (tests/ellipsoid_camera_grad_ref.py).

The bound is the per-splat gradients': relative L2 <= 1e-4, applied to the 12 entries of VP the frame reads as one vector and
to the eye as one vector (a single entry can cancel to nearly nothing).  Every test prints the figure it asserts on."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from tests import ellipsoid_camera_grad_ref as CR
from tests import ellipsoid_depth_grad_ref as DR
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER
from tests import test_gpu_ellipsoid_depth_grad as TD
from tests import test_gpu_ellipsoid_grad as TG

pytestmark = pytest.mark.gpu

BOUND = 1e-4
SENT = np.uint32(0x7FC0BEEF)  # a quiet NaN with a payload: no kernel arithmetic produces these bits
rel_l2 = CR.rel_l2
bits = TD.bits


def _f(a):
    return np.ascontiguousarray(a, np.float32)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _strided(a, stride):
    """(n, 4) rows stride float4s apart, NaN between them."""
    out = np.full((a.shape[0] * stride, 4), np.nan, np.float32)
    out[::stride] = a
    return out


def project_camera(d, u, pos, scl, rot, grec, gz, strides=(1, 1, 1), gu_offset=0):
    """(rc, gpos, gscl, grot, grad_uniforms (22,)) of splat_project_ellipsoid_backward_camera; grad_uniforms pre-filled with SENT."""
    n = pos.shape[0]
    up = _f(u)
    planes = [d.createBufferFrom(_strided(_f(a), max(s, 1)) if n else np.zeros((1, 4), np.float32)) for a, s in zip((pos, scl, rot), strides)]
    more = [d.createBufferFrom(_f(a) if a.size else np.zeros(4, np.float32)) for a in (grec, gz if gz is not None else np.zeros(1))]
    outs = [d.createBuffer(max(n, 1) * 16) for _ in range(3)]
    gu = d.createBufferFrom(np.full(32, SENT, np.uint32))
    rc = d.lib.splat_project_ellipsoid_backward_camera(d.ctx, _fp(up), planes[0].ptr, strides[0], planes[1].ptr, strides[1], planes[2].ptr,
                                                       strides[2], n, more[0].ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr,
                                                       more[1].ptr if gz is not None else None, gu.ptr + gu_offset)
    res = [o.read(np.float32, count=n * 4).reshape(n, 4) for o in outs] if rc == 0 else [None] * 3
    g = gu.read(np.float32, count=32) if rc == 0 else None
    for b in planes + more + outs + [gu]:
        b.destroy()
    return (rc, *res, g)


def project_plain(d, u, pos, scl, rot, grec, gz):
    n = pos.shape[0]
    bufs = [d.createBufferFrom(_f(a)) for a in (pos, scl, rot, grec, gz if gz is not None else np.zeros(1))]
    outs = [d.createBuffer(n * 16) for _ in range(3)]
    args = (d.ctx, _fp(_f(u)), bufs[0].ptr, 1, bufs[1].ptr, 1, bufs[2].ptr, 1, n, bufs[3].ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr)
    rc = d.lib.splat_project_ellipsoid_backward(*args) if gz is None else d.lib.splat_project_ellipsoid_backward_depth(*args, bufs[4].ptr)
    assert rc == 0
    res = [o.read(np.float32).reshape(n, 4) for o in outs]
    for b in bufs + outs:
        b.destroy()
    return res


def _check_block(got, want, eye_expected, label):
    """grad_uniforms (32 floats read, 22 written) against dL/du (22,) float64."""
    g = got[:22]
    assert np.isfinite(g).all(), label
    assert (bits(got[22:]) == SENT).all(), f"{label}: floats past the 22 written"
    assert (bits(g[CR.VP_ROW_2]) == 0).all() and (bits(g[19:22]) == 0).all(), f"{label}: row 2 / [19:22] not exact zeros"
    e_vp = rel_l2(g[CR.VP_ROWS_013], want[CR.VP_ROWS_013])
    print(f"{label}: VP relative L2 {e_vp:.3g}", end="")
    assert e_vp <= BOUND, f"{label}: VP relative L2 {e_vp:.3g}"
    if eye_expected:
        e_eye = rel_l2(g[16:19], want[16:19])
        print(f", eye relative L2 {e_eye:.3g}")
        assert e_eye <= BOUND, f"{label}: eye relative L2 {e_eye:.3g}"
        assert np.abs(g[16:19]).max() > 0
    else:
        print()
        assert (bits(g[16:19]) == 0).all(), f"{label}: eye not zero without grad_depth"


# splat_grad.hip sums up to CAM_DIRECT = 1024 per-wave partials (4 per 256 splats) with k_camera_sum alone and more through
# k_camera_sum_slices first: 70 001 splats give 1096 partials, slices of 18 in sixteenths of 2, ragged and empty tails
TWO_LEVEL = (70001, 333, 200, 12, 1.0, 0.02)
assert 4 * -(-TWO_LEVEL[0] // 256) > 1024 >= 4 * -(-max(c[0] for c in TG.CASES[:4]) // 256)


@pytest.mark.parametrize("n,w,h,seed,spread,scale", TG.CASES[:4] + [TWO_LEVEL])
def test_project_backward_camera(device, n, w, h, seed, spread, scale):
    pos, scl, rot, _ = ER.make_cloud(n, seed, spread, scale)
    u = TG.camera_u(w, h)
    rng = np.random.default_rng(seed)
    grec = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
    gz = rng.uniform(-1, 1, n).astype(np.float32)
    good = GR.sigma2_cond(u, pos, scl, rot) <= 1e4
    assert good.sum() > n // 3
    grec[~good] = 0
    gz[~good] = 0
    cull = GR.culled(u, pos, scl, rot)
    assert cull[[2, 3, 4, 5]].all()
    # culled splats must add exact zeros whatever their upstream: give them one (they are outside `good`, so restore it)
    grec[cull] = rng.uniform(-1, 1, (int(cull.sum()), 8)).astype(np.float32)
    gz[cull] = 1.0
    for depth in (True, False):
        label = f"project n={n} {'depth' if depth else 'colour'}"
        rc, gp, gs, gq, gu = project_camera(device, u, pos, scl, rot, grec, gz if depth else None)
        assert rc == 0
        want = CR.project_camera_grads(u, pos, scl, rot, ~cull, grec, gz if depth else None)
        _check_block(gu, want, depth, label)
        plain = project_plain(device, u, pos, scl, rot, grec, gz if depth else None)
        for name, a, b in zip(("gpos", "gscl", "grot"), (gp, gs, gq), plain):
            assert np.array_equal(bits(a), bits(b)), f"{label}: {name} differs from the entry point without the camera"
        again = project_camera(device, u, pos, scl, rot, grec, gz if depth else None)
        assert again[0] == 0 and np.array_equal(bits(again[4]), bits(gu)), f"{label}: two calls differ"
        # strides > 1: the same bits
        for ss in ((2, 3, 4), (3, 1, 2)):
            st = project_camera(device, u, pos, scl, rot, grec, gz if depth else None, strides=ss)
            assert st[0] == 0 and np.array_equal(bits(st[4]), bits(gu)), f"{label}: strides {ss}"
            assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(st[1:4], (gp, gs, gq))), f"{label}: strides {ss}"


def test_project_backward_camera_no_splats_and_all_culled(device):
    u = TG.camera_u(64, 64)
    e = np.zeros((0, 4), np.float32)
    for gz in (None, np.zeros(0, np.float32)):
        rc, _, _, _, gu = project_camera(device, u, e, e, e, np.zeros((0, 8), np.float32), gz)
        assert rc == 0 and (bits(gu[:22]) == 0).all() and (bits(gu[22:]) == SENT).all()
    # every splat behind the camera: zeros again, through the kernels
    n = 700
    pos, scl, rot, _ = ER.make_cloud(n, 3, 0.5, 0.05, degenerate=False)
    pos[:, :3] += 50.0 * (u[16:19] / np.linalg.norm(u[16:19]))
    assert GR.culled(u, pos, scl, rot).all()
    rc, gp, gs, gq, gu = project_camera(device, u, pos, scl, rot, np.ones((n, 8), np.float32), np.ones(n, np.float32))
    assert rc == 0 and (bits(gu[:22]) == 0).all() and (gp == 0).all() and (gs == 0).all() and (gq == 0).all()


def sh_camera(d, eye, pos, sh, degree, op, gcol, camera=True, ge_offset=0):
    n, nb = pos.shape[0], (degree + 1) ** 2
    stride = sh.size // n if n else 3 * nb  # (the floats per splat that `sh` holds; a degree that needs more is refused)
    bufs = [d.createBufferFrom(_f(a)) for a in (pos, sh.reshape(n, stride), op, gcol)]
    gsh, gp, gop = d.createBuffer(n * stride * 4), d.createBuffer(n * 16), d.createBuffer(n * 4)
    ge = d.createBufferFrom(np.full(8, SENT, np.uint32))
    args = (d.ctx, _fp(_f(eye)), bufs[0].ptr, 1, bufs[1].ptr, stride, degree, bufs[2].ptr, bufs[3].ptr, n, gsh.ptr, gp.ptr, gop.ptr)
    rc = d.lib.splat_sh_colors_backward_camera(*args, ge.ptr + ge_offset) if camera else d.lib.splat_sh_colors_backward(*args)
    out = (rc, gsh.read(np.float32), gp.read(np.float32), gop.read(np.float32), ge.read(np.float32, count=8))
    for b in bufs + [gsh, gp, gop, ge]:
        b.destroy()
    return out


@pytest.mark.parametrize("degree,n", [(0, 5000), (1, 5000), (2, 5000), (3, 5000), (1, TWO_LEVEL[0]), (3, TWO_LEVEL[0])])
def test_sh_backward_camera(device, degree, n):
    rng = np.random.default_rng(degree + 20)
    pos, _, _, _ = ER.make_cloud(n, degree + 20, degenerate=False)
    nb = (degree + 1) ** 2
    sh = rng.normal(0, 0.5, (n, nb, 3)).astype(np.float32)
    op = rng.uniform(0, 1, n).astype(np.float32)
    gcol = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    eye = TG.camera_u(64, 64)[16:19].astype(np.float32)
    rc, gsh, gp, gop, ge = sh_camera(device, eye, pos, sh, degree, op, gcol)
    assert rc == 0
    ref = sh_camera(device, eye, pos, sh, degree, op, gcol, camera=False)
    for name, a, b in zip(("grad_sh", "grad_positions", "grad_opacity"), (gsh, gp, gop), ref[1:4]):
        assert np.array_equal(bits(a), bits(b)), f"{name} differs from splat_sh_colors_backward's"
    again = sh_camera(device, eye, pos, sh, degree, op, gcol)
    assert np.array_equal(bits(again[4]), bits(ge))
    assert (bits(ge[3:4]) == 0).all() and (bits(ge[4:]) == SENT).all()
    if degree == 0:  # (the constant basis function has no direction: exact zeros)
        assert (bits(ge[:3]) & 0x7FFFFFFF == 0).all()
        return
    passed = ER.sh_colors(eye, pos, sh, degree, op, dtype=np.float32)[:, :3] > 0
    E = torch.tensor(eye.astype(np.float64), requires_grad=True)
    out = CR.sh_colors64(E, torch.as_tensor(pos.astype(np.float64)), torch.as_tensor(sh.astype(np.float64)), degree,
                         torch.as_tensor(op.astype(np.float64)), passed)
    (out * torch.as_tensor(gcol.astype(np.float64))).sum().backward()
    e = rel_l2(ge[:3], E.grad.numpy())
    print(f"sh degree {degree} n={n}: eye relative L2 {e:.3g}")
    assert e <= BOUND, f"eye relative L2 {e:.3g}"
    # n = 0 writes the zeros
    z = np.zeros((0, 4), np.float32)
    rc, _, _, _, ge0 = sh_camera(device, eye, z, np.zeros((0, nb, 3), np.float32), degree, np.zeros(0, np.float32), z)
    assert rc == 0 and (bits(ge0[:4]) == 0).all() and (bits(ge0[4:]) == SENT).all()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _reference_chain_camera(u, pos, scl, rot, op, sh, degree, w, h, g, gd):
    """TD._reference_chain_depth extended to the camera: dL/du (22,) float64."""
    U = CR.utensor(u)
    P, S, Q, OP, SH = (torch.as_tensor(a.astype(np.float64)) for a in (pos, scl, rot, op, sh))
    _reference_chain_camera_loss(u, U, P, S, Q, OP, SH, degree, w, h, g, gd).backward()
    return U.grad.numpy()


def _reference_chain_camera_loss(u, U, P, S, Q, OP, SH, degree, w, h, g, gd):
    """The float64 chain's loss as a function of the block U (a (22,) float64 tensor, a leaf or the result of a graph) and of
    the splats' float64 tensors, any of which may require grad; every decision comes from the binary32 pass under the binary32
    block u."""
    pos, scl, rot, op, sh = (a.detach().numpy().astype(np.float32) for a in (P, S, Q, OP, SH))
    rec32, counts, offsets, idx = TG.lists(u, pos, scl, rot, w, h)
    col32 = ER.sh_colors(u[16:19], pos, sh, degree, op, dtype=np.float32).astype(np.float32)
    dec = GR.decisions(rec32, col32, idx, counts, offsets, w, h)
    passed = col32[:, :3] > 0
    rec = CR.records64(U, GR._v(P, 4, 1.0), GR._v(S), Q, ~GR.culled(u, pos, scl, rot))
    col = CR.sh_colors64(U[16:19], P, SH, degree, OP, passed)
    z = CR.depth64(U, P)
    rgb, alpha, _zw, ws, D = DR.composite_depth64(rec, col, z, dec["steps"], w, h)
    gt = torch.as_tensor(g.astype(np.float64).reshape(-1, 4))
    gdt = torch.as_tensor(gd.astype(np.float64).reshape(-1))
    some = ws > 0
    Dz = torch.where(some, D, torch.zeros_like(D))
    return (rgb * gt[:, :3]).sum() + (alpha * gt[:, 3]).sum() + (Dz * torch.where(some, gdt, torch.zeros_like(gdt))).sum()


@pytest.mark.parametrize("where,dtype", [("cuda", torch.float32), ("cpu", torch.float64)])
def test_render_gaussians_camera_gradient(device, where, dtype):
    n, w, h, seed, degree = 3000, 160, 120, 7, 1
    pos, scl, rot, col, sh, op = TD._scene_with_sh(n, w, h, seed, degree)
    u = TG.camera_u(w, h)
    # ill-conditioned splats are left out by making them transparent on both sides (a row mask cannot be applied to a sum)
    good = GR.sigma2_cond(u, pos, scl, rot) <= 1e4
    kept = good | GR.culled(u, pos, scl, rot)
    assert kept.sum() > n // 3 and good.sum() > n // 3
    op = np.where(kept, op, 0).astype(np.float32)
    col = col.copy()
    col[:, 3] = op
    g, gd = TD._upstreams(u, pos, scl, rot, col, w, h, seed)
    want = _reference_chain_camera(u, pos, scl, rot, op, sh, degree, w, h, g, gd)
    leaves = dict(means=TD._leaf(pos), scales=TD._leaf(scl), rotations=TD._leaf(rot), opacities=TD._leaf(op), sh=TD._leaf(sh))
    ut = torch.tensor(u, dtype=dtype, device=where, requires_grad=True)
    TD._torch_loss(ut, leaves, w, h, g, gd, degree).backward()
    assert ut.grad is not None and ut.grad.shape == ut.shape and ut.grad.dtype == dtype and ut.grad.device == ut.device
    got = ut.grad.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all()
    assert (got[CR.VP_ROW_2] == 0).all() and (got[19:22] == 0).all()
    e_vp, e_eye = rel_l2(got[CR.VP_ROWS_013], want[CR.VP_ROWS_013]), rel_l2(got[16:19], want[16:19])
    print(f"end to end ({where}): VP relative L2 {e_vp:.3g}, eye relative L2 {e_eye:.3g}")
    assert e_vp <= BOUND, f"VP relative L2 {e_vp:.3g}"
    assert e_eye <= BOUND, f"eye relative L2 {e_eye:.3g}"
    # the other leaves: those of the same call with the camera as a NumPy block
    ref = dict(means=TD._leaf(pos), scales=TD._leaf(scl), rotations=TD._leaf(rot), opacities=TD._leaf(op), sh=TD._leaf(sh))
    TD._torch_loss(u, ref, w, h, g, gd, degree).backward()
    # (every leaf is downstream of the composite's float atomic sums, whose order of arrival varies between the two runs: the
    # existing end-to-end bound; the deterministic kernels are compared bit for bit in the staged test below)
    for name in ("means", "scales", "rotations", "opacities", "sh"):
        a, b = leaves[name].grad.cpu().numpy(), ref[name].grad.cpu().numpy()
        rows = good if name in ("means", "scales", "rotations") else np.ones(n, bool)
        e = rel_l2(a[rows].reshape(-1), b[rows].astype(np.float64).reshape(-1))
        assert e <= 1e-4, f"{name}: relative L2 {e:.3g} between the tensor and the NumPy camera"


def test_staged_functions_carry_the_camera_and_match_the_kernels_bit_for_bit(device):
    """project_ellipsoids(..., return_depth=True) and sh_colors(eye=tensor) with a given upstream: deterministic kernels, so the
    leaves' gradients are those of the constant-camera call bit for bit, and two backwards give the same camera gradient."""
    from splat_renderer_amd import autograd as AG
    n, w, h, degree = 3000, 160, 120, 2
    pos, scl, rot, col, sh = TG._torch_scene(n, w, h, 7, degree=degree)
    u = TG.camera_u(w, h)
    rng = np.random.default_rng(1)
    grec = torch.as_tensor(rng.uniform(-1, 1, (n, 8)).astype(np.float32), device="cuda")
    gz = torch.as_tensor(rng.uniform(-1, 1, n).astype(np.float32), device="cuda")
    gcol = torch.as_tensor(rng.uniform(-1, 1, (n, 4)).astype(np.float32), device="cuda")

    def run(camera):
        leaves = [TD._leaf(a) for a in (pos, scl, rot, col[:, 3], sh)]
        rec, depths, _aux = AG.project_ellipsoids(camera, leaves[0], leaves[1], leaves[2], return_depth=True)
        eye = camera[16:19]
        c = AG.sh_colors(eye, leaves[0], leaves[4], degree, leaves[3])
        ((rec * grec).sum() + (depths * gz).sum() + (c * gcol).sum()).backward()
        return [leaf.grad.cpu().numpy() for leaf in leaves]
    const = run(u)
    cams = [torch.tensor(u, device="cuda", requires_grad=True) for _ in range(2)]
    got = [run(c) for c in cams]
    for a, b in zip(got[0], const):
        assert np.array_equal(bits(a), bits(b))
    assert cams[0].grad is not None and np.array_equal(bits(cams[0].grad.cpu().numpy()), bits(cams[1].grad.cpu().numpy()))
    # rec alone (no depth gradient): the eye receives the SH term only; the frame's VP part is unchanged by it
    cam = torch.tensor(u, device="cuda", requires_grad=True)
    rec, _aux = AG.project_ellipsoids(cam, TD._leaf(pos), TD._leaf(scl), TD._leaf(rot))
    (rec * grec).sum().backward()
    assert (cam.grad[16:] == 0).all() and float(cam.grad[:16].abs().max()) > 0


# ---- a pose fit ----------------------------------------------------------------------------------------------------------------
def _skew(v):
    z = torch.zeros((), dtype=v.dtype, device=v.device)
    return torch.stack([torch.stack([z, -v[2], v[1]]), torch.stack([v[2], z, -v[0]]), torch.stack([-v[1], v[0], z])])


def _angle(Ra, Rb):
    c = (torch.trace(Ra @ Rb.transpose(0, 1)) - 1) / 2
    return float(torch.acos(c.clamp(-1, 1)))


FIT_STEPS, FIT_LR_ROT, FIT_LR_T = 200, 1e-3, 2e-3


def pose_fit(steps=FIT_STEPS, lr_rot=FIT_LR_ROT, lr_t=FIT_LR_T):
    """A fixed cloud, a target rendered from a pinhole pose, the start that pose turned by 1 degree and moved by 1 % of the
    scene's depth; Adam on an axis-angle increment and t.  Returns (losses, (angle, distance) at the start, at the end, seconds)."""
    from splat_renderer_amd import autograd as AG
    n, w, h = 2000, 256, 256
    pos, scl, rot, col = ER.make_cloud(n, 31, 1.0, 0.04, degenerate=False)
    t32 = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")  # noqa: E731
    P, S, Q, OP, CL = t32(pos[:, :3]), t32(scl[:, :3]), t32(rot), t32(col[:, 3]), t32(col[:, :3])
    D = torch.float64
    depth = 3.0
    R_gt = torch.linalg.matrix_exp(_skew(torch.tensor([0.4, 0.5, 0.1], dtype=D)))
    t_gt = torch.tensor([0.05, -0.1, depth], dtype=D)
    f = 0.5 * w / np.tan(np.radians(22.5))

    def frame(R, t):
        u = AG.pinhole_uniforms(R, t, f, f, w / 2, h / 2, w, h)
        rgb, _ = AG.render_gaussians(u, P, S, Q, OP, colors=CL, width=w, height=h)
        return rgb
    with torch.no_grad():
        target = frame(R_gt, t_gt).clone()
    axis = torch.tensor([1.0, -2.0, 1.5], dtype=D)
    R0 = torch.linalg.matrix_exp(_skew(axis / axis.norm() * np.radians(1.0))) @ R_gt
    d = torch.tensor([2.0, 1.0, -2.0], dtype=D)
    t0 = t_gt + d / d.norm() * (0.01 * depth)
    wv = torch.zeros(3, dtype=D, requires_grad=True)
    t = t0.clone().requires_grad_()
    opt = torch.optim.Adam([{"params": [wv], "lr": lr_rot}, {"params": [t], "lr": lr_t}])
    start = (_angle(R0, R_gt), float((t0 - t_gt).norm()))
    losses = []
    t_begin = time.time()
    for _ in range(steps):
        opt.zero_grad()
        loss = ((frame(torch.linalg.matrix_exp(_skew(wv)) @ R0, t) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    with torch.no_grad():
        R_end = torch.linalg.matrix_exp(_skew(wv)) @ R0
        losses.append(float(((frame(R_end, t) - target) ** 2).mean()))
        end = (_angle(R_end, R_gt), float((t.detach() - t_gt).norm()))
    return losses, start, end, time.time() - t_begin


def test_pose_fit_converges(device):
    losses, start, end, elapsed = pose_fit()
    print(f"pose fit: loss {losses[0]:.4g} -> {losses[-1]:.4g} ({losses[0] / losses[-1]:.1f}x), rotation {np.degrees(start[0]):.3f} -> "
          f"{np.degrees(end[0]):.3f} deg, translation {start[1]:.4f} -> {end[1]:.4f} in {elapsed:.1f} s")
    assert all(np.isfinite(losses))
    assert losses[-1] <= losses[0] / 10
    assert end[0] < 0.5 * start[0] and end[1] < 0.5 * start[1]


# ---- rejections ----------------------------------------------------------------------------------------------------------------
def test_camera_rejections(device):
    n, w, h = 500, 64, 64
    pos, scl, rot, col = ER.make_cloud(n, 3, 0.5, 0.05)
    u = TG.camera_u(w, h)
    grec, gz = np.zeros((n, 8), np.float32), np.zeros(n, np.float32)
    d = device
    assert project_camera(d, u, pos, scl, rot, grec, gz, gu_offset=4)[0] == -1       # misaligned grad_uniforms
    assert project_camera(d, u, pos, scl, rot, grec, gz, strides=(0, 1, 1))[0] == -1  # stride 0
    bufs = [d.createBufferFrom(_f(a)) for a in (pos, scl, rot, grec, gz)]
    out = d.createBuffer(n * 16 + 128)
    head = (d.ctx, _fp(_f(u)), bufs[0].ptr, 1, bufs[1].ptr, 1, bufs[2].ptr, 1, n, bufs[3].ptr)
    fn = d.lib.splat_project_ellipsoid_backward_camera
    assert fn(*head, out.ptr, out.ptr, out.ptr, bufs[4].ptr, None) == -1              # NULL grad_uniforms
    assert fn(*head, out.ptr, out.ptr, out.ptr, bufs[4].ptr + 2, out.ptr) == -1       # misaligned grad_depth
    assert fn(*head, out.ptr + 4, out.ptr, out.ptr, bufs[4].ptr, out.ptr) == -1       # misaligned grad_positions
    assert fn(d.ctx, None, *head[2:], out.ptr, out.ptr, out.ptr, bufs[4].ptr, out.ptr) == -1  # NULL uniforms
    assert fn(d.ctx, head[1], None, *head[3:], out.ptr, out.ptr, out.ptr, bufs[4].ptr, out.ptr) == -1  # NULL positions, n > 0
    for b in bufs + [out]:
        b.destroy()
    eye = u[16:19]
    sh = np.zeros((n, 4, 3), np.float32)
    assert sh_camera(d, eye, pos, sh, 1, col[:, 3], col, ge_offset=4)[0] == -1        # misaligned grad_eye
    assert sh_camera(d, eye, pos, sh, 4, col[:, 3], col)[0] == -1                      # degree 4
    bufs = [d.createBufferFrom(_f(a)) for a in (pos, sh.reshape(n, -1), col)]
    out = d.createBuffer(n * 48)
    assert d.lib.splat_sh_colors_backward_camera(d.ctx, _fp(_f(eye)), bufs[0].ptr, 1, bufs[1].ptr, 12, 1, None, bufs[2].ptr, n, out.ptr, out.ptr,
                                                 out.ptr, None) == -1                  # NULL grad_eye
    for b in bufs + [out]:
        b.destroy()


def test_a_uniforms_tensor_of_the_wrong_length_or_dtype_is_refused(device):
    from splat_renderer_amd import autograd as AG
    n, w, h = 50, 64, 64
    pos, scl, rot, col, _ = TG._torch_scene(n, w, h, 3)
    args = [TD._leaf(a) for a in (pos, scl, rot, col[:, 3])]
    for bad in (torch.zeros(21, device="cuda", requires_grad=True), torch.zeros(16, requires_grad=True),
                torch.zeros(22, dtype=torch.float16, device="cuda", requires_grad=True),
                torch.zeros(23, dtype=torch.float64, requires_grad=True)):
        with pytest.raises(sr.SplatError):
            AG.render_gaussians(bad, *args, colors=TD._leaf(col[:, :3]), width=w, height=h)
    with pytest.raises(sr.SplatError):
        AG.sh_colors(torch.zeros(4, requires_grad=True), args[0], TD._leaf(np.zeros((n, 3), np.float32)), 0, args[3])
    # 20 floats with width and height: accepted, and the gradient has the tensor's 20
    u20 = torch.tensor(TG.camera_u(w, h)[:20], device="cuda", requires_grad=True)
    rgb, _ = AG.render_gaussians(u20, *args, colors=TD._leaf(col[:, :3]), width=w, height=h)
    rgb.sum().backward()
    assert u20.grad.shape == (20,) and float(u20.grad[:16].abs().max()) > 0
