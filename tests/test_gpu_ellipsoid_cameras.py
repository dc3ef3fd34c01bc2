"""GPU tests of the 3D Gaussian (ellipsoid) kernels under more than one camera (tests/cameras.py): the projector, whole frames, the
SH colours, the projector's backward with and without depth, the camera gradients and the autograd chain, each held to the
reference the default-camera tests hold it to and with their bounds, through their drivers (test_gpu_ellipsoid*.py).

The default orbit's VP has m[4] = m[12] = 0 and m[13] ~ 0, so every term those entries multiply is silent under it; the camera
gradient is also compared entry by entry here (|got - want| <= 1e-4 max|want over the 12|), which one relative L2 over the 12
cannot see.  The conditions that keep these tests from passing on nothing (pixels skipped, rows kept, splats on screen) are
asserted from the references alone in tests/test_ellipsoid_cameras_cpu.py.  Last, the splat at the eye: |p - eye| = 0 has no
direction, and splat_sh_colors and its backward give it (0, 0, 0) instead of 0 * inf.  Every test prints the figures it asserts on."""
import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from tests import cameras as CAMS
from tests import ellipsoid_camera_grad_ref as CR
from tests import ellipsoid_depth_grad_ref as DR
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER
from tests import test_gpu_ellipsoid as TE
from tests import test_gpu_ellipsoid_camera_grad as TC
from tests import test_gpu_ellipsoid_depth_grad as TD
from tests import test_gpu_ellipsoid_grad as TG
from tests.test_ellipsoid_cameras_cpu import ROW_SCENES, SCENES

pytestmark = pytest.mark.gpu

BOUND = TC.BOUND  # 1e-4: relative L2 of a gradient, and the per-entry bound relative to the largest of the 12 entries
rel_l2 = CR.rel_l2
bits = TD.bits
CLOUDS = [SCENES["frames"], ROW_SCENES["large"]]  # (n, w, h, seed, spread, scale, degenerate): 3000 and 20 000 splats
CHAIN_CAMERAS = ("pinhole_rolled_offaxis", "pinhole_inside", "pinhole_subpixel", "general_vp", "pinhole_at_origin", "orbit_off_target")


def _cloud(case):
    n, w, h, seed, spread, scale, degenerate = case
    return (n, w, h) + ER.make_cloud(n, seed, spread, scale, degenerate)


# ---- the projector -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CLOUDS, ids=lambda c: f"n{c[0]}")
@pytest.mark.parametrize("name", CAMS.NAMES)
def test_projector_bit_exact(device, name, case):
    n, w, h, pos, scl, rot, col = _cloud(case)
    u = CAMS.camera(name, w, h)
    rec = TE.projector_bit_exact(device, u, pos, scl, rot, col)
    cull = GR.culled(u, pos, scl, rot)
    assert np.array_equal(cull, (rec == 0).all(axis=1)) and (~cull).sum() >= n / 3
    print(f"{name} n={n}: records, ProjectedSplats, keys and payload bit-exact; {int((~cull).sum())} live, {int(cull.sum())} culled")


# ---- whole frames --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,tile", [("default", 16), ("sortFirst", 16), ("default", 8), ("sortFirst", 32)])
@pytest.mark.parametrize("name", CAMS.NAMES)
def test_whole_frames(device, name, order, tile):
    n, w, h, pos, scl, rot, col = _cloud(SCENES["frames"])
    u = CAMS.camera(name, w, h)
    ref = TE.whole_frame(device, u, pos, scl, rot, col, order, "lit", True, tile, w, h)
    print(f"{name} {order} tile {tile}: {ref['indices'].shape[0]} list entries, longest {int(ref['counts'].max())}, counts, lists and "
          f"ProjectedSplats bit-exact; image held off {float((ref['rim'] | ref['near']).mean()):.4f} of the pixels")


# ---- the SH colours ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("name", CAMS.NAMES)
def test_sh_colors_float64(device, name, degree):
    n = 5000
    rng = np.random.default_rng(degree)
    pos, scl, rot, _ = ER.make_cloud(n, degree, degenerate=False)
    sh = rng.normal(0, 0.5, (n, (degree + 1) ** 2, 3)).astype(np.float32)
    op = rng.uniform(0, 1, n).astype(np.float32)
    eye = CAMS.camera(name, 64, 64)[16:19]
    cloud = sr.GaussianCloud.fromArrays(device, pos, scl, rot, opacity=op, sh=sh)
    cloud.updateColors(eye)
    got = cloud.colorOpacity.read(np.float32).reshape(n, 4)
    cloud.destroy()
    want = ER.sh_colors(eye.astype(np.float64), pos, sh, degree, op)
    e = float(np.abs(got - want).max())
    print(f"{name} degree {degree}: max |colour - float64| {e:.3g}")
    assert e <= 2e-6


# ---- the projector's backward --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CLOUDS, ids=lambda c: f"n{c[0]}")
@pytest.mark.parametrize("name", CAMS.NAMES)
def test_project_backward(device, name, case):
    """splat_project_ellipsoid_backward and _backward_depth against GR.records64 (+ DR.depth64) differentiated by autograd."""
    n, w, h, pos, scl, rot, _ = _cloud(case)
    u = CAMS.camera(name, w, h)
    rng = np.random.default_rng(case[3])
    grec = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
    gz = rng.uniform(-1, 1, n).astype(np.float32)
    cull = GR.culled(u, pos, scl, rot)
    good = GR.sigma2_cond(u, pos, scl, rot) <= 1e4
    assert good.sum() >= n / 3 and not (good & cull).any()
    for depth in (False, True):
        gp, gs, gq = TC.project_plain(device, u, pos, scl, rot, grec, gz if depth else None)
        assert np.isfinite(gp).all() and np.isfinite(gs).all() and np.isfinite(gq).all()
        assert (gp[cull] == 0).all() and (gs[cull] == 0).all() and (gq[cull] == 0).all()
        P = torch.tensor(pos.astype(np.float64), requires_grad=True)
        S = torch.tensor(scl.astype(np.float64), requires_grad=True)
        Q = torch.tensor(rot.astype(np.float64), requires_grad=True)
        L = (GR.records64(u, P, S, Q, ~cull) * torch.as_tensor(grec.astype(np.float64))).sum()
        if depth:
            L = L + (DR.depth64(u, P) * torch.as_tensor(np.where(cull, 0.0, gz.astype(np.float64)))).sum()
        L.backward()
        worst = {}
        for what, got, want in (("position", gp, P.grad.numpy()), ("scale", gs, S.grad.numpy()), ("rotation", gq, Q.grad.numpy())):
            worst[what] = max(rel_l2(got[good, k], want[good, k]) for k in range(3 if what != "rotation" else 4))
            if what != "rotation":
                assert (got[:, 3] == 0).all()
        print(f"{name} n={n} {'with depth' if depth else 'records only'}: {int(good.sum())} rows, worst relative L2 per component "
              + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()) + f"; {int(cull.sum())} culled rows exact zeros")
        for what, e in worst.items():
            assert e <= BOUND, f"{name} {what}: relative L2 {e:.3g}"


# ---- the camera's backward -----------------------------------------------------------------------------------------------------
def check_entries(got, want, label):
    """The 12 entries of dL/dVP the frame reads, one by one: |got - want| <= BOUND max|want over the 12|."""
    g, wv = np.asarray(got, np.float64)[CR.VP_ROWS_013], np.asarray(want, np.float64)[CR.VP_ROWS_013]
    scale = np.abs(wv).max()
    err = np.abs(g - wv) / scale
    k = int(err.argmax())
    print(f"{label}: per-entry VP error {err.max():.3g} of the largest entry (worst at m[{CR.VP_ROWS_013[k]}]; smallest |entry| "
          f"{np.abs(wv).min() / scale:.3g} of the largest)")
    assert scale > 0 and (err <= BOUND).all(), f"{label}: dL/dVP entries {[CR.VP_ROWS_013[i] for i in np.nonzero(err > BOUND)[0]]} are off by " \
                                               f"{err[err > BOUND]} of the largest entry"
    return float(err.max())


@pytest.mark.parametrize("case", CLOUDS, ids=lambda c: f"n{c[0]}")
@pytest.mark.parametrize("name", CAMS.NAMES)
def test_project_backward_camera(device, name, case):
    n, w, h, pos, scl, rot, _ = _cloud(case)
    u = CAMS.camera(name, w, h)
    rng = np.random.default_rng(case[3])
    grec = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
    gz = rng.uniform(-1, 1, n).astype(np.float32)
    good = GR.sigma2_cond(u, pos, scl, rot) <= 1e4
    assert good.sum() >= n / 3
    grec[~good] = 0
    gz[~good] = 0
    cull = GR.culled(u, pos, scl, rot)
    # culled splats must add exact zeros whatever their upstream
    grec[cull] = rng.uniform(-1, 1, (int(cull.sum()), 8)).astype(np.float32)
    gz[cull] = 1.0
    for depth in (True, False):
        label = f"{name} n={n} {'depth' if depth else 'colour'}"
        rc, gp, gs, gq, gu = TC.project_camera(device, u, pos, scl, rot, grec, gz if depth else None)
        assert rc == 0
        want = CR.project_camera_grads(u, pos, scl, rot, ~cull, grec, gz if depth else None)
        TC._check_block(gu, want, depth, label)
        check_entries(gu[:22], want, label)
        plain = TC.project_plain(device, u, pos, scl, rot, grec, gz if depth else None)
        for what, a, b in zip(("gpos", "gscl", "grot"), (gp, gs, gq), plain):
            assert np.array_equal(bits(a), bits(b)), f"{label}: {what} differs from the entry point without the camera"


@pytest.mark.parametrize("degree", [1, 2, 3])
@pytest.mark.parametrize("name", CAMS.NAMES)
def test_sh_backward_camera(device, name, degree):
    n = 5000
    rng = np.random.default_rng(degree + 20)
    pos, _, _, _ = ER.make_cloud(n, degree + 20, degenerate=False)
    sh = rng.normal(0, 0.5, (n, (degree + 1) ** 2, 3)).astype(np.float32)
    op = rng.uniform(0, 1, n).astype(np.float32)
    gcol = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    eye = CAMS.camera(name, 64, 64)[16:19].astype(np.float32)
    rc, gsh, gp, gop, ge = TC.sh_camera(device, eye, pos, sh, degree, op, gcol)
    assert rc == 0 and np.isfinite(gsh).all() and np.isfinite(gp).all() and np.isfinite(ge[:4]).all()
    assert (bits(ge[3:4]) == 0).all() and (bits(ge[4:]) == TC.SENT).all()
    passed = ER.sh_colors(eye, pos, sh, degree, op, dtype=np.float32)[:, :3] > 0
    E = torch.tensor(eye.astype(np.float64), requires_grad=True)
    P = torch.tensor(pos.astype(np.float64), requires_grad=True)
    out = CR.sh_colors64(E, P, torch.as_tensor(sh.astype(np.float64)), degree, torch.as_tensor(op.astype(np.float64)), passed)
    (out * torch.as_tensor(gcol.astype(np.float64))).sum().backward()
    e = rel_l2(ge[:3], E.grad.numpy())
    e_p = float(np.abs(gp.reshape(n, 4)[:, :3] - P.grad.numpy()[:, :3]).max())
    print(f"{name} sh degree {degree}: eye relative L2 {e:.3g}, max |grad_positions - float64| {e_p:.3g}")
    assert e <= BOUND, f"eye relative L2 {e:.3g}"
    assert e_p <= 1e-5 * max(1.0, float(np.abs(P.grad.numpy()).max()))


# ---- the chain -----------------------------------------------------------------------------------------------------------------
def _chain_scene(u, degree=1):
    """test_render_gaussians_camera_gradient's scene under the block u: ill-conditioned splats are left out by making them
    transparent on both sides (a row mask cannot be applied to a sum)."""
    n, w, h, seed = SCENES["chain"][:4]
    pos, scl, rot, col, sh, op = TD._scene_with_sh(n, w, h, seed, degree)
    cull = GR.culled(u, pos, scl, rot)
    good = (GR.sigma2_cond(u, pos, scl, rot) <= 1e4) & ~cull
    assert good.sum() >= n / 3
    op = np.where(good | cull, op, 0).astype(np.float32)
    col = col.copy()
    col[:, 3] = op
    g, gd = TD._upstreams(u, pos, scl, rot, col, w, h, seed)
    return n, w, h, pos, scl, rot, op, sh, good, g, gd


LEAVES = ("means", "scales", "rotations", "opacities", "sh")


def _reference_leaves(u, U, pos, scl, rot, op, sh, degree, w, h, g, gd):
    """The float64 chain of TC._reference_chain_camera with every splat tensor a leaf: name -> gradient (after backward)."""
    t = {k: torch.tensor(a.astype(np.float64), requires_grad=True) for k, a in zip(LEAVES, (pos, scl, rot, op, sh))}
    TC._reference_chain_camera_loss(u, U, t["means"], t["scales"], t["rotations"], t["opacities"], t["sh"], degree, w, h, g, gd).backward()
    return {k: v.grad.numpy() for k, v in t.items()}


def _check_leaves(leaves, want, good, label):
    figures = {}
    for k in LEAVES:
        got = leaves[k].grad.detach().cpu().numpy()
        assert np.isfinite(got).all(), f"{label}: {k}"
        rows = good if k in ("means", "scales", "rotations") else np.ones(got.shape[0], bool)
        figures[k] = rel_l2(got[rows].reshape(-1), want[k][rows].reshape(-1))
    print(f"{label}: per-leaf relative L2 " + ", ".join(f"{k} {v:.3g}" for k, v in figures.items()))
    for k, e in figures.items():
        assert e <= BOUND, f"{label}: {k} relative L2 {e:.3g}"


def _check_camera(got, want, label):
    got = np.asarray(got, np.float64)
    assert np.isfinite(got).all(), label
    assert (got[CR.VP_ROW_2] == 0).all() and (got[19:22] == 0).all()
    e_vp, e_eye = rel_l2(got[CR.VP_ROWS_013], want[CR.VP_ROWS_013]), rel_l2(got[16:19], want[16:19])
    print(f"{label}: VP relative L2 {e_vp:.3g}, eye relative L2 {e_eye:.3g}")
    per_entry = check_entries(got, want, label)
    assert e_vp <= BOUND, f"{label}: VP relative L2 {e_vp:.3g}"
    assert e_eye <= BOUND, f"{label}: eye relative L2 {e_eye:.3g}"
    return e_vp, e_eye, per_entry


@pytest.mark.parametrize("name", CHAIN_CAMERAS)
def test_render_gaussians_camera_gradient(device, name):
    """render_gaussians(..., return_depth=True) with a uniforms tensor that requires grad: dL/du and every leaf's gradient
    against the float64 chain, as test_gpu_ellipsoid_camera_grad.py's test of that name does under the default camera."""
    degree = 1
    u = CAMS.camera(name, *SCENES["chain"][1:3])
    n, w, h, pos, scl, rot, op, sh, good, g, gd = _chain_scene(u, degree)
    U = CR.utensor(u)
    want = _reference_leaves(u, U, pos, scl, rot, op, sh, degree, w, h, g, gd)
    leaves = {k: TD._leaf(a) for k, a in zip(LEAVES, (pos, scl, rot, op, sh))}
    ut = torch.tensor(u, dtype=torch.float32, device="cuda", requires_grad=True)
    TD._torch_loss(ut, leaves, w, h, g, gd, degree).backward()
    assert ut.grad is not None and ut.grad.shape == ut.shape
    _check_camera(ut.grad.detach().cpu().numpy(), U.grad.numpy(), f"chain {name}")
    _check_leaves(leaves, want, good, f"chain {name}")


@pytest.mark.parametrize("name", [c for c in CHAIN_CAMERAS if c in CAMS.PINHOLES])
def test_render_gaussians_gradient_reaches_the_pinhole_pose(device, name):
    """The block built inside the graph: pinhole_uniforms(R, t, fx, fy, cx, cy) of leaf tensors.  The gradients that reach R, t
    and the four intrinsics against the float64 chain differentiated through a float64 pinhole_uniforms."""
    from splat_renderer_amd import autograd as AG
    degree = 1
    w, h = SCENES["chain"][1:3]
    params = CAMS.pinhole_params(w, h)[name]

    def pose_leaves():
        R = torch.tensor(params[0], dtype=torch.float64, requires_grad=True)
        t = torch.tensor(params[1], dtype=torch.float64, requires_grad=True)
        k = torch.tensor(params[2:], dtype=torch.float64, requires_grad=True)
        return R, t, k, AG.pinhole_uniforms(R, t, k[0], k[1], k[2], k[3], w, h)
    R0, t0, k0, U = pose_leaves()
    u = U.detach().numpy().astype(np.float32)
    assert np.array_equal(bits(u), bits(CAMS.camera(name, w, h)))
    n, w, h, pos, scl, rot, op, sh, good, g, gd = _chain_scene(u, degree)
    want = _reference_leaves(u, U, pos, scl, rot, op, sh, degree, w, h, g, gd)
    R1, t1, k1, U1 = pose_leaves()
    leaves = {k: TD._leaf(a) for k, a in zip(LEAVES, (pos, scl, rot, op, sh))}
    TD._torch_loss(U1, leaves, w, h, g, gd, degree).backward()
    figures = {}
    for what, got, ref in (("R", R1.grad, R0.grad), ("t", t1.grad, t0.grad), ("intrinsics", k1.grad, k0.grad)):
        assert got is not None and torch.isfinite(got).all(), what
        figures[what] = rel_l2(got.numpy().reshape(-1), ref.numpy().reshape(-1))
    print(f"pose {name}: relative L2 " + ", ".join(f"{k} {v:.3g}" for k, v in figures.items()))
    for what, e in figures.items():
        assert e <= BOUND, f"pose {name}: {what} relative L2 {e:.3g}"
    _check_leaves(leaves, want, good, f"pose {name}")


# ---- the splat at the eye ------------------------------------------------------------------------------------------------------
ROW = 17


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("name", ["pinhole_at_origin", "orbit_default"])
def test_a_splat_at_the_eye_staged(device, name, degree):
    """splat_sh_colors, splat_sh_colors_backward and splat_sh_colors_backward_camera on a cloud whose row 17 is the eye: finite
    outputs; that row's colour max(0.5 + C0 sh_0, 0), its grad_sh C0 g in row 0 and zeros below, its grad_positions zeros, its
    grad_opacity passed through; every other row bit-equal to the call without row 17's change; dL/deye the float64 one."""
    n = 5000
    rng = np.random.default_rng(degree + 40)
    away, scl, rot, _ = ER.make_cloud(n, degree + 40, degenerate=False)
    nb = (degree + 1) ** 2
    sh = rng.normal(0, 0.5, (n, nb, 3)).astype(np.float32)
    op = rng.uniform(0, 1, n).astype(np.float32)
    gcol = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    eye = CAMS.camera(name, 64, 64)[16:19].astype(np.float32)
    pos = away.copy()
    pos[ROW, :3] = eye + np.float32(0)  # (the eye of pinhole_at_origin is -0: the position is +0)
    assert not ER.has_direction(eye, pos)[ROW] and ER.has_direction(eye, away).all()
    others = np.arange(n) != ROW

    def colours(p):
        cloud = sr.GaussianCloud.fromArrays(device, p, scl, rot, opacity=op, sh=sh)
        cloud.updateColors(eye)
        out = cloud.colorOpacity.read(np.float32).reshape(n, 4)
        cloud.destroy()
        return out
    col, col_away = colours(pos), colours(away)
    want_row = np.maximum(0.5 + ER.SH_C0 * sh[ROW, 0].astype(np.float64), 0)
    print(f"{name} degree {degree}: forward finite {bool(np.isfinite(col).all())}, row {ROW} colour {col[ROW, :3]} (want {want_row})")
    assert np.isfinite(col).all(), f"colour of the splat at the eye: {col[ROW]}"
    assert np.abs(col[ROW, :3] - want_row).max() <= 2e-6 and col[ROW, 3] == op[ROW]
    assert np.array_equal(bits(col[others]), bits(col_away[others]))
    assert np.abs(col - ER.sh_colors(eye.astype(np.float64), pos, sh, degree, op)).max() <= 2e-6
    passed = ER.sh_colors(eye, pos, sh, degree, op, dtype=np.float32)[:, :3] > 0
    for camera in (False, True):
        label = f"{name} degree {degree} {'_backward_camera' if camera else '_backward'}"
        rc, gsh, gp, gop, ge = TC.sh_camera(device, eye, pos, sh, degree, op, gcol, camera=camera)
        rc2, gsh2, gp2, gop2, _ = TC.sh_camera(device, eye, away, sh, degree, op, gcol, camera=camera)
        assert rc == 0 and rc2 == 0
        gsh, gp, gsh2, gp2 = gsh.reshape(n, nb, 3), gp.reshape(n, 4), gsh2.reshape(n, nb, 3), gp2.reshape(n, 4)
        finite = bool(np.isfinite(gsh).all() and np.isfinite(gp).all() and np.isfinite(gop).all() and (not camera or np.isfinite(ge[:4]).all()))
        print(f"{label}: finite {finite}; row {ROW}: grad_sh[0] {gsh[ROW, 0]}, max |grad_sh[1:]| "
              f"{np.abs(gsh[ROW, 1:]).max(initial=0):.3g}, grad_positions {gp[ROW]}" + (f", grad_eye {ge[:3]}" if camera else ""))
        assert finite, f"{label}: not finite (grad_sh row {gsh[ROW]}, grad_positions {gp[ROW]}, grad_eye {ge[:4]})"
        want0 = np.float32(ER.SH_C0) * np.where(passed[ROW], gcol[ROW, :3], 0).astype(np.float32)
        assert np.abs(gsh[ROW, 0] - want0).max() <= 1e-7 and (gsh[ROW, 1:] == 0).all() and (gp[ROW] == 0).all()
        assert np.array_equal(gop, gcol[:, 3])
        assert np.array_equal(bits(gsh[others]), bits(gsh2[others])) and np.array_equal(bits(gp[others]), bits(gp2[others]))
        if not camera:
            continue
        assert (bits(ge[3:4]) == 0).all() and (bits(ge[4:]) == TC.SENT).all()
        if degree == 0:
            assert (bits(ge[:3]) & 0x7FFFFFFF == 0).all()
            continue
        E = torch.tensor(eye.astype(np.float64), requires_grad=True)
        out = CR.sh_colors64(E, torch.as_tensor(pos[others].astype(np.float64)), torch.as_tensor(sh[others].astype(np.float64)), degree,
                             torch.as_tensor(op[others].astype(np.float64)), passed[others])
        (out * torch.as_tensor(gcol[others].astype(np.float64))).sum().backward()
        e = rel_l2(ge[:3], E.grad.numpy())
        print(f"{label}: eye relative L2 {e:.3g} against float64 with row {ROW} masked")
        assert e <= BOUND, f"{label}: eye relative L2 {e:.3g}"


@pytest.mark.parametrize("name", ["pinhole_at_origin", "orbit_default"])
def test_a_splat_at_the_eye_end_to_end(device, name):
    """render_gaussians + photometric_loss + backward with uniforms that require grad, on a cloud whose row 17 is the eye: the
    projector culls it (clip w = 0), so the image is that of the cloud without the row, every gradient is finite, and the other
    splats' and the camera's gradients are those of the cloud without it (the chain test's bound: relative L2 <= 1e-4)."""
    from splat_renderer_amd import autograd as AG
    degree = 1
    n, w, h, seed = SCENES["chain"][:4]
    u = CAMS.camera(name, w, h)
    pos, scl, rot, col, sh, op = TD._scene_with_sh(n, w, h, seed, degree)
    pos = pos.copy()
    pos[ROW] = u[16:19] + np.float32(0)
    assert GR.culled(u, pos, scl, rot)[ROW] and not ER.has_direction(u[16:19], pos)[ROW]
    others = np.arange(n) != ROW
    good = (GR.sigma2_cond(u, pos, scl, rot) <= 1e4)
    target = torch.as_tensor(np.random.default_rng(seed).uniform(0, 1, (h, w, 3)).astype(np.float32), device="cuda")

    def run(rows):
        leaves = {k: TD._leaf(a[rows]) for k, a in zip(LEAVES, (pos, scl, rot, op, sh))}
        ut = torch.tensor(u, dtype=torch.float32, device="cuda", requires_grad=True)
        rgb, _alpha = AG.render_gaussians(ut, leaves["means"], leaves["scales"], leaves["rotations"], leaves["opacities"], sh=leaves["sh"],
                                          width=w, height=h, degree=degree)
        loss = AG.photometric_loss(rgb, target)
        loss.backward()
        return rgb.detach().cpu().numpy(), float(loss.detach()), {k: v.grad.detach().cpu().numpy() for k, v in leaves.items()}, \
            ut.grad.detach().cpu().numpy().astype(np.float64)
    img, loss, grads, gu = run(np.ones(n, bool))
    img0, loss0, grads0, gu0 = run(others)
    finite = {k: bool(np.isfinite(v).all()) for k, v in grads.items()}
    finite["uniforms"] = bool(np.isfinite(gu).all())
    print(f"end to end {name}: loss {loss:.6g} (without the row {loss0:.6g}); finite gradients {finite}; dL/deye {gu[16:19]}")
    assert np.isfinite(img).all() and np.array_equal(bits(img), bits(img0)), "the culled splat changed the image"
    assert all(finite.values()), f"end to end {name}: gradients that are not finite: {[k for k, v in finite.items() if not v]}"
    figures = {}
    for k in LEAVES:
        rows = good[others] if k in ("means", "scales", "rotations") else np.ones(n - 1, bool)
        figures[k] = rel_l2(grads[k][others][rows].reshape(-1), grads0[k][rows].astype(np.float64).reshape(-1))
    figures["VP"] = rel_l2(gu[CR.VP_ROWS_013], gu0[CR.VP_ROWS_013])
    figures["eye"] = rel_l2(gu[16:19], gu0[16:19])
    print(f"end to end {name}: relative L2 to the cloud without row {ROW}: " + ", ".join(f"{k} {v:.3g}" for k, v in figures.items()))
    for k, e in figures.items():
        assert e <= BOUND, f"end to end {name}: {k} relative L2 {e:.3g}"
    # the row itself: the culled splat receives zeros from the projector and from the SH direction
    assert (grads["means"][ROW] == 0).all() and (grads["scales"][ROW] == 0).all() and (grads["rotations"][ROW] == 0).all()
