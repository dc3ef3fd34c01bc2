"""The float64 restatement of the depth-map normals (tests/depth_normals_ref.py) against analytic planes and against torch
autograd, its validity rules, and the one entry point that needs no device: splat_camera_rays.  No GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from splat_renderer_amd import Camera, _lib
from splat_renderer_amd import autograd as AG
from tests import cameras
from tests import depth_normals_ref as DR

W, H = 37, 29
PLANES = (((0.2, 0.3, -1.0), 0.4), ((-0.5, 0.1, -1.0), -0.2), ((0.0, 0.0, 1.0), 0.3))


def _cams():
    """name -> float32 block: pinhole_uniforms cameras with fx != fy and an off-centre principal point, the Camera class, and a
    camera whose x axis is mirrored."""
    out = {"pinhole_60": DR.pinhole_camera(W, H, 60.0), "pinhole_1200": DR.pinhole_camera(W, H, 1200.0),
           "pinhole_mirrored": DR.pinhole_camera(W, H, 90.0, mirrored=True)}
    R, t, fx, fy, cx, cy = cameras.pinhole_params(W, H)["pinhole_rolled_offaxis"]
    out["pinhole_rolled_offaxis"] = cameras.pinhole(W, H, R, t, fx, fy, cx, cy)
    cam = Camera()
    cam.setAspect(W / H)
    out["camera_class"] = np.asarray(cam.uniforms(W, H), np.float32)
    return out


CAMS = _cams()


def _eye(u):
    M, m = DR.vp_rows(u)
    return -np.linalg.solve(M, m)


@pytest.mark.parametrize("kind", (DR.DISTANCE, DR.Z))
@pytest.mark.parametrize("cam", sorted(CAMS))
def test_planes_give_their_normal_facing_the_eye(cam, kind):
    u = CAMS[cam]
    d = DR.rays(u, W, H)
    seen = 0
    for normal, offset in PLANES:
        z = DR.plane_depth(u, W, H, normal, offset, kind)
        N, valid = DR.normals(z, u, kind)
        if not valid.any():
            continue
        seen += valid.sum()
        t = np.asarray(normal) / np.linalg.norm(normal)
        t = -t if (t * d[H // 2, W // 2]).sum() > 0 else t  # the side that faces the eye
        assert np.abs(N[valid] - t).max() <= 1e-11, (cam, kind, normal)  # (float32 uniforms, float64 arithmetic: measured 1e-13)
        assert ((N * d).sum(axis=2)[valid] < 0).all()
        assert np.abs(np.linalg.norm(N[valid], axis=1) - 1).max() <= 1e-14
        assert (N[~valid] == 0).all()
    assert seen > 0


def test_camera_class_eye_is_the_rays_origin():
    """M eye + m = 0 for the cameras the package builds: the eye the block carries is the point every ray leaves."""
    for name, u in CAMS.items():
        assert np.abs(_eye(u) - u[16:19].astype(np.float64)).max() <= 2e-6 * max(1.0, np.abs(u[16:19]).max()), name


def _bumpy(u, kind, seed=3):
    return DR.depth_maps(u, W, H, kind, seed)


def _leaf(z64):
    """(leaf, depth map): a float64 leaf holding the finite depths, and the map with its non-finite pixels put back."""
    finite = np.isfinite(z64)
    zt = torch.from_numpy(np.where(finite, z64, 1.0)).requires_grad_(True)
    return zt, torch.where(torch.from_numpy(finite), zt, torch.from_numpy(np.where(finite, 0.0, z64)))


@pytest.mark.parametrize("kind", (DR.DISTANCE, DR.Z))
@pytest.mark.parametrize("cam", ("pinhole_60", "pinhole_mirrored", "camera_class"))
def test_hand_written_backward_is_autograd_of_the_forward(cam, kind):
    u = CAMS[cam]
    rng = np.random.default_rng(5)
    for name, z in _bumpy(u, kind).items():
        z64 = z.astype(np.float64)
        gN = rng.standard_normal((H, W, 3))
        F = rng.standard_normal((H, W, 5))
        wt = rng.random((H, W))
        r = DR.forward(z64, u, kind)
        # the map
        zt, zin = _leaf(z64)
        Nt = DR.normals_torch(zin, u, kind)
        assert np.abs(Nt.detach().numpy() - r.N).max() <= 1e-12, name
        (Nt * torch.from_numpy(gN)).sum().backward()
        gz, _ = DR.backward(r, gN)
        want = np.where(np.isfinite(z64), zt.grad.numpy(), 0.0)
        assert np.abs(gz - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), (name, np.abs(gz - want).max())
        # the loss, both gradients
        zt, zin = _leaf(z64)
        Ft = torch.from_numpy(F).requires_grad_(True)
        Lt = DR.loss_torch(Ft, zin, u, torch.from_numpy(wt), kind)
        L, frac, _, r2 = DR.loss(F, z64, u, wt, kind)
        assert abs(L - float(Lt.detach())) <= 1e-12 and frac == r.valid.mean()
        (1.7 * Lt).backward()
        gF, _, gz, _ = DR.loss_backward(r2, F, wt, upstream=1.7)
        assert np.abs(gF - Ft.grad.numpy()[..., :3]).max() <= 1e-14 and (Ft.grad.numpy()[..., 3:] == 0).all()
        want = np.where(np.isfinite(z64), zt.grad.numpy(), 0.0)
        assert np.abs(gz - want).max() <= 1e-9 * max(1.0, np.abs(want).max()), name


def test_validity_rules():
    u = CAMS["pinhole_60"]
    z = _bumpy(u, DR.DISTANCE)["bumpy"].astype(np.float64)
    N, valid = DR.normals(z, u)
    assert valid[1:-1, 1:-1].all() and not valid[0].any() and not valid[-1].any() and not valid[:, 0].any() and not valid[:, -1].any()
    for bad in (np.inf, 0.0, -1.0, np.nan):
        zz = z.copy()
        zz[10, 12] = bad
        Nb, vb = DR.normals(zz, u)
        off = {(10, 11), (10, 13), (9, 12), (11, 12)}  # the pixels whose neighbour it is; its own normal does not read it
        for y in range(8, 13):
            for x in range(10, 15):
                assert vb[y, x] == ((y, x) not in off), (bad, y, x)
        assert (Nb[~vb] == 0).all() and np.isfinite(Nb).all()
        assert np.array_equal(Nb[10, 12], N[10, 12])
        g, b = DR.backward(DR.forward(zz, u), np.where(vb[..., None], 1.0, np.nan) * np.ones(3))  # NaN upstream on invalid pixels
        assert np.isfinite(g).all() and np.isfinite(b).all() and (g[10, 12] == 0 or np.isfinite(bad))
    for w, h in ((1, 1), (2, 7), (7, 2), (3, 3), (3, 4)):
        uu = DR.pinhole_camera(w, h, 20.0)
        zz = DR.plane_depth(uu, w, h, (0.2, 0.3, -1.0), 0.4)
        Ns, vs = DR.normals(zz, uu)
        assert vs.sum() == max(w - 2, 0) * max(h - 2, 0) and (Ns[~vs] == 0).all()
        L, frac, _, _ = DR.loss(np.ones((h, w, 3)), zz, uu)
        if w < 3 or h < 3:
            assert L == 1.0 and frac == 0.0


def _rays(u):
    out = (C.c_double * 10)()
    u = np.ascontiguousarray(u, np.float32)
    rc = _lib.load().splat_camera_rays(u.ctypes.data_as(C.POINTER(C.c_float)), out)
    return rc, np.array(out[:])


@pytest.mark.parametrize("cam", sorted(CAMS))
def test_camera_rays_match_the_numpy_inverse(cam):
    rc, got = _rays(CAMS[cam])
    assert rc == 0
    D0, Dx, Dy, sigma = DR.camera_rays(CAMS[cam])
    for g, want in ((got[0:3], D0), (got[3:6], Dx), (got[6:9], Dy)):
        assert np.linalg.norm(g - want) <= 1e-12 * np.linalg.norm(want), cam
    assert got[9] == sigma
    assert got[9] == (-1.0 if cam == "pinhole_mirrored" else 1.0)


def test_camera_rays_refuse_singular_and_orthographic():
    lib = _lib.load()
    u = CAMS["pinhole_60"].copy()
    ortho = u.copy()
    ortho[[3, 7, 11]] = 0.0  # row 3 of VP = (0, 0, 0, 1): clip w does not depend on the point
    ortho[15] = 1.0
    singular = u.copy()
    singular[[1, 5, 9]] = 2.0 * singular[[0, 4, 8]]  # row 1 parallel to row 0
    for bad in (ortho, singular):
        rc, _ = _rays(bad)
        assert rc == -1
        assert b"singular" in lib.splat_last_error(None)
        with pytest.raises(DR.RefusedCamera):
            DR.camera_rays(bad)
    screen = u.copy()
    screen[20] = 0.0
    assert _rays(screen)[0] == -1
    assert lib.splat_camera_rays(None, (C.c_double * 10)()) == -1


def test_refusals_that_need_no_device():
    z = torch.ones(4, 4)
    with pytest.raises(AG.SplatError):
        AG.depth_normals(z, CAMS["pinhole_60"])  # a CPU tensor
    with pytest.raises(AG.SplatError):
        AG.normal_consistency_loss(torch.ones(4, 4, 3), z, CAMS["pinhole_60"])
    with pytest.raises(AG.SplatError):
        AG.depth_normals(z, CAMS["pinhole_60"], depth_kind="planar")


def test_splat_normals_matches_its_float64_restatement():
    rng = np.random.default_rng(2)
    n = 50
    means, scales, rot = rng.standard_normal((n, 3)), rng.random((n, 3)) + 0.1, rng.standard_normal((n, 4))
    eye = np.array([0.3, -0.2, -4.0])
    got = AG.splat_normals(torch.from_numpy(means), torch.from_numpy(scales), torch.from_numpy(rot), eye).numpy()
    assert np.abs(got - splat_normals_ref(means, scales, rot, eye)).max() <= 1e-14


def splat_normals_ref(means, scales, rot, eye):
    """Per splat: column argmin(scales) of the rotation matrix of the normalised quaternion (w, x, y, z), facing the eye."""
    out = np.zeros((len(means), 3))
    for i, (p, s, q) in enumerate(zip(np.asarray(means, np.float64), np.asarray(scales, np.float64), np.asarray(rot, np.float64))):
        w, x, y, z = q / np.linalg.norm(q)
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        a = R[:, int(np.argmin(s))]
        out[i] = -a if np.dot(p - eye, a) > 0 else a
    return out
