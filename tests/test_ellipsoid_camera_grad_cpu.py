"""CPU checks of the camera-gradient reference (tests/ellipsoid_camera_grad_ref.py), of autograd.pinhole_uniforms and of the
bindings of the two camera entry points."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import oracle as O
from tests import ellipsoid_camera_grad_ref as CR
from tests import ellipsoid_depth_grad_ref as DR
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("splat_project_ellipsoid_backward_camera", "splat_sh_colors_backward_camera")
D = torch.float64


def camera_u(w, h):
    vp, eye = O.camera(aspect=w / h)
    return O.uniforms(vp, eye, w, h)


def _t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def test_records_equal_the_constant_camera_restatement():
    n, w, h = 3000, 160, 120
    pos, scl, rot, _ = ER.make_cloud(n, 1, 1.0, 0.03)
    u = camera_u(w, h)
    keep = ~GR.culled(u, pos, scl, rot)
    assert keep.sum() > n // 2
    want = GR.records64(u, _t64(pos), _t64(scl), _t64(rot), keep)
    got = CR.records64(CR.utensor(u, requires_grad=False), _t64(pos), _t64(scl), _t64(rot), keep)
    assert torch.equal(got, want)
    # (make_cloud's degenerate splats include a non-finite position: NaN on both sides)
    got_z, want_z = CR.depth64(CR.utensor(u, False), _t64(pos)), DR.depth64(u, _t64(pos))
    assert torch.equal(torch.isnan(got_z), torch.isnan(want_z)) and torch.equal(got_z[keep], want_z[keep])


def test_gradcheck_of_the_records_and_depth_with_respect_to_the_camera():
    w, h = 160, 120
    pos, scl, rot, _ = ER.make_cloud(40, 5, 0.6, 0.05, degenerate=False)
    u = camera_u(w, h)
    keep = ~GR.culled(u, pos, scl, rot)
    rows = np.nonzero(keep & (GR.sigma2_cond(u, pos, scl, rot) <= 1e4))[0][:6]
    assert rows.size == 6
    P, S, Q = _t64(pos[rows]), _t64(scl[rows]), _t64(rot[rows])
    k = np.ones(rows.size, bool)
    U = CR.utensor(u)

    def f(uu):
        return CR.records64(uu, P, S, Q, k)[:, [0, 1, 2, 3, 5]], CR.depth64(uu, P)
    # (W and H enter as constants: the check perturbs VP, the eye and time)
    head = U.detach()[:20].clone().requires_grad_()
    assert torch.autograd.gradcheck(lambda v: f(torch.cat([v, U.detach()[20:]])), (head,), eps=1e-6, atol=1e-6, rtol=1e-5)
    # row 2 of VP, time, W and H: no gradient; the records do not read the eye, the depth reads nothing else
    rec, z = f(U)
    g_rec, = torch.autograd.grad(rec.sum(), U, retain_graph=True)
    g_z, = torch.autograd.grad(z.sum(), U)
    assert (g_rec[CR.VP_ROW_2] == 0).all() and (g_rec[16:] == 0).all() and (g_rec[CR.VP_ROWS_013] != 0).all()
    assert (g_z[:16] == 0).all() and (g_z[19:] == 0).all() and (g_z[16:19] != 0).all()


@pytest.mark.parametrize("degree", [1, 2, 3])
def test_gradcheck_of_the_sh_colours_with_respect_to_the_eye(degree):
    n = 5
    rng = np.random.default_rng(degree)
    pos = rng.normal(0, 1, (n, 3))
    sh = rng.normal(0, 0.5, (n, (degree + 1) ** 2, 3))
    eye = torch.tensor([0.3, -2.0, 1.5], dtype=D, requires_grad=True)
    mask = np.ones((n, 3), bool)
    mask[1, 0] = False
    assert torch.autograd.gradcheck(lambda e: CR.sh_colors64(e, _t64(pos), _t64(sh), degree, _t64(np.ones(n)), mask), (eye,), eps=1e-6,
                                    atol=1e-7)
    got = CR.sh_colors64(eye.detach(), _t64(pos), _t64(sh), degree, _t64(np.ones(n)), mask)
    want = GR.sh_colors64(eye.detach().numpy(), _t64(pos), _t64(sh), degree, _t64(np.ones(n)), mask)
    assert torch.equal(got, want)


def _random_pose(rng):
    q, _ = np.linalg.qr(rng.normal(0, 1, (3, 3)))
    if np.linalg.det(q) < 0:
        q[:, 0] = -q[:, 0]
    return q, rng.normal(0, 0.3, 3) + np.array([0.0, 0.0, 3.0])


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_pinhole_uniforms_lands_points_on_their_pixels(seed):
    from splat_renderer_amd import autograd as AG
    rng = np.random.default_rng(seed)
    w, h = (160, 120) if seed % 2 == 0 else (333, 200)
    R, t = _random_pose(rng)
    fx, fy = rng.uniform(0.8, 1.6, 2) * w
    cx, cy = w / 2 + rng.uniform(-10, 10), h / 2 + rng.uniform(-10, 10)
    u = AG.pinhole_uniforms(torch.as_tensor(R), torch.as_tensor(t), fx, fy, cx, cy, w, h)
    assert u.shape == (22,) and u.dtype == D
    assert torch.allclose(u[16:19], torch.as_tensor(-R.T @ t), rtol=0, atol=1e-15)
    assert float(u[20]) == w and float(u[21]) == h and float(u[19]) == 0
    n = 200
    X = rng.normal(0, 0.6, (n, 3))
    Xc = X @ R.T + t
    front = Xc[:, 2] > 0.5
    assert front.sum() > n // 2
    pos = np.concatenate([X, np.ones((n, 1))], axis=1).astype(np.float32)
    scl = np.full((n, 4), 0.01, np.float32)
    rot = np.tile(np.array([1, 0, 0, 0], np.float32), (n, 1))
    u32 = u.numpy().astype(np.float32)
    rec, _, _ = ER.project(u32, pos, scl, rot)
    live = front & (rec != 0).any(axis=1)
    assert live.sum() > n // 2
    Xc32 = pos[:, :3].astype(np.float64) @ R.T + t
    px, py = fx * Xc32[:, 0] / Xc32[:, 2] + cx, fy * Xc32[:, 1] / Xc32[:, 2] + cy
    # binary32 rounding: VP's entries, four products and three sums per clip coordinate, a divide and the screen map, each
    # relative 2^-24 of magnitudes up to ~ max(W, H) (1 + |clip| / w): a few ulps of the screen size
    tol = 32 * 2.0 ** -24 * max(w, h) * (1 + np.abs(Xc32[:, :2]).max(axis=1) / Xc32[:, 2] * max(fx, fy) / max(w, h))
    assert (np.abs(rec[live, 0] - px[live]) <= tol[live]).all(), np.abs(rec[live, 0] - px[live]).max()
    assert (np.abs(rec[live, 1] - py[live]) <= tol[live]).all(), np.abs(rec[live, 1] - py[live]).max()
    # clip w is the camera-space z
    cw = u32[3] * pos[:, 0] + u32[7] * pos[:, 1] + u32[11] * pos[:, 2] + u32[15]
    assert np.allclose(cw, Xc32[:, 2], rtol=1e-5, atol=1e-5)


def test_pinhole_uniforms_is_differentiable():
    from splat_renderer_amd import autograd as AG
    rng = np.random.default_rng(9)
    R, t = _random_pose(rng)
    Rt = torch.tensor(R, dtype=D, requires_grad=True)
    tt = torch.tensor(t, dtype=D, requires_grad=True)
    intr = torch.tensor([200.0, 210.0, 81.0, 59.0], dtype=D, requires_grad=True)
    assert torch.autograd.gradcheck(lambda r, v, k: AG.pinhole_uniforms(r, v, k[0], k[1], k[2], k[3], 160, 120), (Rt, tt, intr))
    # float32 in, float32 out, on the inputs' device
    u = AG.pinhole_uniforms(Rt.detach().float(), tt.detach().float(), 200.0, 210.0, 81.0, 59.0, 160, 120)
    assert u.dtype == torch.float32 and u.shape == (22,)


def test_bindings_declare_the_camera_entry_points():
    from splat_renderer_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES[NEW[0]][1]) == 15 and len(_lib.SIGNATURES[NEW[1]][1]) == 14
    src = open(os.path.join(ROOT, "splat_renderer_amd", "napi", "splat_napi.c")).read()
    exported = set(re.findall(r"EXPORT\(([a-z0-9_]+)\)", src.split("napi_property_descriptor d[]")[1]))
    assert {n[len("splat_"):] for n in NEW} <= exported
    header = open(os.path.join(ROOT, "include", "splat.h")).read()
    assert all(re.search(rf"\bint {n}\(", header) for n in NEW)
    assert "#define SPLAT_ABI_VERSION 3" in header or re.search(r"SPLAT_ABI_VERSION\s+3\b", header)
