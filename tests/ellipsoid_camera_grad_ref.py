"""The ellipsoid frame's dependence on its camera in float64 for the camera gradients (include/splat.h, "Gradients of the
camera"): tests/ellipsoid_grad_ref.py's records and SH colours and tests/ellipsoid_depth_grad_ref.py's depth restated with the
uniform block `u` (22 floats: VP column-major, eye, time, W, H) as a float64 torch tensor that may require grad, so that
torch.autograd differentiates them with respect to the camera — independently of the kernels' hand-derived sums.

As there, every decision (the culls, the SH clamp, the per-pixel cut and stop) comes from the binary32 pass and is held fixed.
W and H are the screen's integers: they enter as constants (detached), as the library offers no gradient for them.
"""
import numpy as np
import torch

from tests import ellipsoid_ref as ER

D = torch.float64
VP_ROWS_013 = [4 * k + r for k in range(4) for r in (0, 1, 3)]  # the 12 entries of VP the records read
VP_ROW_2 = [2, 6, 10, 14]


def utensor(u, requires_grad=True):
    """The uniform block as a float64 leaf."""
    return torch.tensor(np.asarray(u, np.float64), dtype=D, requires_grad=requires_grad)


def records64(u, pos, scl, rot, keep):
    """GR.records64 with u a (22,) float64 tensor: (n, 8) records {c.x, c.y, B00, B01, 0, B11, 0, 0} of the splats in `keep`
    (zeros elsewhere), differentiable in u, pos, scl, rot."""
    m = u
    n = pos.shape[0]
    idx = torch.as_tensor(np.nonzero(np.asarray(keep))[0], dtype=torch.long)
    p, s, q = pos[idx, :3], scl[idx, :3], rot[idx]
    q = q / torch.sqrt((q * q).sum(dim=1, keepdim=True))
    qr, qx, qy, qz = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = [[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qr * qz), 2 * (qx * qz + qr * qy)],
         [2 * (qx * qy + qr * qz), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qr * qx)],
         [2 * (qx * qz - qr * qy), 2 * (qy * qz + qr * qx), 1 - 2 * (qx * qx + qy * qy)]]
    M = [[R[i][j] * s[:, j] for j in range(3)] for i in range(3)]
    cx = m[0] * p[:, 0] + m[4] * p[:, 1] + m[8] * p[:, 2] + m[12]
    cy = m[1] * p[:, 0] + m[5] * p[:, 1] + m[9] * p[:, 2] + m[13]
    cw = m[3] * p[:, 0] + m[7] * p[:, 1] + m[11] * p[:, 2] + m[15]
    nx, ny = cx / cw, cy / cw
    W, H = float(m[20].detach()), float(m[21].detach())
    scx, scy = (nx + 1) * 0.5 * W, (1 - ny) * 0.5 * H
    ax, ay = 0.5 * W / cw, 0.5 * H / cw
    j0 = [ax * (m[4 * k] - nx * m[4 * k + 3]) for k in range(3)]
    j1 = [ay * (ny * m[4 * k + 3] - m[4 * k + 1]) for k in range(3)]
    t0 = [j0[0] * M[0][c] + j0[1] * M[1][c] + j0[2] * M[2][c] for c in range(3)]
    t1 = [j1[0] * M[0][c] + j1[1] * M[1][c] + j1[2] * M[2][c] for c in range(3)]
    a = t0[0] * t0[0] + t0[1] * t0[1] + t0[2] * t0[2] + 0.3
    b = t0[0] * t1[0] + t0[1] * t1[1] + t0[2] * t1[2]
    c = t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2] + 0.3
    det = a * c - b * b
    z = torch.zeros_like(a)
    vals = torch.stack([scx, scy, torch.sqrt(c / det) / 3, -b / torch.sqrt(c * det) / 3, z, 1 / torch.sqrt(c) / 3, z, z], dim=1)
    out = torch.zeros((n, 8), dtype=D)
    return out.index_put((idx,), vals)


def depth64(u, pos):
    """(n,) |p - eye| in float64, eye = u[16:19]: differentiable in u and pos."""
    d = pos[:, :3] - u[16:19][None, :]
    return torch.sqrt((d * d).sum(dim=1))


def sh_colors64(eye, pos, sh, degree, opacity, pass_mask):
    """GR.sh_colors64 with eye a (3,) float64 tensor: (n, 4), rgb = 0.5 + sum_k Y_k(normalize(p - eye)) sh_k where pass_mask
    (the binary32 forward did not clamp), 0 elsewhere; differentiable in eye, pos, sh, opacity."""
    d = pos[:, :3] - eye[None, :]
    # no direction (the binary32 decision: a splat at the eye, a position that is not finite): (0, 0, 0), and no gradient through it
    ok = torch.as_tensor(ER.has_direction(eye.detach().numpy(), pos.detach().numpy()))[:, None]
    d = torch.where(ok, d, torch.ones_like(d))
    d = torch.where(ok, d / torch.sqrt((d * d).sum(dim=1, keepdim=True)), torch.zeros_like(d))
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    Y = [torch.full_like(x, ER.SH_C0)]
    if degree > 0:
        Y += [-ER.SH_C1 * y, ER.SH_C1 * z, -ER.SH_C1 * x]
    if degree > 1:
        xx, yy, zz = x * x, y * y, z * z
        c2 = ER.SH_C2
        Y += [c2[0] * x * y, c2[1] * y * z, c2[2] * (2 * zz - xx - yy), c2[3] * x * z, c2[4] * (xx - yy)]
        if degree > 2:
            c3 = ER.SH_C3
            Y += [c3[0] * y * (3 * xx - yy), c3[1] * x * y * z, c3[2] * y * (4 * zz - xx - yy), c3[3] * z * (2 * zz - 3 * xx - 3 * yy),
                  c3[4] * x * (4 * zz - xx - yy), c3[5] * z * (xx - yy), c3[6] * x * (xx - 3 * yy)]
    Yt = torch.stack(Y, dim=1)
    nb = (degree + 1) ** 2
    coef = sh.reshape(pos.shape[0], -1)[:, :3 * nb].reshape(pos.shape[0], nb, 3)
    rgb = 0.5 + torch.einsum("nk,nkc->nc", Yt, coef)
    rgb = torch.where(torch.as_tensor(pass_mask), rgb, torch.zeros_like(rgb))
    return torch.cat([rgb, opacity.reshape(-1, 1)], dim=1)


def project_camera_grads(u, pos, scl, rot, keep, grad_records, grad_depth=None):
    """dL/du (22,) float64 of L = sum grad_records . records + sum grad_depth . |p - eye| over the splats in `keep`, by autograd
    (pos, scl, rot: float32 arrays, held constant)."""
    U = utensor(u)
    P = torch.as_tensor(np.asarray(pos, np.float64))
    S = torch.as_tensor(np.asarray(scl, np.float64))
    Q = torch.as_tensor(np.asarray(rot, np.float64))
    L = (records64(U, P, S, Q, keep) * torch.as_tensor(np.asarray(grad_records, np.float64))).sum()
    if grad_depth is not None:
        rows = torch.as_tensor(np.nonzero(np.asarray(keep))[0], dtype=torch.long)  # (a dropped splat's position may be NaN)
        L = L + (depth64(U, P[rows]) * torch.as_tensor(np.asarray(grad_depth, np.float64))[rows]).sum()
    L.backward()
    return U.grad.numpy()


def rel_l2(got, ref):
    nr = np.linalg.norm(ref)
    return np.linalg.norm(np.asarray(got, np.float64) - ref) / nr if nr > 0 else np.linalg.norm(got)
