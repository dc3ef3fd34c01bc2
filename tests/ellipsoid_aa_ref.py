"""Restatements for the antialiased ellipsoid frames (include/splat.h, "antialiased frames"), beside tests/ellipsoid_ref.py and
tests/ellipsoid_grad_ref.py, which this module extends by import:

rho32():         the 2D Mip filter's factor in binary32, one rounding per operator in csrc/ellipsoid.h's order, so that
                 splat_project_ellipsoid_aa's rho_out compares bit for bit.  The culls are ellipsoid_ref.records()'s.
compensated():   the colour plane (r, g, b, fl32(opacity * rho)).
rho64():         the same factor in torch float64, differentiable in the splat's planes and in the uniform block.
sampling_rate(): splat_sampling_rate_max in binary32.
"""
import numpy as np
import torch

from tests import ellipsoid_ref as ER

F = np.float32
D = torch.float64


def abc32(u, pos, scl, rot):
    """(a0, b, c0) in binary32: |T0|^2, T0.T1, |T1|^2 of T = J M, formed as ellipsoid_ref.records() forms them before it adds
    the 0.3 (the same operations in the same order)."""
    m = np.asarray(u, F)
    p, s, q = (ER._v4(a) for a in (pos, scl, rot))
    with np.errstate(all="ignore"):
        n2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
        k = F(1) / np.sqrt(n2)
        qr, qx, qy, qz = q[:, 0] * k, q[:, 1] * k, q[:, 2] * k, q[:, 3] * k
        one, two = F(1), F(2)
        r = [[one - two * (qy * qy + qz * qz), two * (qx * qy - qr * qz), two * (qx * qz + qr * qy)],
             [two * (qx * qy + qr * qz), one - two * (qx * qx + qz * qz), two * (qy * qz - qr * qx)],
             [two * (qx * qz - qr * qy), two * (qy * qz + qr * qx), one - two * (qx * qx + qy * qy)]]
        M = [[r[i][j] * s[:, j] for j in range(3)] for i in range(3)]
        cx = ((m[0] * p[:, 0] + m[4] * p[:, 1]) + m[8] * p[:, 2]) + m[12]
        cy = ((m[1] * p[:, 0] + m[5] * p[:, 1]) + m[9] * p[:, 2]) + m[13]
        cw = ((m[3] * p[:, 0] + m[7] * p[:, 1]) + m[11] * p[:, 2]) + m[15]
        nx, ny = cx / cw, cy / cw
        icw = F(1) / cw
        ax, ay = (F(0.5) * m[20]) * icw, (F(0.5) * m[21]) * icw
        j0 = [ax * (m[0] - nx * m[3]), ax * (m[4] - nx * m[7]), ax * (m[8] - nx * m[11])]
        j1 = [ay * (ny * m[3] - m[1]), ay * (ny * m[7] - m[5]), ay * (ny * m[11] - m[9])]
        t0 = [(j0[0] * M[0][c] + j0[1] * M[1][c]) + j0[2] * M[2][c] for c in range(3)]
        t1 = [(j1[0] * M[0][c] + j1[1] * M[1][c]) + j1[2] * M[2][c] for c in range(3)]
        a0 = (t0[0] * t0[0] + t0[1] * t0[1]) + t0[2] * t0[2]
        b = (t0[0] * t1[0] + t0[1] * t1[1]) + t0[2] * t1[2]
        c0 = (t1[0] * t1[0] + t1[1] * t1[1]) + t1[2] * t1[2]
    return a0.astype(F), b.astype(F), c0.astype(F)


def rho32(u, pos, scl, rot):
    """(n,) float32: rho = det0 > 0 ? sqrt(det0 / det) : 0 with a = a0 + 0.3, c = c0 + 0.3, det = a c - b b, det0 = a0 c0 - b b;
    0 for every splat ellipsoid_ref.records() culls."""
    a0, b, c0 = abc32(u, pos, scl, rot)
    live = (ER.records(u, pos, scl, rot) != 0).any(axis=1)
    with np.errstate(all="ignore"):
        a, c = a0 + F(0.3), c0 + F(0.3)
        det = a * c - b * b
        det0 = a0 * c0 - b * b
        rho = np.where(det0 > 0, np.sqrt(det0 / det), F(0)).astype(F)
    return np.where(live, rho, F(0)).astype(F)


def compensated(col, rho):
    """(n, 4) float32 (r, g, b, fl32(opacity * rho))."""
    out = np.array(col, F, copy=True)
    out[:, 3] = (out[:, 3] * np.asarray(rho, F)).astype(F)
    return out


def rho64(u, pos, scl, rot, live):
    """(n,) float64 rho of the splats in `live` (zeros elsewhere), differentiable in pos, scl, rot ((n, 3|4) float64 tensors) and
    in u when it is a (22,) float64 tensor (W and H enter as constants).  Beside ellipsoid_grad_ref.records64."""
    m = u if isinstance(u, torch.Tensor) else torch.as_tensor(np.asarray(u, np.float64))
    n = pos.shape[0]
    idx = torch.as_tensor(np.nonzero(np.asarray(live))[0], dtype=torch.long)
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
    ax, ay = 0.5 * W / cw, 0.5 * H / cw
    j0 = [ax * (m[4 * k] - nx * m[4 * k + 3]) for k in range(3)]
    j1 = [ay * (ny * m[4 * k + 3] - m[4 * k + 1]) for k in range(3)]
    t0 = [j0[0] * M[0][c] + j0[1] * M[1][c] + j0[2] * M[2][c] for c in range(3)]
    t1 = [j1[0] * M[0][c] + j1[1] * M[1][c] + j1[2] * M[2][c] for c in range(3)]
    a0 = t0[0] * t0[0] + t0[1] * t0[1] + t0[2] * t0[2]
    b = t0[0] * t1[0] + t0[1] * t1[1] + t0[2] * t1[2]
    c0 = t1[0] * t1[0] + t1[1] * t1[1] + t1[2] * t1[2]
    det = (a0 + 0.3) * (c0 + 0.3) - b * b
    det0 = a0 * c0 - b * b
    out = torch.zeros(n, dtype=D)
    return out.index_put((idx,), torch.sqrt(det0 / det))


def sampling_rate(u, focal_px, near, margin, pos, rate):
    """splat_sampling_rate_max in binary32: rate (n,) with fmaxf(rate, focal_px / c.w) where c.w > near and the screen centre (as
    to_screen() forms it) lies in [-margin W, (1 + margin) W] x [-margin H, (1 + margin) H]; unchanged elsewhere."""
    m = np.asarray(u, F)
    p = ER._v4(pos)
    focal_px, near, margin = F(focal_px), F(near), F(margin)
    with np.errstate(all="ignore"):
        cx = ((m[0] * p[:, 0] + m[4] * p[:, 1]) + m[8] * p[:, 2]) + m[12]
        cy = ((m[1] * p[:, 0] + m[5] * p[:, 1]) + m[9] * p[:, 2]) + m[13]
        cw = ((m[3] * p[:, 0] + m[7] * p[:, 1]) + m[11] * p[:, 2]) + m[15]
        nx, ny = cx / cw, cy / cw
        sx, sy = ((nx + F(1)) * F(0.5)) * m[20], ((F(1) - ny) * F(0.5)) * m[21]
        lo_x, hi_x = (-margin) * m[20], (F(1) + margin) * m[20]
        lo_y, hi_y = (-margin) * m[21], (F(1) + margin) * m[21]
        seen = (cw > near) & (sx >= lo_x) & (sx <= hi_x) & (sy >= lo_y) & (sy <= hi_y)
        new = np.fmax(np.asarray(rate, F), (focal_px / cw).astype(F))
    return np.where(seen, new, np.asarray(rate, F)).astype(F), seen
