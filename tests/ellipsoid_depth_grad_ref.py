"""The depth map of an ellipsoid frame in float64 for its gradients (include/splat.h, "Gradients of the depth map"): the AOV
depth D = sum w z / sum w over tests/ellipsoid_grad_ref.py's recorded pairs, differentiable in the records, the colours and
the per-splat z by torch.autograd, the ProjectedSplat depth |p - eye|, and a NumPy restatement of the composite backward's
second walk with the centred depth channel.
"""
import numpy as np
import torch

from tests import ellipsoid_grad_ref as GR

D64 = torch.float64
BG = GR.BG


def composite_depth64(rec, col, z, steps, width, height):
    """GR.composite64's rgb (H W, 3) and alpha (H W), and per pixel zw = sum w z, ws = sum w and D = zw / ws (+inf where
    ws = 0), all float64 and differentiable in rec (n, 8), col (n, 4) and z (n,)."""
    rgb, alpha = GR.composite64(rec, col, steps, width, height)
    P = width * height
    pix_x = torch.arange(P, dtype=D64) % width + 0.5
    pix_y = torch.div(torch.arange(P), width, rounding_mode="floor").to(D64) + 0.5
    T = torch.ones(P, dtype=D64)
    zw = torch.zeros(P, dtype=D64)
    ws = torch.zeros(P, dtype=D64)
    for pix, s, _stop in steps:
        if pix.size == 0:
            continue
        pix_t, s_t = torch.as_tensor(pix, dtype=torch.long), torch.as_tensor(s, dtype=torch.long)
        r = rec[s_t]
        dx, dy = pix_x[pix_t] - r[:, 0], pix_y[pix_t] - r[:, 1]
        u = r[:, 2] * dx + r[:, 3] * dy
        v = r[:, 4] * dx + r[:, 5] * dy
        a = col[s_t, 3] * torch.exp(-4.5 * (u * u + v * v))
        Tp = T[pix_t]
        w = Tp * a
        zw = zw.index_add(0, pix_t, w * z[s_t])
        ws = ws.index_add(0, pix_t, w)
        T = T.index_put((pix_t,), Tp * (1 - a))
    some = ws > 0
    D = torch.where(some, zw / torch.where(some, ws, torch.ones_like(ws)), torch.full_like(ws, np.inf))
    return rgb, alpha, zw, ws, D


def depth64(u, pos):
    """(n,) |p - eye| in float64, differentiable in pos ((n, 3|4) tensor); eye = u[16:19]."""
    eye = torch.as_tensor(np.asarray(u, np.float64)[16:19])
    d = pos[:, :3] - eye[None, :]
    return torch.sqrt((d * d).sum(dim=1))


def upstream_depth(ws, rim, near, seed):
    """Random dL/dD in [-1, 1] (H, W) float32, zero on the rim and near pixels and where ws < 1e-3 (there the gradient is
    G_D / ws: true, but large enough that binary32 rounding of ws dominates the comparison)."""
    rng = np.random.default_rng(seed + 1000)
    g = rng.uniform(-1, 1, ws.shape).astype(np.float32)
    g[rim | near | (ws < 1e-3)] = 0
    return g


def composite_depth_grads(rec32, col32, z32, steps, width, height, g, gd):
    """dL/drec (n, 8), dL/dcol (n, 4), dL/dz (n,) of L = sum g . (rgb, alpha) + sum gd D (gd not read where ws = 0), by
    autograd over composite_depth64."""
    rec = torch.tensor(np.asarray(rec32, np.float64), requires_grad=True)
    col = torch.tensor(np.asarray(col32, np.float64), requires_grad=True)
    z = torch.tensor(np.asarray(z32, np.float64), requires_grad=True)
    rgb, alpha, _zw, ws, D = composite_depth64(rec, col, z, steps, width, height)
    gt = torch.as_tensor(np.asarray(g, np.float64).reshape(-1, 4))
    gdt = torch.as_tensor(np.asarray(gd, np.float64).reshape(-1))
    some = ws > 0
    Dz = torch.where(some, D, torch.zeros_like(D))
    gdt = torch.where(some, gdt, torch.zeros_like(gdt))
    ((rgb * gt[:, :3]).sum() + (alpha * gt[:, 3]).sum() + (Dz * gdt).sum()).backward()
    zg = z.grad.numpy() if z.grad is not None else np.zeros(z.shape[0])
    return rec.grad.numpy(), col.grad.numpy(), zg


def walk2(alpha, col, z, G, GD):
    """The composite backward's second walk for one pixel that consumed all L entries (alpha (L,), col (L, 3), z (L,), float64),
    with G = dL/d(rgb, alpha) and GD = dL/dD: T recovered by division except at the last entry (kept from the first walk),
    D carried as the centred fifth channel.  Returns (dL/dalpha (L,), dL/dc (L, 3), dL/dz (L,))."""
    L = alpha.shape[0]
    T = np.concatenate([[1.0], np.cumprod(1.0 - alpha)])  # T_0 .. T_L, the first walk's
    w = T[:-1] * alpha
    ws = w.sum()
    zw = (w * z).sum()
    D, GDn = (zw / ws, GD / ws) if ws > 0 else (0.0, 0.0)
    S = float(np.dot(G[:3], BG))
    Tn = T[L]
    dA, dc, dz = np.zeros(L), np.zeros((L, 3)), np.zeros(L)
    for i in range(L - 1, -1, -1):
        Ti = T[L - 1] if i == L - 1 else Tn / (1.0 - alpha[i])
        cg = float(np.dot(G[:3], col[i])) + G[3] + GDn * (z[i] - D)
        dA[i] = Ti * (cg - S)
        dc[i] = Ti * alpha[i] * G[:3]
        dz[i] = Ti * alpha[i] * GDn
        S = alpha[i] * cg + (1.0 - alpha[i]) * S
        Tn = Ti
    return dA, dc, dz


def pixel64(alpha, col, z, G, GD):
    """The same pixel's L = G . (rgb, alpha) + GD D by autograd: (dL/dalpha, dL/dc, dL/dz)."""
    a = torch.tensor(alpha, dtype=D64, requires_grad=True)
    c = torch.tensor(col, dtype=D64, requires_grad=True)
    zz = torch.tensor(z, dtype=D64, requires_grad=True)
    T = torch.ones((), dtype=D64)
    rgb = torch.zeros(3, dtype=D64)
    zw = torch.zeros((), dtype=D64)
    ws = torch.zeros((), dtype=D64)
    for i in range(a.shape[0]):
        w = T * a[i]
        rgb = rgb + w * c[i]
        zw = zw + w * zz[i]
        ws = ws + w
        T = T * (1 - a[i])
    rgb = rgb + T * torch.tensor(BG, dtype=D64)
    Gt = torch.as_tensor(np.asarray(G, np.float64))
    loss = (rgb * Gt[:3]).sum() + (1 - T) * Gt[3] + GD * (zw / ws)
    loss.backward()
    return a.grad.numpy(), c.grad.numpy(), zz.grad.numpy()
