"""A torch float64 restatement of the ellipsoid frame for its gradients (include/splat.h, "gradients of a frame of anisotropic 3D
Gaussians"): the records, the SH colours and the composite over given lists, differentiated by torch.autograd — independently of
the kernels' hand-derived formulas.

Every branch decision comes from tests/ellipsoid_ref.py's binary32 pass: which splats the projector culled (records()), and per
pixel which list entries are inside the cut and were consumed before the early-out stop (decisions(), the loop of
ellipsoid_ref.composite recording its choices).  Between those decisions the function is smooth, and that is what is
differentiated.
"""
import numpy as np
import torch

from oracle import np_oracle as NO
from tests import ellipsoid_ref as ER

F = np.float32
D = torch.float64
BG = (0.05, 0.05, 0.1)


def _v(a, cols=4, fill=0.0):
    a = torch.as_tensor(a, dtype=D) if not isinstance(a, torch.Tensor) else a
    if a.shape[1] == 3 and cols == 4:
        a = torch.cat([a, torch.full((a.shape[0], 1), fill, dtype=a.dtype)], dim=1)
    return a


def culled(u, pos, scl, rot):
    """(n,) bool: the binary32 projector's culls (an all-zero record)."""
    return ~(ER.records(u, pos, scl, rot) != 0).any(axis=1)


def records64(u, pos, scl, rot, keep):
    """(n, 8) float64 records {c.x, c.y, B00, B01, 0, B11, 0, 0} of the splats in `keep` (zeros elsewhere), differentiable in
    pos, scl, rot ((n, 3|4) tensors)."""
    m = [float(x) for x in np.asarray(u, np.float64)]
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
    W, H = m[20], m[21]
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


def sigma2_cond(u, pos, scl, rot):
    """(n,) condition number of Sigma2 in float64 (inf for culled splats)."""
    keep = ~culled(u, pos, scl, rot)
    rec = records64(u, _v(pos, 4, 1.0), _v(scl), torch.as_tensor(rot, dtype=D), keep).numpy()
    b00, b01, b11 = rec[:, 2] * 3, rec[:, 3] * 3, rec[:, 5] * 3
    # U = [[b00, b01], [0, b11]], Sigma2^-1 = U^T U: its condition number is Sigma2's
    with np.errstate(all="ignore"):
        sv = np.linalg.svd(np.stack([np.stack([b00, b01], 1), np.stack([np.zeros_like(b11), b11], 1)], 1), compute_uv=False)
        cond = (sv[:, 0] / sv[:, 1]) ** 2
    return np.where(keep, cond, np.inf)


def sh_colors64(eye, pos, sh, degree, opacity, pass_mask):
    """(n, 4) float64: rgb = 0.5 + sum_k Y_k(dir) sh_k where pass_mask (the binary32 forward did not clamp), 0 elsewhere."""
    e = torch.as_tensor(np.asarray(eye, np.float64)[:3])
    d = pos[:, :3] - e[None, :]
    # no direction (the binary32 decision: a splat at the eye, a position that is not finite): (0, 0, 0), and no gradient through it
    ok = torch.as_tensor(ER.has_direction(eye, pos.detach().numpy()))[:, None]
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


def decisions(rec, color_opacity, indices, counts, offsets, width, height, tile=16):
    """ellipsoid_ref.composite's loop (binary32, early-out), recording its choices.  Returns dict(steps=[(pixel, splat, stop)
    per list position], rim, near (H, W) masks, alpha (pair alphas, binary32), img (the binary32 image)).  pixel = y W + x; a
    pair is an entry inside the cut that the pixel consumed; stop marks the entry its early-out stopped at."""
    rec = np.asarray(rec, F)
    col = np.asarray(color_opacity, F)
    bnd, okb = NO.disc_bounds(rec)
    ntx, nty = -(-width // tile), -(-height // tile)
    tiles = np.arange(ntx * nty)
    ly, lx = np.divmod(np.arange(tile * tile), tile)
    px = (tiles % ntx)[:, None] * tile + lx[None, :]
    py = (tiles // ntx)[:, None] * tile + ly[None, :]
    inimg = (px < width) & (py < height)
    flat = np.where(inimg, py * width + px, -1)
    pxf, pyf = px.astype(F) + F(0.5), py.astype(F) + F(0.5)
    shape = px.shape
    T = np.ones(shape, F)
    live = inimg.copy()
    rim = np.zeros(shape, bool)
    near = np.zeros(shape, bool)
    steps, alphas = [], []
    cnt, off = counts.astype(np.int64), offsets.astype(np.int64)
    for i in range(int(cnt.max()) if cnt.size else 0):
        act = np.nonzero((cnt > i) & live.any(axis=1))[0]
        if act.size == 0:
            break
        s = indices[off[act] + i].astype(np.int64)
        r, b = rec[s], bnd[s]
        dx, dy = pxf[act] - r[:, 0:1], pyf[act] - r[:, 1:2]
        with np.errstate(all="ignore"):
            uu, vv = r[:, 2:3] * dx + r[:, 3:4] * dy, r[:, 4:5] * dx + r[:, 5:6] * dy
            d2 = uu * uu + vv * vv
            g = (col[s, 3:4] * np.exp(F(-4.5) * d2)).astype(F)
        inside = ~((pxf[act] < b[:, 0:1]) | (pxf[act] > b[:, 2:3]) | (pyf[act] < b[:, 1:2]) | (pyf[act] > b[:, 3:4]))
        lv = live[act]
        rim[act] |= lv & okb[s][:, None] & (np.abs(d2 - F(1)) <= F(1e-3))
        take = lv & okb[s][:, None] & inside & (d2 <= F(1))
        g = np.where(take, g, F(0))
        Ta = T[act]
        Tn = (Ta * (F(1) - g)).astype(F)
        near[act] |= lv & (np.abs((F(1) - Tn) - F(0.99)) < F(2e-5))
        stop = lv & ((F(1) - Tn) >= F(0.99))
        T[act] = Tn
        live[act] &= ~stop
        tt, pp = np.nonzero(take)
        steps.append((flat[act][tt, pp], s[tt], stop[tt, pp]))
        alphas.append(g[tt, pp])

    def scatter(a):
        img = np.zeros((height, width), bool)
        img[py[inimg], px[inimg]] = a[inimg]
        return img
    return dict(steps=steps, alpha=alphas, rim=scatter(rim), near=scatter(near))


def composite64(rec, col, steps, width, height, pixels=None):
    """(rgb (H W, 3), alpha (H W)) float64 over the recorded pairs, differentiable in rec (n, 8) and col (n, 4).  pixels (sorted
    flat pixel indices y W + x, optional): only those pixels, in that order — every pixel of `steps` must be one of them."""
    flat = torch.arange(width * height) if pixels is None else torch.as_tensor(np.asarray(pixels, np.int64))
    P = flat.shape[0]
    pix_x = (flat % width).to(D) + 0.5
    pix_y = torch.div(flat, width, rounding_mode="floor").to(D) + 0.5
    T = torch.ones(P, dtype=D)
    C = torch.zeros((P, 3), dtype=D)
    for pix, s, _stop in steps:
        if pix.size == 0:
            continue
        if pixels is not None:
            pix = np.searchsorted(np.asarray(pixels, np.int64), pix)
        pix_t, s_t = torch.as_tensor(pix, dtype=torch.long), torch.as_tensor(s, dtype=torch.long)
        r = rec[s_t]
        dx, dy = pix_x[pix_t] - r[:, 0], pix_y[pix_t] - r[:, 1]
        u = r[:, 2] * dx + r[:, 3] * dy
        v = r[:, 4] * dx + r[:, 5] * dy
        a = col[s_t, 3] * torch.exp(-4.5 * (u * u + v * v))
        Tp = T[pix_t]
        C = C.index_add(0, pix_t, (Tp * a)[:, None] * col[s_t, :3])
        T = T.index_put((pix_t,), Tp * (1 - a))
    rgb = C + T[:, None] * torch.tensor(BG, dtype=D)[None, :]
    return rgb, 1 - T


def upstream(width, height, rim, near, seed):
    """Random dL/d(rgb, alpha) in [-1, 1], zero on the rim and near pixels: (H, W, 4) float32."""
    rng = np.random.default_rng(seed)
    g = rng.uniform(-1, 1, (height, width, 4)).astype(F)
    g[rim | near] = 0
    return g


def composite_grads(rec32, col32, steps, width, height, g, pixels=None):
    """dL/drec (n, 8) and dL/dcol (n, 4) of L = sum g . (rgb, alpha), by autograd over composite64 (pixels: as there; g is zero
    at every other pixel)."""
    rec = torch.tensor(np.asarray(rec32, np.float64), requires_grad=True)
    col = torch.tensor(np.asarray(col32, np.float64), requires_grad=True)
    rgb, alpha = composite64(rec, col, steps, width, height, pixels)
    gt = torch.as_tensor(np.asarray(g, np.float64).reshape(-1, 4))
    if pixels is not None:
        gt = gt[torch.as_tensor(np.asarray(pixels, np.int64))]
    ((rgb * gt[:, :3]).sum() + (alpha * gt[:, 3]).sum()).backward()
    return rec.grad.numpy(), col.grad.numpy()
