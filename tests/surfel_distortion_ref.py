"""Restatements of the surfel frame's depth-distortion map (include/splat.h, "Depth distortion"; csrc/surfel.h states the order).

distortion32(): the map in NumPy binary32 over surfel_ref.composite's recorded steps, one rounding per operator in csrc/surfel.h's
order: m'_i = c (1 / t_first - 1 / t_i), Dist += w (m'^2 A + Q - 2 m' M), A += w, M += w m', Q += w m'^2.  shifted=False is the same
prefix form over the plain m_i = far (t_i - near) / ((far - near) t_i): what cancels, kept to show that the bound tells them apart.
composite64(): surfel_ref.composite64's loop in torch (float64, or float32 tensors for a binary32 restatement of the same
formulas) with Dist the plain pairwise sum over each pixel's participating entries, differentiable in rec, col and z by autograd:
independent of the kernels' hand-derived formulas.  pixel_grads(): those formulas for one pixel in NumPy float64.
"""
import numpy as np
import torch

from tests import surfel_ref as SR

F = np.float32


def constant(near, far):
    """c of csrc/surfel.h as binary32: near when far = +inf, else near far / (far - near) formed in binary64 and rounded once."""
    near, far = float(F(near)), float(F(far))
    return F(near) if np.isinf(far) else F(near * far / (far - near))


def distortion32(rec, color_opacity, z, steps, width, height, near, far, shifted=True):
    """(H, W) float32 map over the recorded steps (each a (pixels, splats, stop) of entries inside the cut, front to back)."""
    rec, col, z = np.asarray(rec, F), np.asarray(color_opacity, F), np.asarray(z, F)
    c = constant(near, far)
    nearf, farf = F(near), F(far)
    P = width * height
    flat = np.arange(P)
    pxf, pyf = (flat % width).astype(F) + F(0.5), (flat // width).astype(F) + F(0.5)
    T = np.ones(P, F)
    dist, A, M, Q = (np.zeros(P, F) for _ in range(4))
    rt0 = np.full(P, -1, F)
    for pix, s, _stop in steps:
        if pix.size == 0:
            continue
        r = rec[s]
        dx, dy = pxf[pix] - r[:, 0], pyf[pix] - r[:, 1]
        with np.errstate(all="ignore"):
            rd = F(1) / (F(1) - (r[:, 6] * dx + r[:, 7] * dy))
            uu, vv = (r[:, 2] * dx + r[:, 3] * dy) * rd, (r[:, 4] * dx + r[:, 5] * dy) * rd
            g = (col[s, 3] * np.exp(F(-4.5) * (uu * uu + vv * vv))).astype(F)
            w = T[pix] * g
            T[pix] = (T[pix] * (F(1) - g)).astype(F)
            t = z[s] * rd
            part = (t > 0) & np.isfinite(t)
            pix, w, t = pix[part], w[part], t[part]
            if shifted:
                rt = F(1) / t
                first = rt0[pix] < 0
                rt0[pix[first]] = rt[first]
                mp = c * (rt0[pix] - rt)
            else:
                mp = (F(1) - nearf / t) if np.isinf(farf) else (farf * (t - nearf)) / ((farf - nearf) * t)
            mm = mp * mp
            d = (mm * A[pix] + Q[pix]) - (F(2) * mp) * M[pix]
            dist[pix] = dist[pix] + w * d
            A[pix] = A[pix] + w
            M[pix] = M[pix] + w * mp
            Q[pix] = Q[pix] + w * mm
    assert dist.dtype == F
    return dist.reshape(height, width)


def composite64(rec, col, z, steps, width, height, near, far):
    """surfel_ref.composite64's dict(rgb, alpha, zw, ws) and dist (H W): the pairwise sum_{i > j} w_i w_j (m_i - m_j)^2 with
    m = far (t - near) / ((far - near) t), t = z rd, over the entries whose t is finite and > 0.  The arithmetic is rec's dtype."""
    D = rec.dtype
    P = width * height
    flat = torch.arange(P)
    pix_x = (flat % width).to(D) + 0.5
    pix_y = torch.div(flat, width, rounding_mode="floor").to(D) + 0.5
    T = torch.ones(P, dtype=D)
    C = torch.zeros((P, 3), dtype=D)
    zw, ws = torch.zeros(P, dtype=D), torch.zeros(P, dtype=D)
    rank = np.zeros(P, np.int64)  # participating entries so far, per pixel
    slots, ws_all, ms_all = [], [], []
    for pix, s, _stop in steps:
        if pix.size == 0:
            continue
        pix_t, s_t = torch.as_tensor(pix, dtype=torch.long), torch.as_tensor(s, dtype=torch.long)
        r = rec[s_t]
        op = col[s_t, 3]
        dx, dy = pix_x[pix_t] - r[:, 0], pix_y[pix_t] - r[:, 1]
        rd = 1 / (1 - (r[:, 6] * dx + r[:, 7] * dy))
        u = (r[:, 2] * dx + r[:, 3] * dy) * rd
        v = (r[:, 4] * dx + r[:, 5] * dy) * rd
        a = op * torch.exp(-4.5 * (u * u + v * v))
        Tp = T[pix_t]
        w = Tp * a
        C = C.index_add(0, pix_t, w[:, None] * col[s_t, :3])
        ws = ws.index_add(0, pix_t, w)
        t = z[s_t] * rd
        zw = zw.index_add(0, pix_t, w * t)
        T = T.index_put((pix_t,), Tp * (1 - a))
        part = ((t.detach() > 0) & torch.isfinite(t.detach())).numpy()
        if part.any():
            pp = torch.as_tensor(part)
            tp = t[pp]
            m = (1 - near / tp) if np.isinf(far) else far * (tp - near) / ((far - near) * tp)
            slots.append((pix[part], rank[pix[part]].copy()))
            rank[pix[part]] += 1
            ws_all.append(w[pp])
            ms_all.append(m)
    rgb = C + T[:, None] * torch.tensor(SR.BG, dtype=D)[None, :]
    dist = torch.zeros(P, dtype=D)
    if ws_all:
        L = int(rank.max())
        where = torch.as_tensor(np.concatenate([p * L + k for p, k in slots]), dtype=torch.long)
        Wm = torch.zeros(P * L, dtype=D).index_put((where,), torch.cat(ws_all)).reshape(P, L)  # (a padded slot: w = 0)
        Mm = torch.zeros(P * L, dtype=D).index_put((where,), torch.cat(ms_all)).reshape(P, L)
        for k in range(1, L):  # the pairs k list positions apart
            dist = dist + (Wm[:, k:] * Wm[:, :-k] * (Mm[:, k:] - Mm[:, :-k]) ** 2).sum(dim=1)
    return dict(rgb=rgb, alpha=1 - T, zw=zw, ws=ws, dist=dist)


def loss64(out, g, gd=None, gdist=None):
    """surfel_ref.loss64 [+ sum gdist dist]."""
    L = SR.loss64(out, g, gd)
    if gdist is not None:
        L = L + (out["dist"] * torch.as_tensor(np.asarray(gdist, np.float64).reshape(-1)).to(out["dist"].dtype)).sum()
    return L


def maps(rec32, col32, z32, steps, width, height, near, far):
    """float64 (depth (H, W), +inf where nothing contributed; dist (H, W))."""
    with torch.no_grad():
        out = composite64(*(torch.tensor(np.asarray(a, np.float64)) for a in (rec32, col32, z32)), steps, width, height, near, far)
    ws, zw = out["ws"].numpy(), out["zw"].numpy()
    depth = np.where(ws > 0, zw / np.where(ws > 0, ws, 1), np.inf)
    return depth.reshape(height, width), out["dist"].numpy().reshape(height, width)


def composite_grads(rec32, col32, z32, steps, width, height, near, far, g, gd, gdist, dtype=torch.float64):
    """(dL/drec (n, 8), dL/dcol (n, 4), dL/dz (n,)) of loss64 as float64 arrays, by autograd over composite64 in `dtype`."""
    rec, col, z = (torch.tensor(np.asarray(a, np.float64)).to(dtype).requires_grad_() for a in (rec32, col32, z32))
    loss64(composite64(rec, col, z, steps, width, height, near, far), g, gd, gdist).backward()
    return tuple((a.grad if a.grad is not None else torch.zeros_like(a)).to(torch.float64).numpy() for a in (rec, col, z))


def pixel_grads(alpha, t, near, far):
    """The backward's formulas for one pixel (include/splat.h) in float64: (Dist, dDist/dalpha_i, dDist/dt_i) of entries front to
    back with alphas `alpha` and depths `t`, all participating.  Through the weights Dist is a colour channel of per-entry colour
    e_i = W (m'_i - M / W)^2 + Dist / W and background 0, swept back to front as the kernel's second walk does (S = alpha cg +
    (1 - alpha) S, dL/dalpha_i = T_i (cg_i - S)); through m_i, dDist/dt_i = 2 w_i (m'_i W - M) c / t_i^2."""
    alpha, t = np.asarray(alpha, np.float64), np.asarray(t, np.float64)
    c = near if np.isinf(far) else near * far / (far - near)
    T = np.concatenate([[1.0], np.cumprod(1 - alpha)[:-1]])
    w = T * alpha
    mp = c * (1 / t[0] - 1 / t)
    dist = A = M = Q = 0.0
    for wi, mi in zip(w, mp):
        dist += wi * (mi * mi * A + Q - 2 * mi * M)
        A, M, Q = A + wi, M + wi * mi, Q + wi * mi * mi
    e = A * (mp - M / A) ** 2 + dist / A
    galpha = np.zeros_like(alpha)
    S = 0.0
    for i in range(len(alpha) - 1, -1, -1):
        galpha[i] = T[i] * (e[i] - S)
        S = alpha[i] * e[i] + (1 - alpha[i]) * S
    gt = 2 * w * (mp * A - M) * c / (t * t)
    return dist, galpha, gt
