"""Restatements of the 2D Gaussian surfel footprint (SPLAT_FOOTPRINT_SURFEL, include/splat.h "2D Gaussian surfels").

records() / project(): the projector in NumPy binary32, one rounding per operation in csrc/surfel.h's order, so records,
ProjectedSplats, keys and the centres' clip w compare bit for bit.  composite(): the per-pixel blend over given lists in binary32
with the whole record, (u, v) = B d / (1 - q.d), in the shape of ellipsoid_ref.composite / ellipsoid_grad_ref.decisions: image,
alpha, the intersection depth map, the rim / near masks and the recorded (pixel, splat) pairs.  records64() / composite64(): the
same functions in torch float64 between those decisions, for torch.autograd — independent of the kernels' hand-derived formulas.
"""
import numpy as np
import torch

from oracle import np_oracle as NO

F = np.float32
D = torch.float64
BG = (0.05, 0.05, 0.1)


def _v4(a):
    a = np.asarray(a, F)
    return np.concatenate([a, np.zeros((a.shape[0], 1), F)], axis=1) if a.shape[1] == 3 else a


def records(u, pos, scl, rot):
    """((n, 8) float32 records, all zeros when culled; (n,) float32 clip w of the centres, 0 when culled), as surfel_record()."""
    m = np.asarray(u, F)
    p, s, q = (_v4(a) for a in (pos, scl, rot))
    with np.errstate(all="ignore"):
        n2 = ((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2]) + q[:, 3] * q[:, 3]
        k = F(1) / np.sqrt(n2)
        qr, qx, qy, qz = q[:, 0] * k, q[:, 1] * k, q[:, 2] * k, q[:, 3] * k
        one, two = F(1), F(2)
        r0 = [one - two * (qy * qy + qz * qz), two * (qx * qy + qr * qz), two * (qx * qz - qr * qy)]
        r1 = [two * (qx * qy - qr * qz), one - two * (qx * qx + qz * qz), two * (qy * qz + qr * qx)]
        a0, a1 = F(3) * s[:, 0], F(3) * s[:, 1]
        e0 = [c * a0 for c in r0]
        e1 = [c * a1 for c in r1]

        def lin(row, e):
            return (m[row] * e[0] + m[4 + row] * e[1]) + m[8 + row] * e[2]

        ctx, cty, ctw = lin(0, e0), lin(1, e0), lin(3, e0)
        cbx, cby, cbw = lin(0, e1), lin(1, e1), lin(3, e1)
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        cpx = ((m[0] * x + m[4] * y) + m[8] * z) + m[12]
        cpy = ((m[1] * x + m[5] * y) + m[9] * z) + m[13]
        cpw = ((m[3] * x + m[7] * y) + m[11] * z) + m[15]
        front = (cpw - (np.abs(ctw) + np.abs(cbw))) > F(0)
        hw, hh = F(0.5) * m[20], F(0.5) * m[21]
        m00, m01, m02 = hw * (ctx + ctw), hw * (cbx + cbw), hw * (cpx + cpw)
        m10, m11, m12 = hh * (ctw - cty), hh * (cbw - cby), hh * (cpw - cpy)
        icw = F(1) / cpw
        scx, scy = m02 * icw, m12 * icw
        a00, a01 = m00 - scx * ctw, m01 - scx * cbw
        a10, a11 = m10 - scy * ctw, m11 - scy * cbw
        det = a00 * a11 - a01 * a10
        ok = front & (np.abs(det) > F(0))
        idet = F(1) / det
        kk = cpw * idet
        rec = np.stack([scx, scy, a11 * kk, (-a01) * kk, (-a10) * kk, a00 * kk,
                        (a11 * ctw - a10 * cbw) * idet, (a00 * cbw - a01 * ctw) * idet], axis=1).astype(F)
        ok &= np.isfinite(rec).all(axis=1)
    rec[~ok] = 0
    return rec, np.where(ok, cpw, F(0)).astype(F)


def project(u, pos, scl, rot):
    """records, ProjectedSplat records (n, 8), depth keys and clip w, as splat_project_surfel writes them."""
    rec, cw = records(u, pos, scl, rot)
    bnd, _ = NO.disc_bounds(rec)
    p = _v4(pos)
    u = np.asarray(u, F)
    with np.errstate(all="ignore"):
        dx, dy, dz = p[:, 0] - u[16], p[:, 1] - u[17], p[:, 2] - u[18]
        depth = np.sqrt((dx * dx + dy * dy) + dz * dz)
    proj = np.zeros((rec.shape[0], 8), F)
    proj[:, :4] = bnd
    proj[:, 4] = depth
    proj[:, 5] = F(0.5) * np.fmax(bnd[:, 2] - bnd[:, 0], bnd[:, 3] - bnd[:, 1])
    proj[:, 6] = np.arange(rec.shape[0], dtype=np.uint32).view(F)
    keys, _ = NO.extract_keys(proj)
    return rec, proj, keys, cw


def lists(u, pos, scl, rot, w, h):
    """(rec, cw, counts, offsets, idx): the frame's records and its 16 x 16 tile lists, by the oracle's sort and binner."""
    rec, proj, keys, cw = project(u, pos, scl, rot)
    _, order = NO.sort_pairs(keys, np.arange(keys.shape[0], dtype=np.uint32))
    counts, offsets, idx = NO.bin_sorted(proj, order, w, h, 16)
    return rec, cw, counts, offsets, idx


def geometry64(u, pos, scl, rot):
    """float64 pieces of every surfel: dict(e0, e1 (n, 3) half-axes, cw (n,) clip w of the centre, persp (n,) = hypot(ctw, cbw) / cw,
    cond (n,) the condition number of the quad's 2 x 2 screen Jacobian)."""
    m = np.asarray(u, np.float64)
    p, s, q = (np.asarray(_v4(a), np.float64) for a in (pos, scl, rot))
    with np.errstate(all="ignore"):
        q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
        r, x, y, z = q.T
        R0 = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)], 1)
        R1 = np.stack([2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)], 1)
        e0, e1 = 3 * s[:, 0:1] * R0, 3 * s[:, 1:2] * R1
        rows = m[:16].reshape(4, 4).T  # rows[r] = row r of VP
        ct, cb = e0 @ rows[:, :3].T, e1 @ rows[:, :3].T
        cp = p[:, :3] @ rows[:, :3].T + rows[:, 3]
        hw, hh = 0.5 * m[20], 0.5 * m[21]
        scx, scy = hw * (cp[:, 0] + cp[:, 3]) / cp[:, 3], hh * (cp[:, 3] - cp[:, 1]) / cp[:, 3]
        A = np.stack([np.stack([hw * (ct[:, 0] + ct[:, 3]) - scx * ct[:, 3], hw * (cb[:, 0] + cb[:, 3]) - scx * cb[:, 3]], 1),
                      np.stack([hh * (ct[:, 3] - ct[:, 1]) - scy * ct[:, 3], hh * (cb[:, 3] - cb[:, 1]) - scy * cb[:, 3]], 1)], 1)
        A = np.where(np.isfinite(A), A, 0.0)
        sv = np.linalg.svd(A, compute_uv=False)
        cond = np.where(sv[:, 1] > 0, sv[:, 0] / np.where(sv[:, 1] > 0, sv[:, 1], 1), np.inf)
        persp = np.hypot(ct[:, 3], cb[:, 3]) / cp[:, 3]
    return dict(e0=e0, e1=e1, cw=cp[:, 3], persp=persp, cond=cond, centre=np.stack([scx, scy], 1))


def records64(u, pos, scl, rot, keep):
    """((n, 8) float64 records of the surfels in `keep` (zeros elsewhere), (n,) clip w), differentiable in pos, scl, rot."""
    m = [float(x) for x in np.asarray(u, np.float64)]
    n = pos.shape[0]
    idx = torch.as_tensor(np.nonzero(np.asarray(keep))[0], dtype=torch.long)
    p, s, q = pos[idx, :3], scl[idx, :2], rot[idx]
    q = q / torch.sqrt((q * q).sum(dim=1, keepdim=True))
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R0 = [1 - 2 * (y * y + z * z), 2 * (x * y + r * z), 2 * (x * z - r * y)]
    R1 = [2 * (x * y - r * z), 1 - 2 * (x * x + z * z), 2 * (y * z + r * x)]
    e0 = [3 * s[:, 0] * c for c in R0]
    e1 = [3 * s[:, 1] * c for c in R1]

    def lin(row, e):
        return m[row] * e[0] + m[4 + row] * e[1] + m[8 + row] * e[2]

    ctx, cty, ctw = lin(0, e0), lin(1, e0), lin(3, e0)
    cbx, cby, cbw = lin(0, e1), lin(1, e1), lin(3, e1)
    P = [p[:, 0], p[:, 1], p[:, 2]]
    cpx, cpy, cpw = lin(0, P) + m[12], lin(1, P) + m[13], lin(3, P) + m[15]
    hw, hh = 0.5 * m[20], 0.5 * m[21]
    scx, scy = hw * (cpx + cpw) / cpw, hh * (cpw - cpy) / cpw
    a00, a01 = hw * (ctx + ctw) - scx * ctw, hw * (cbx + cbw) - scx * cbw
    a10, a11 = hh * (ctw - cty) - scy * ctw, hh * (cbw - cby) - scy * cbw
    det = a00 * a11 - a01 * a10
    k = cpw / det
    vals = torch.stack([scx, scy, a11 * k, -a01 * k, -a10 * k, a00 * k, (a11 * ctw - a10 * cbw) / det, (a00 * cbw - a01 * ctw) / det], dim=1)
    return torch.zeros((n, 8), dtype=D).index_put((idx,), vals), torch.zeros(n, dtype=D).index_put((idx,), cpw)


def composite(rec, color_opacity, z, indices, counts, offsets, width, height, tile=16):
    """The binary32 frame over the given lists, in ellipsoid_ref.composite's loop with the whole record: dict(img (H, W, 4),
    alpha, depth (H, W) float64 = sum w z rd / sum w or +inf, rim, near (H, W) bool, steps [(pixel, splat, stop) per list
    position]).  rim: |d2 - 1| <= 1e-3 at some entry (the cut is a step of opacity e^-4.5); near: 1 - T within 2e-5 of 0.99 at
    some entry (the stop may move by one entry)."""
    rec = np.asarray(rec, F)
    col = np.asarray(color_opacity, F)
    z = np.asarray(z, F)
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
    C = np.zeros(shape + (3,), F)
    live = inimg.copy()
    rim = np.zeros(shape, bool)
    near = np.zeros(shape, bool)
    zw, ws = np.zeros(shape), np.zeros(shape)
    steps = []
    cnt, off = counts.astype(np.int64), offsets.astype(np.int64)
    for i in range(int(cnt.max()) if cnt.size else 0):
        act = np.nonzero((cnt > i) & live.any(axis=1))[0]
        if act.size == 0:
            break
        s = indices[off[act] + i].astype(np.int64)
        r, b = rec[s], bnd[s]
        dx, dy = pxf[act] - r[:, 0:1], pyf[act] - r[:, 1:2]
        with np.errstate(all="ignore"):
            rd = F(1) / (F(1) - (r[:, 6:7] * dx + r[:, 7:8] * dy))
            uu, vv = (r[:, 2:3] * dx + r[:, 3:4] * dy) * rd, (r[:, 4:5] * dx + r[:, 5:6] * dy) * rd
            d2 = uu * uu + vv * vv
            g = (col[s, 3:4] * np.exp(F(-4.5) * d2)).astype(F)
        inside = ~((pxf[act] < b[:, 0:1]) | (pxf[act] > b[:, 2:3]) | (pyf[act] < b[:, 1:2]) | (pyf[act] > b[:, 3:4]))
        lv = live[act]
        rim[act] |= lv & okb[s][:, None] & (np.abs(d2 - F(1)) <= F(1e-3))
        take = lv & okb[s][:, None] & inside & (d2 <= F(1))
        g = np.where(take, g, F(0))
        Ta = T[act]
        w = Ta * g
        C[act] += w[..., None] * col[s, None, :3]
        Tn = (Ta * (F(1) - g)).astype(F)
        near[act] |= lv & (np.abs((F(1) - Tn) - F(0.99)) < F(2e-5))
        zw[act] += np.where(take, w.astype(np.float64) * z[s][:, None] * np.where(take, rd, 0), 0.0)
        ws[act] += w
        stop = lv & ((F(1) - Tn) >= F(0.99))
        T[act] = Tn
        live[act] &= ~stop
        tt, pp = np.nonzero(take)
        steps.append((flat[act][tt, pp], s[tt], stop[tt, pp]))

    def scatter(a, fill, dtype, extra=()):
        img = np.full((height, width) + extra, fill, dtype)
        img[py[inimg], px[inimg]] = a[inimg]
        return img
    rgb = C + T[..., None] * np.asarray(BG, F)[None, None, :]
    img = np.concatenate([rgb, np.ones(shape + (1,), F)], axis=-1).astype(F)
    with np.errstate(all="ignore"):
        depth = np.where(ws > 0, zw / np.where(ws > 0, ws, 1), np.inf)
    return dict(img=scatter(img, 0, F, (4,)), alpha=scatter((F(1) - T).astype(F), 0, F), depth=scatter(depth, np.inf, np.float64),
                rim=scatter(rim, False, bool), near=scatter(near, False, bool), steps=steps)


def composite64(rec, col, steps, width, height, z=None, feats=None, pairs=None):
    """float64 over the recorded pairs, differentiable in rec (n, 8), col (n, 4), z (n,) and feats (n, K): dict(rgb (H W, 3),
    alpha (H W), zw, ws (H W): depth = zw / ws where ws > 0; feat (H W, K)).  The arithmetic is rec's dtype: float32 tensors
    make it the binary32 restatement of the same formulas that the feature tests take their error constants from.  pairs (a list):
    receives per step (splat indices, the gathered record rows, opacities and feature rows with their gradients retained), so that
    after backward() each row's .grad is that (pixel, splat) pair's own term of the splat's gradient."""
    D = rec.dtype
    P = width * height
    flat = torch.arange(P)
    pix_x = (flat % width).to(D) + 0.5
    pix_y = torch.div(flat, width, rounding_mode="floor").to(D) + 0.5
    T = torch.ones(P, dtype=D)
    C = torch.zeros((P, 3), dtype=D)
    zw, ws = torch.zeros(P, dtype=D), torch.zeros(P, dtype=D)
    Fm = torch.zeros((P, feats.shape[1]), dtype=D) if feats is not None else None
    for pix, s, _stop in steps:
        if pix.size == 0:
            continue
        pix_t, s_t = torch.as_tensor(pix, dtype=torch.long), torch.as_tensor(s, dtype=torch.long)
        r = rec[s_t]
        op = col[s_t, 3]
        fr = feats[s_t] if feats is not None else None
        if pairs is not None:
            for t in (r, op, fr):
                t.retain_grad()
            pairs.append((s_t, r, op, fr))
        dx, dy = pix_x[pix_t] - r[:, 0], pix_y[pix_t] - r[:, 1]
        rd = 1 / (1 - (r[:, 6] * dx + r[:, 7] * dy))
        u = (r[:, 2] * dx + r[:, 3] * dy) * rd
        v = (r[:, 4] * dx + r[:, 5] * dy) * rd
        a = op * torch.exp(-4.5 * (u * u + v * v))
        Tp = T[pix_t]
        w = Tp * a
        C = C.index_add(0, pix_t, w[:, None] * col[s_t, :3])
        ws = ws.index_add(0, pix_t, w)
        if z is not None:
            zw = zw.index_add(0, pix_t, w * z[s_t] * rd)
        if feats is not None:
            Fm = Fm.index_add(0, pix_t, w[:, None] * fr)
        T = T.index_put((pix_t,), Tp * (1 - a))
    rgb = C + T[:, None] * torch.tensor(BG, dtype=D)[None, :]
    return dict(rgb=rgb, alpha=1 - T, zw=zw, ws=ws, feat=Fm)


def loss64(out, g, gd=None, gf=None):
    """sum g . (rgb, alpha) [+ sum gd depth over the pixels something contributed to] [+ sum gf . feat]: the scalar the GPU tests'
    upstreams are the gradient of.  g (H, W, 4), gd (H, W), gf (H, W, K)."""
    D = out["rgb"].dtype
    gt = torch.as_tensor(np.asarray(g, np.float64).reshape(-1, 4)).to(D)
    L = (out["rgb"] * gt[:, :3]).sum() + (out["alpha"] * gt[:, 3]).sum()
    if gd is not None:
        has = out["ws"].detach() > 0
        depth = out["zw"][has] / out["ws"][has]
        L = L + (depth * torch.as_tensor(np.asarray(gd, np.float64).reshape(-1)).to(D)[has]).sum()
    if gf is not None:
        L = L + (out["feat"] * torch.as_tensor(np.asarray(gf, np.float64).reshape(out["feat"].shape)).to(D)).sum()
    return L


def composite_grads(rec32, col32, steps, width, height, g, z32=None, gd=None):
    """dL/drec (n, 8), dL/dcol (n, 4) [, dL/dz (n,)] of loss64, by autograd over composite64."""
    rec = torch.tensor(np.asarray(rec32, np.float64), requires_grad=True)
    col = torch.tensor(np.asarray(col32, np.float64), requires_grad=True)
    z = torch.tensor(np.asarray(z32, np.float64), requires_grad=True) if z32 is not None else None
    loss64(composite64(rec, col, steps, width, height, z), g, gd).backward()
    out = (rec.grad.numpy(), col.grad.numpy())
    return out if z is None else out + (z.grad.numpy() if z.grad is not None else np.zeros(rec.shape[0]),)


def feature_maps(rec32, col32, feats32, steps, width, height, dtype=torch.float64):
    """(F (H W, K), m_px (H W, K) = sum w |f|) of the feature map over the recorded pairs, in `dtype` arithmetic."""
    rec, col = (torch.tensor(np.asarray(a, np.float64)).to(dtype) for a in (rec32, col32))
    f = torch.tensor(np.asarray(feats32, np.float64)).to(dtype)
    with torch.no_grad():
        F_ = composite64(rec, col, steps, width, height, feats=f)["feat"]
        m = composite64(rec, col, steps, width, height, feats=f.abs())["feat"]
    return F_.to(torch.float64).numpy(), m.to(torch.float64).numpy()


def feature_grads(rec32, col32, feats32, steps, width, height, gf, dtype=torch.float64, magnitudes=False):
    """(n, 9 + K) sums of L = sum gf . feat in the order {the eight record columns, opacity, the K feature columns}, by autograd
    over composite64 in `dtype`.  magnitudes=True: also m (n, 9 + K), per splat and number the sum over its pairs of |the pair's
    term| (test_gpu_features.py's m: what an error of a sum of signed terms is measured in)."""
    rec = torch.tensor(np.asarray(rec32, np.float64)).to(dtype).requires_grad_()
    col = torch.tensor(np.asarray(col32, np.float64)).to(dtype).requires_grad_()
    f = torch.tensor(np.asarray(feats32, np.float64)).to(dtype).requires_grad_()
    pairs = [] if magnitudes else None
    out = composite64(rec, col, steps, width, height, feats=f, pairs=pairs)
    (out["feat"] * torch.as_tensor(np.asarray(gf, np.float64).reshape(out["feat"].shape)).to(dtype)).sum().backward()
    sums = torch.cat([rec.grad, col.grad[:, 3:4], f.grad], dim=1).to(torch.float64).numpy()
    if not magnitudes:
        return sums
    m = torch.zeros(sums.shape, dtype=torch.float64)
    for s_t, r, op, fr in pairs:
        m = m.index_add(0, s_t, torch.cat([r.grad, op.grad[:, None], fr.grad], dim=1).abs().to(torch.float64))
    return sums, m.numpy()
