"""A NumPy restatement of the anisotropic Gaussian footprint (SPLAT_FOOTPRINT_ELLIPSOID, include/splat.h).

project(): the projector in binary32, one rounding per operation in csrc/ellipsoid.h's order, so records, ProjectedSplats and
keys compare bit for bit.  sh_colors(): splat_sh_colors in float64 (the contract) or float32.  composite(): the per-pixel
blend over the oracle's lists in the shape of aov_ref._disc_g — alpha = opacity exp(-4.5 d2) inside d2 = |B d|^2 <= 1 and the
record's bounds, nearest on top, the early-out, the background (0.05, 0.05, 0.1) — with the pixels where the kernel's rounding
may decide differently marked: rim (|d2 - 1| <= 1e-3 at some entry: the cut is a step of opacity e^-4.5 ~ 0.011) and near
(1 - T within 2e-5 of 0.99 at some entry: the stop may move by one entry).
"""
import numpy as np

from oracle import np_oracle as NO

F = np.float32
BG = np.array([0.05, 0.05, 0.1], F)
SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
SH_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658,
         1.445305721320277, -0.5900435899266435]


def _v4(a):
    """(n, 3) or (n, 4) -> (n, 4) float32 (a zero fourth column added)."""
    a = np.asarray(a, F)
    return np.concatenate([a, np.zeros((a.shape[0], 1), F)], axis=1) if a.shape[1] == 3 else a


def records(u, pos, scl, rot):
    """(n, 8) float32 records {c.x, c.y, B00, B01, 0, B11, 0, 0} (all zeros when culled), as ellipsoid_record()."""
    m = np.asarray(u, F)
    p, s, q = (_v4(a) for a in (pos, scl, rot))
    n = p.shape[0]
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
        v = [(m[3] * M[0][j] + m[7] * M[1][j]) + m[11] * M[2][j] for j in range(3)]
        reach = cw - F(3) * np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        nx, ny = cx / cw, cy / cw
        scx, scy = ((nx + F(1)) * F(0.5)) * m[20], ((F(1) - ny) * F(0.5)) * m[21]
        icw = F(1) / cw
        ax, ay = (F(0.5) * m[20]) * icw, (F(0.5) * m[21]) * icw
        j0 = [ax * (m[0] - nx * m[3]), ax * (m[4] - nx * m[7]), ax * (m[8] - nx * m[11])]
        j1 = [ay * (ny * m[3] - m[1]), ay * (ny * m[7] - m[5]), ay * (ny * m[11] - m[9])]
        t0 = [(j0[0] * M[0][c] + j0[1] * M[1][c]) + j0[2] * M[2][c] for c in range(3)]
        t1 = [(j1[0] * M[0][c] + j1[1] * M[1][c]) + j1[2] * M[2][c] for c in range(3)]
        a = ((t0[0] * t0[0] + t0[1] * t0[1]) + t0[2] * t0[2]) + F(0.3)
        b = (t0[0] * t1[0] + t0[1] * t1[1]) + t0[2] * t1[2]
        c = ((t1[0] * t1[0] + t1[1] * t1[1]) + t1[2] * t1[2]) + F(0.3)
        det = a * c - b * b
        b00 = np.sqrt(c / det) / F(3)
        b01 = ((-b) / np.sqrt(c * det)) / F(3)
        b11 = (F(1) / np.sqrt(c)) / F(3)
    out = np.zeros((n, 8), F)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3], out[:, 5] = scx, scy, b00, b01, b11
    ok = (cw > 0) & (reach > 0) & (det > 0) & np.isfinite(out).all(axis=1) & np.isfinite(det)
    out[~ok] = 0
    return out


def project(u, pos, scl, rot):
    """records, ProjectedSplat records (n, 8) and depth keys, as splat_project_ellipsoid writes them."""
    rec = records(u, pos, scl, rot)
    bnd, _ = NO.disc_bounds(rec)
    p = _v4(pos)
    u = np.asarray(u, F)
    dx, dy, dz = p[:, 0] - u[16], p[:, 1] - u[17], p[:, 2] - u[18]
    depth = np.sqrt((dx * dx + dy * dy) + dz * dz)
    proj = np.zeros((rec.shape[0], 8), F)
    proj[:, :4] = bnd
    proj[:, 4] = depth
    proj[:, 5] = F(0.5) * np.fmax(bnd[:, 2] - bnd[:, 0], bnd[:, 3] - bnd[:, 1])
    proj[:, 6] = np.arange(rec.shape[0], dtype=np.uint32).view(F)
    keys, _ = NO.extract_keys(proj)
    return rec, proj, keys


def sh_basis(d, degree, dtype=np.float64):
    """(n, (degree + 1)^2) real SH basis values of 3DGS's eval_sh at unit directions d (n, 3)."""
    d = np.asarray(d, dtype)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    c = lambda v: dtype(v)  # noqa: E731
    Y = [np.full(x.shape, c(SH_C0), dtype)]
    if degree > 0:
        Y += [-c(SH_C1) * y, c(SH_C1) * z, -c(SH_C1) * x]
    if degree > 1:
        xx, yy, zz = x * x, y * y, z * z
        Y += [c(SH_C2[0]) * (x * y), c(SH_C2[1]) * (y * z), c(SH_C2[2]) * ((c(2) * zz - xx) - yy), c(SH_C2[3]) * (x * z),
              c(SH_C2[4]) * (xx - yy)]
        if degree > 2:
            Y += [c(SH_C3[0]) * (y * (c(3) * xx - yy)), c(SH_C3[1]) * ((x * y) * z), c(SH_C3[2]) * (y * ((c(4) * zz - xx) - yy)),
                  c(SH_C3[3]) * (z * ((c(2) * zz - c(3) * xx) - c(3) * yy)), c(SH_C3[4]) * (x * ((c(4) * zz - xx) - yy)),
                  c(SH_C3[5]) * (z * (xx - yy)), c(SH_C3[6]) * (x * (xx - c(3) * yy))]
    return np.stack(Y, axis=1)


def has_direction(eye, pos):
    """(n,) bool, the kernels' binary32 decision: |p - eye| is a positive finite number.  Where it is not (a splat at the eye,
    a position that is not finite), the direction is (0, 0, 0)."""
    p = np.asarray(pos, F)[:, :3]
    e = np.asarray(eye, F).reshape(-1)[:3]
    with np.errstate(all="ignore"):
        x, y, z = p[:, 0] - e[0], p[:, 1] - e[1], p[:, 2] - e[2]
        ln = np.sqrt((x * x + y * y) + z * z)
        return (ln > 0) & (ln < np.inf)


def sh_colors(eye, pos, sh, degree, opacity, dtype=np.float64):
    """(n, 4): max(0.5 + sum_k Y_k(normalize(p - eye)) sh_k, 0), opacity.  sh: (n, K, 3) basis-major.  A splat without a
    direction (has_direction) takes (0, 0, 0) for it: max(0.5 + C0 sh_0, 0)."""
    p = np.asarray(pos, dtype)[:, :3]
    ok = has_direction(eye, pos)[:, None]
    d = np.where(ok, p - np.asarray(eye, dtype)[None, :3], dtype(1))
    d = np.where(ok, d / np.sqrt((d * d).sum(axis=1, keepdims=True)), dtype(0))
    nb = (degree + 1) ** 2
    Y = sh_basis(d, degree, dtype)
    coef = np.asarray(sh, dtype).reshape(p.shape[0], -1, 3)[:, :nb, :]
    rgb = np.maximum(dtype(0.5) + np.einsum("nk,nkc->nc", Y, coef), dtype(0))
    return np.concatenate([rgb, np.asarray(opacity, dtype).reshape(-1, 1)], axis=1)


def composite(rec, color_opacity, z, indices, counts, offsets, width, height, tile=16, early_out=True):
    """rgba (H, W, 4) float32 image, alpha, depth, id, and the rim / near masks, over the given lists."""
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
    pxf, pyf = px.astype(F) + F(0.5), py.astype(F) + F(0.5)
    shape = px.shape
    T = np.ones(shape, F)
    C = np.zeros(shape + (3,), F)
    live = inimg.copy()
    rim = np.zeros(shape, bool)
    near = np.zeros(shape, bool)
    zw, ws = np.zeros(shape), np.zeros(shape)
    wmax = np.zeros(shape, F)
    idm = np.full(shape, 0xFFFFFFFF, np.uint32)
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
        g = np.where(lv & okb[s][:, None] & inside & (d2 <= F(1)), g, F(0))
        Ta = T[act]
        w = Ta * g
        C[act] += w[..., None] * col[s, None, :3]
        Tn = (Ta * (F(1) - g)).astype(F)
        near[act] |= lv & (np.abs((F(1) - Tn) - F(0.99)) < F(2e-5))
        zw[act] += w.astype(np.float64) * z[s][:, None]
        ws[act] += w
        top = w > wmax[act]
        wmax[act] = np.where(top, w, wmax[act])
        idm[act] = np.where(top, s.astype(np.uint32)[:, None], idm[act])
        T[act] = Tn
        if early_out:
            live[act] &= ~((F(1) - Tn) >= F(0.99))

    def scatter(a, fill, dtype, extra=()):
        img = np.full((height, width) + extra, fill, dtype)
        img[py[inimg], px[inimg]] = a[inimg]
        return img
    rgb = C + T[..., None] * BG[None, None, :]
    img = np.concatenate([rgb, np.ones(shape + (1,), F)], axis=-1).astype(F)
    with np.errstate(all="ignore"):
        depth = np.where(ws > 0, zw / np.where(ws > 0, ws, 1), np.inf)
    return dict(img=scatter(img, 0, F, (4,)), alpha=scatter((F(1) - T).astype(F), 0, F), depth=scatter(depth, np.inf, np.float64),
                id=scatter(idm, 0xFFFFFFFF, np.uint32), rim=scatter(rim, False, bool), near=scatter(near, False, bool))


def make_cloud(n, seed=0, spread=1.0, scale=0.03, degenerate=True):
    """A random cloud in front of the default camera: (n, 4) positions, scales, rotations, colour+opacity.  With degenerate
    splats mixed in: zero and huge scales, a zero quaternion, NaN, behind the camera, crossing w = 0."""
    rng = np.random.default_rng(seed)
    pos = np.ones((n, 4), F)
    pos[:, :3] = rng.uniform(-spread, spread, (n, 3))
    scl = np.zeros((n, 4), F)
    scl[:, :3] = np.exp(rng.normal(np.log(scale), 0.6, (n, 3)))
    rot = rng.normal(size=(n, 4)).astype(F)
    col = np.empty((n, 4), F)
    col[:, :3] = rng.uniform(0, 1, (n, 3))
    col[:, 3] = rng.uniform(0.2, 1.0, n)
    if degenerate and n >= 16:
        scl[0, :3] = 0                      # a point: only the 0.3 px dilation
        scl[1, :3] = [5.0, 0.01, 0.01]      # a needle larger than the screen
        scl[2, :3] = 50.0                   # reaches w = 0: culled
        rot[3] = 0                          # no rotation: NaN, culled
        pos[4, :3] = np.nan                 # culled
        pos[5, :3] = [3.2, 3.6, 5.8]        # behind the camera (eye at ~(1.3, 1.4, 2.3) looking at the origin)
        pos[6, :3] = [40.0, 0.0, 0.0]       # off screen
        scl[7, :3] = [0.0, 0.0, 1e-30]      # flat
    return pos, scl, rot, col
