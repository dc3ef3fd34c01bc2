"""Float64 restatement of include/splat.h, "Normals of a depth map": the camera's rays, the normal of the surface a depth map
describes, 2DGS's normal-consistency loss, their hand-written backward, and the error bounds the GPU tests hold the binary32
kernels to.  NumPy throughout; normals_torch / loss_torch state the forward again in torch float64 ops so that CPU autograd can
check the hand-written backward.

The normal is evaluated in the contract's own form, n = sigma (a_y x a_x) with a_x = (s_r - s_l) d + (s_r + s_l) Dx and
a_y = (s_d - s_u) d + (s_d + s_u) Dy, not in the kernels' expanded one: in float64 the two agree to 1e-13.

Bounds (eps = 2^-24, all per pixel, zero where the pixel is invalid):
  kappa   = || sum |products of the cross| || / |n|, the products taken of the terms a_x and a_y are themselves sums of:
            with A_x = |s_r - s_l| |d| + |s_r + s_l| |Dx| (componentwise) and A_y likewise, component i of the sum is
            A_y[j] A_x[k] + A_y[k] A_x[j].  It bounds what one rounding of every product and sum of the cross does to N.
  lambda  = sum_k ||dN/ds_k|| |s_k| over the four neighbours: what the last bit of each ray parameter does to N.
  E       = kappa + lambda;  ||N32 - N64|| <= k eps E is the forward check.
  dL/ddepth: pixel q adds up to four contributions c = dL/ds_k(p) ds/ddepth(q), each g_n . dn_k with g_n = (I - N N^T) gN / |n|
            and dn_k = dn/ds_k.  To first order the error of c is dg_n . dn_k + g_n . d(dn_k), beside the roundings of the dot
            product itself (at most a few eps |c|).
            dg_n: an error of relative size eps E in n changes (I - N N^T) / |n| by at most 3 eps E / |n| in norm (two terms from
            N, one from |n|), so |dg_n . dn_k| <= 3 eps E M_k with M_k = ||gN|| ||dn_k|| / |n|.
            d(dn_k): dn_r = sigma [(s_d - s_u) P + (s_d + s_u) (Q + C)] with P = d x Dx, Q = Dy x d, C = Dy x Dx (the d x d term of
            a_y x (d + Dx) is zero), and likewise for the others.  The difference s_d - s_u carries the rounding of both ray
            parameters, eps (s_d + s_u), and every product one more: componentwise |d(dn_k)| <= eps T_k,
            T_k = (|s + s'| + |s - s'|) |P| + |s + s'| (|Q| + |C|) (P and Q exchanged for k = u, d), so |g_n . d(dn_k)| <= eps m_k
            with m_k = ||gN|| ||T_k|| / |n|.
            The bound on q's sum is k eps sum over its contributions of (|c| + 3 E_p M_k + m_k) ds/ddepth(q).
"""
import types

import numpy as np

EPS = 2.0 ** -24
DISTANCE, Z = "distance", "z"
KINDS = {DISTANCE: 0, Z: 1}


class RefusedCamera(ValueError):
    pass


def vp_rows(u):
    """(M (3, 3), m (3,)): rows 0, 1, 3 of the block's VP (VP[r][c] = u[4 c + r]) on xyz, and their fourth column."""
    vp = np.asarray(u, np.float64)[:16].reshape(4, 4).T
    return vp[[0, 1, 3], :3], vp[[0, 1, 3], 3]


def camera_rays(u, width=None, height=None):
    """(D0, Dx, Dy, sigma) in float64 of the block's camera on a width x height screen (default: u[20], u[21])."""
    u = np.asarray(u, np.float64)
    W = float(u[20] if width is None else width)
    H = float(u[21] if height is None else height)
    M, _ = vp_rows(u)
    scale = np.prod(np.linalg.norm(M, axis=1))
    if not abs(np.linalg.det(M)) > 1e-14 * scale:
        raise RefusedCamera("rows 0, 1, 3 of VP are singular on xyz")
    Mi = np.linalg.inv(M)
    D0 = Mi @ np.array([1.0 / W - 1.0, 1.0 - 1.0 / H, 1.0])
    Dx = Mi @ np.array([2.0 / W, 0.0, 0.0])
    Dy = Mi @ np.array([0.0, -2.0 / H, 0.0])
    dc = Mi @ np.array([0.0, 0.0, 1.0])
    sigma = -np.sign(np.dot(np.cross(Dy, Dx), dc))
    if sigma == 0 or not np.isfinite(sigma):
        raise RefusedCamera("sigma is 0")
    return D0, Dx, Dy, float(sigma)


def rays(u, width, height):
    """d (H, W, 3): the ray of every pixel centre."""
    D0, Dx, Dy, _ = camera_rays(u, width, height)
    ys, xs = np.mgrid[0:height, 0:width].astype(np.float64)
    return D0 + xs[..., None] * Dx + ys[..., None] * Dy


def plane_depth(u, width, height, normal, offset, kind=DISTANCE):
    """The depth map (float64) of the plane normal . X = offset seen through the block's camera (eye = u[16:19] must be the
    camera's: M eye + m = 0), +inf where a ray does not meet it in front of the eye."""
    eye = -np.linalg.solve(*vp_rows(u))
    d = rays(u, width, height)
    with np.errstate(divide="ignore", invalid="ignore"):
        s = (offset - eye @ np.asarray(normal, np.float64)) / (d @ np.asarray(normal, np.float64))
    s = np.where(np.isfinite(s) & (s > 0), s, np.inf)
    return s * np.linalg.norm(d, axis=2) if kind == DISTANCE else s


def _cross(a, b):
    return np.cross(a, b)


def forward(depth, u, kind=DISTANCE):
    """Everything about the normals of `depth` (H, W): a namespace with N (H, W, 3), valid (H, W) and, on the interior
    (H - 2, W - 2) grid, the intermediate quantities the backward and the bounds need."""
    depth = np.asarray(depth, np.float64)
    H, W = depth.shape
    r = types.SimpleNamespace(H=H, W=W, kind=kind, depth=depth, N=np.zeros((H, W, 3)), valid=np.zeros((H, W), bool), E=np.zeros((H, W)))
    r.D0, r.Dx, r.Dy, r.sigma = camera_rays(u, W, H)
    d = rays(u, W, H)
    r.inv = 1.0 / np.linalg.norm(d, axis=2) if kind == DISTANCE else np.ones((H, W))
    if H < 3 or W < 3:
        r.interior = None
        return r
    ok_depth = np.isfinite(depth) & (depth > 0)
    s = np.where(ok_depth, depth, 1.0) * r.inv  # (an unusable depth invalidates its neighbours below; 1 keeps the arithmetic quiet)
    sl, sr, su, sd = s[1:-1, :-2], s[1:-1, 2:], s[:-2, 1:-1], s[2:, 1:-1]
    ok = ok_depth[1:-1, :-2] & ok_depth[1:-1, 2:] & ok_depth[:-2, 1:-1] & ok_depth[2:, 1:-1]
    dp = d[1:-1, 1:-1]
    i = types.SimpleNamespace(sl=sl, sr=sr, su=su, sd=sd, d=dp)
    i.ax = (sr - sl)[..., None] * dp + (sr + sl)[..., None] * r.Dx
    i.ay = (sd - su)[..., None] * dp + (sd + su)[..., None] * r.Dy
    i.n = r.sigma * _cross(i.ay, i.ax)
    nn = (i.n * i.n).sum(axis=2)
    ok = ok & np.isfinite(nn) & (nn > 0)
    i.len = np.sqrt(np.where(ok, nn, 1.0))
    i.ok = ok
    i.N = np.where(ok[..., None], i.n / i.len[..., None], 0.0)
    r.N[1:-1, 1:-1] = i.N
    r.valid[1:-1, 1:-1] = ok
    # the four derivatives dn/ds_k, k = l, r, u, d
    i.e = (r.Dx - dp, dp + r.Dx, r.Dy - dp, dp + r.Dy)
    i.dn = (r.sigma * _cross(i.ay, i.e[0]), r.sigma * _cross(i.ay, i.e[1]), r.sigma * _cross(i.e[2], i.ax), r.sigma * _cross(i.e[3], i.ax))
    # bounds
    ad = np.abs(dp)
    i.Ax = np.abs(sr - sl)[..., None] * ad + np.abs(sr + sl)[..., None] * np.abs(r.Dx)
    i.Ay = np.abs(sd - su)[..., None] * ad + np.abs(sd + su)[..., None] * np.abs(r.Dy)
    prod = np.stack([i.Ay[..., 1] * i.Ax[..., 2] + i.Ay[..., 2] * i.Ax[..., 1],
                     i.Ay[..., 2] * i.Ax[..., 0] + i.Ay[..., 0] * i.Ax[..., 2],
                     i.Ay[..., 0] * i.Ax[..., 1] + i.Ay[..., 1] * i.Ax[..., 0]], axis=2)
    i.kappa = np.linalg.norm(prod, axis=2) / i.len
    lam = 0.0
    for dn, sk in zip(i.dn, (sl, sr, su, sd)):
        dN = (dn - i.N * (i.N * dn).sum(axis=2, keepdims=True)) / i.len[..., None]
        lam = lam + np.linalg.norm(dN, axis=2) * np.abs(sk)
    i.lam = lam
    i.E = np.where(ok, i.kappa + lam, 0.0)
    r.E[1:-1, 1:-1] = i.E
    # T_k: componentwise bound, per unit eps, on the error of dn_k (the module's docstring), k = l, r, u, d
    aP, aQ, aC = np.abs(_cross(dp, r.Dx)), np.abs(_cross(r.Dy, dp)), np.abs(_cross(r.Dy, r.Dx))
    Ty = (np.abs(sd + su) + np.abs(sd - su))[..., None] * aP + np.abs(sd + su)[..., None] * (aQ + aC)
    Tx = (np.abs(sr + sl) + np.abs(sr - sl))[..., None] * aQ + np.abs(sr + sl)[..., None] * (aP + aC)
    i.T = (Ty, Ty, Tx, Tx)
    r.interior = i
    return r


def normals(depth, u, kind=DISTANCE):
    r = forward(depth, u, kind)
    return r.N, r.valid


def _gather(r, per_k):
    """Add the four interior arrays (for k = l, r, u, d) into the pixels they name, in the contract's order."""
    out = np.zeros((r.H, r.W))
    out[1:-1, :-2] += per_k[0]   # q is the left neighbour of q + (1, 0)
    out[1:-1, 2:] += per_k[1]    # the right one of q - (1, 0)
    out[:-2, 1:-1] += per_k[2]   # the upper one of q + (0, 1)
    out[2:, 1:-1] += per_k[3]    # the lower one of q - (0, 1)
    return out


def backward(r, gN):
    """(dL/ddepth (H, W), its error bound per unit k eps (H, W)) from dL/dN (H, W, 3) for the forward `r`.  The upstream of an
    invalid pixel is selected away."""
    zero = np.zeros((r.H, r.W))
    if r.interior is None:
        return zero, zero
    i = r.interior
    g = np.where(i.ok[..., None], np.asarray(gN, np.float64)[1:-1, 1:-1], 0.0)
    gn = (g - i.N * (i.N * g).sum(axis=2, keepdims=True)) / i.len[..., None]
    c = [np.where(i.ok, (gn * dn).sum(axis=2), 0.0) for dn in i.dn]
    gnorm = np.linalg.norm(g, axis=2)
    scale = np.where(i.ok, gnorm / i.len, 0.0)
    extra = [scale * (3.0 * i.E * np.linalg.norm(dn, axis=2) + np.linalg.norm(T, axis=2)) for dn, T in zip(i.dn, i.T)]
    finite = np.isfinite(r.depth)
    grad = np.where(finite, _gather(r, c) * r.inv, 0.0)
    bound = np.where(finite, _gather(r, [np.abs(ck) + ek for ck, ek in zip(c, extra)]) * r.inv, 0.0)
    return grad, bound


def loss(normal_map, depth, u, weight=None, kind=DISTANCE):
    """(L, fraction of valid pixels, per-pixel error bound of the term per unit k eps (H, W), the forward)."""
    r = forward(depth, u, kind)
    F = np.where(r.valid[..., None], np.asarray(normal_map, np.float64)[..., :3], 0.0)
    w = np.ones((r.H, r.W)) if weight is None else np.where(r.valid, np.asarray(weight, np.float64), 0.0)
    L = float(np.mean(1.0 - w * (F * r.N).sum(axis=2)))
    bound = np.abs(w) * np.linalg.norm(F, axis=2) * r.E
    return L, float(r.valid.mean()), bound, r


def loss_backward(r, normal_map, weight=None, upstream=1.0):
    """(dL/dF (H, W, 3), its bound per unit k eps (H, W), dL/ddepth (H, W), its bound per unit k eps (H, W))."""
    F = np.where(r.valid[..., None], np.asarray(normal_map, np.float64)[..., :3], 0.0)
    w = np.ones((r.H, r.W)) if weight is None else np.where(r.valid, np.asarray(weight, np.float64), 0.0)
    k = -float(upstream) / (r.W * r.H)
    gF = k * w[..., None] * r.N
    gF_bound = np.abs(k * w) * r.E
    gz, gz_bound = backward(r, k * w[..., None] * F)
    return gF, gF_bound, gz, gz_bound


# ---- the forward in torch float64 ops, for CPU autograd ----------------------------------------------------------------------
def normals_torch(depth, u, kind=DISTANCE):
    """N (H, W, 3) of a torch float64 depth map, differentiable in it (the camera is a constant)."""
    import torch
    H, W = depth.shape
    D0, Dx, Dy, sigma = camera_rays(u, W, H)
    d = torch.from_numpy(rays(u, W, H))
    Dx, Dy = torch.from_numpy(Dx), torch.from_numpy(Dy)
    N = torch.zeros((H, W, 3), dtype=torch.float64)
    if H < 3 or W < 3:
        return N
    ok_depth = torch.isfinite(depth) & (depth > 0)
    s = torch.where(ok_depth, depth, torch.ones_like(depth))
    if kind == DISTANCE:
        s = s / d.norm(dim=2)
    sl, sr, su, sd = s[1:-1, :-2], s[1:-1, 2:], s[:-2, 1:-1], s[2:, 1:-1]
    ok = ok_depth[1:-1, :-2] & ok_depth[1:-1, 2:] & ok_depth[:-2, 1:-1] & ok_depth[2:, 1:-1]
    dp = d[1:-1, 1:-1]
    ax = (sr - sl)[..., None] * dp + (sr + sl)[..., None] * Dx
    ay = (sd - su)[..., None] * dp + (sd + su)[..., None] * Dy
    n = sigma * torch.linalg.cross(ay, ax)
    nn = (n * n).sum(dim=2)
    ok = ok & torch.isfinite(nn) & (nn > 0)
    n = torch.where(ok[..., None], n, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64).expand_as(n))
    inner = torch.where(ok[..., None], n / n.norm(dim=2, keepdim=True), torch.zeros_like(n))
    return torch.nn.functional.pad(inner.permute(2, 0, 1), (1, 1, 1, 1)).permute(1, 2, 0)


def loss_torch(normal_map, depth, u, weight=None, kind=DISTANCE):
    import torch
    N = normals_torch(depth, u, kind)
    valid = (N != 0).any(dim=2)
    F = torch.where(valid[..., None], normal_map[..., :3], torch.zeros_like(N))
    w = torch.ones_like(depth) if weight is None else torch.where(valid, weight, torch.zeros_like(depth))
    return (1.0 - w * (F * N).sum(dim=2)).mean()


# ---- inputs the tests share ----------------------------------------------------------------------------------------------------
def pinhole_camera(width, height, focal, mirrored=False):
    """A pinhole block (float32) with fx != fy and an off-centre principal point, looking at the origin from (0.4, 0.3, -3);
    mirrored: the x axis of the screen flipped (column 0 of the pose negated: det R = -1)."""
    import torch
    from splat_renderer_amd import autograd as AG
    from tests import cameras
    R, t = cameras.look_at((0.4, 0.3, -3.0), (0.0, 0.0, 0.0), roll=0.2)
    if mirrored:
        R = R.copy()
        R[0] = -R[0]
        t = t.copy()
        t[0] = -t[0]
    u = AG.pinhole_uniforms(torch.as_tensor(R), torch.as_tensor(t), focal, 1.1 * focal, 0.47 * width, 0.55 * height, width, height)
    return u.numpy().astype(np.float32)


def depth_maps(u, width, height, kind, seed=0):
    """name -> (H, W) float32 depth map: a bumpy plane, a step discontinuity, holes (+inf) in the interior, touching a border and
    as a 1-pixel island of depth in a hole, and an all-+inf map."""
    rng = np.random.default_rng(seed)
    base = plane_depth(u, width, height, (0.2, 0.3, -1.0), 0.4, kind)
    base = np.where(np.isfinite(base), base, 3.0)
    ys, xs = np.mgrid[0:height, 0:width]
    bumpy = base * (1.0 + 0.01 * np.sin(0.9 * xs + 0.3) * np.cos(0.7 * ys) + 0.002 * rng.standard_normal((height, width)))
    step = np.where(xs + ys // 2 > (width + height // 2) // 2, base * 1.5, base)
    holes = bumpy.copy()
    holes[: max(height // 4, 1), : max(width // 5, 1)] = np.inf                   # touches two borders
    y0, x0 = height // 2, width // 2
    holes[y0 - 2:y0 + 3, x0 - 2:x0 + 3] = np.inf                                  # an interior hole ...
    if height > 2 and width > 2:
        holes[y0, x0] = bumpy[y0, x0]                                             # ... with a 1-pixel island in it
    if height > 6 and width > 6:
        holes[height - 3, 2] = np.inf                                             # a 1-pixel hole
    return {"bumpy": bumpy.astype(np.float32), "step": step.astype(np.float32), "holes": holes.astype(np.float32),
            "empty": np.full((height, width), np.inf, np.float32)}
