"""AbsGS's absolute screen-space gradient (include/splat.h, splat_composite_backward_abs) in NumPy: per splat the sum over its
(pixel, consumed entry inside the cut) pairs of |term c.x| and |term c.y|, the terms being the ones whose signed sums are
columns 0 and 1 of grad_records.

The float64 value is already there: tests/composite_grad_terms_ref.terms64() returns m, the per-splat sum of |term|, and
m[:, :2] is the quantity (scene(name)["m"], ["m_depth"] with the depth channel).

pair_terms32()  the per-pair terms in binary32: terms32's arithmetic up to the per-splat sum (a test holds its signed sum to
                terms32's bits, so the two cannot drift apart).
abs32()         the per-splat sum of np.abs of those terms, accumulated in binary32 pair by pair, columns 0 and 1.
restated_abs()  abs32 on a scene under one update order, with c_abs = the largest |abs32 - m| / m over reached splats and the
                two numbers: the scale of the per-splat bound of the GPU tests, never taken from the kernel.
symmetric_uniforms(), symmetric_perturbation(), one_splat_sums(), density_statistic()
                the one-splat 32 x 32 frame of the fit's test: a splat whose record centre is exactly (16, 16) and an upstream
                that is point-symmetric about it, so that the signed dL/dc cancels and the absolute sum does not.
"""
import functools

import numpy as np

from tests import composite_grad_terms_ref as CT

F = np.float32


def pair_terms32(rec, col, z, lay, width, g, gd=None, order="quadrant"):
    """(pairs, 9 | 10) float32: what every pair adds, every operation rounded once in the kernel's order (CT.terms32 without
    its last step)."""
    assert order in CT.ORDERS
    r, c, dx, dy, u, v, ge, alpha = CT._geometry(rec, col, lay, width, F)
    start, K, keeps = lay["start"], lay["K"], lay["keeps"]
    G, GD = CT._upstreams(lay, g, gd, F)
    P = start.shape[0]
    zz = np.asarray(z, F)[lay["spl"]]
    op = c[:, 3]
    Tb = np.empty(alpha.shape[0], F)
    T, ws, zw = np.ones(P, F), np.zeros(P, F), np.zeros(P, F)
    for k in range(int(K.max()) if P else 0):
        rows = np.nonzero(K > k)[0]
        j = start[rows] + k
        Tb[j] = T[rows]
        if order == "px":
            w = T[rows] * ge[j]
            wgt = w * op[j]
            T[rows] = (T[rows].astype(np.float64) - op[j].astype(np.float64) * w.astype(np.float64)).astype(F)
        else:
            wgt = T[rows] * alpha[j]
            T[rows] = T[rows] - wgt
        zw[rows] = zw[rows] + zz[j] * wgt
        ws[rows] = ws[rows] + wgt
    GDn = Dp = None
    if gd is not None:
        some = ws > 0
        with np.errstate(all="ignore"):
            Dp = np.where(some, zw / ws, F(0)).astype(F)
            GDn = np.where(some, GD / ws, F(0)).astype(F)
    pid = np.repeat(np.arange(P), K)
    cg = ((G[pid, 0] * c[:, 0] + G[pid, 1] * c[:, 1]) + G[pid, 2] * c[:, 2]) + G[pid, 3]
    if gd is not None:
        cg = cg + GDn[pid] * (zz - Dp[pid])
    S = (G[:, 0] * F(0.05) + G[:, 1] * F(0.05)) + G[:, 2] * F(0.1)
    Tn = T.copy()
    Ti, dA = np.empty(alpha.shape[0], F), np.empty(alpha.shape[0], F)
    for k in range(int(K.max()) - 1 if P else -1, -1, -1):
        rows = np.nonzero(K > k)[0]
        j = start[rows] + k
        Ti[j] = np.where(keeps[j], Tb[j], Tn[rows] / (F(1) - alpha[j]))
        dA[j] = Ti[j] * (cg[j] - S[rows])
        S[rows] = alpha[j] * cg[j] + (F(1) - alpha[j]) * S[rows]
        Tn[rows] = Ti[j]
    t = CT._pair_terms(r, c, G[pid], dx, dy, u, v, ge, alpha, Ti, dA, None if gd is None else GDn[pid], F)
    assert t.dtype == F
    return t


def abs32(rec, col, z, lay, width, g, gd=None, order="quadrant"):
    """(n, 2) float32: per splat sum |term c.x|, sum |term c.y| of the binary32 terms, accumulated in binary32 pair by pair in
    (pixel, list position) order."""
    t = pair_terms32(rec, col, z, lay, width, g, gd, order)
    total = np.zeros((np.asarray(rec).shape[0], 2), F)
    np.add.at(total, lay["spl"], np.abs(t[:, :2]))
    return total


def want_abs(name, depth):
    """(n, 2) float64: the scene's reference, m[:, :2] of terms64 (with the depth channel: of the depth variant's terms)."""
    s = CT.scene(name)
    return (s["m_depth"] if depth else s["m"])[:, :2]


@functools.lru_cache(maxsize=None)
def restated_abs(name, order, depth):
    """dict(abs32 (n, 2), c (c_abs: the largest |abs32 - m| / m over reached splats and the two numbers))."""
    s = CT.scene(name)
    m = want_abs(name, depth)
    a = abs32(s["rec"], s["col"], s["z"], s["lay"], s["w"], s["g"], s["gd"] if depth else None, order)
    q = CT.ratios(a, m, m)
    a.setflags(write=False)
    return dict(abs32=a, c=float(q.max()))


# ---- the case the statistic exists for ---------------------------------------------------------------------------------------
SYM_W = SYM_H = 32
SYM_PIXELS = ((11, 12), (13, 9))   # (x, y) of the two perturbed pixels of tile (0, 0); their mirrors (31 - x, 31 - y) lie in tile (1, 1)
SYM_AMPLITUDES = (0.2, 0.13)       # the perturbation at the two pixels (and at their mirrors), fixed


def symmetric_uniforms(w=SYM_W, h=SYM_H):
    """A uniform block whose camera sits at the origin and looks down +z with clip = (x, y, z, z): a splat on the axis lands at
    exactly (w / 2, h / 2), with no rounding."""
    u = np.zeros(22, F)
    u[0] = u[5] = u[10] = u[11] = 1.0
    u[20], u[21] = w, h
    return u


def symmetric_perturbation(w=SYM_W, h=SYM_H):
    """(h, w, 3) float32, point-symmetric about the screen's centre (w / 2, h / 2): P(x, y) = P(w - 1 - x, h - 1 - y) at pixel
    centres, non-zero at the two pixels SYM_PIXELS and their mirrors only.

    Why so sparse.  A splat centred on (w / 2, h / 2) gives mirrored pixels terms that are each other's negatives bit for bit, in
    any precision.  Whether their SUM is zero depends on the order of the additions alone: float64 summed in pixel order leaves a
    residue near 1e-17 of the absolute sum, the kernel's binary32 sums (a DPP tree per wave, four waves, four tiles) one near
    1e-7 of it for a dense perturbation - the larger of the two by nine orders of magnitude, with the threshold (the geometric
    mean of the float64 statistics) between them on the wrong side.  With at most two non-zero terms per tile, all in tiles
    (0, 0) and (1, 1), every order of additions gives tile (0, 0) the sum fl(t1 + t2) and tile (1, 1) its negative, and s - s is
    0 in every order: the kernel's signed sum is exactly zero, as the symmetry says."""
    p = np.zeros((h, w, 3), F)
    for (x, y), a in zip(SYM_PIXELS, SYM_AMPLITUDES):
        p[y, x] = p[h - 1 - y, w - 1 - x] = a
    assert np.array_equal(p, p[::-1, ::-1])
    return p


def one_splat_sums(rec, col, g, w=SYM_W, h=SYM_H):
    """(signed (2,), absolute (2,)) float64: the sums over the pixels inside the cut of term c.x, term c.y and of their absolute
    values, added one by one in pixel order, of a frame of ONE splat with record rec (8,) and colour col (4,) under the
    upstream g (h, w, 4).  Every pixel has T = 1 and S = G . bg (nothing is behind the splat): composite_grad.hip's formulas with T_i = 1."""
    r, c = np.asarray(rec, np.float64), np.asarray(col, np.float64)
    y, x = np.mgrid[0:h, 0:w].astype(np.float64) + 0.5
    dx, dy = x - r[0], y - r[1]
    u, v = r[2] * dx + r[3] * dy, r[5] * dy
    d2 = u * u + v * v
    inside = d2 <= 1.0
    ge = np.where(inside, np.exp(-4.5 * d2), 0.0)
    alpha = ge * c[3]
    G = np.asarray(g, np.float64)
    cg = G[..., 0] * c[0] + G[..., 1] * c[1] + G[..., 2] * c[2] + G[..., 3]
    S = G[..., 0] * 0.05 + G[..., 1] * 0.05 + G[..., 2] * 0.1
    dd2 = -4.5 * alpha * (cg - S)
    du, dv = 2 * u * dd2, 2 * v * dd2
    t = np.stack([(-du * r[2])[inside], (-(du * r[3] + dv * r[5]))[inside]], axis=1)
    seq = lambda a: np.cumsum(a, axis=0)[-1]  # noqa: E731  (one add per pixel, in order: no pairwise regrouping)
    return seq(t), seq(np.abs(t))


def density_statistic(sums, w=SYM_W, h=SYM_H):
    """hypot(g.x W / 2, g.y H / 2): what splat_density_accumulate makes of a splat's two sums."""
    return float(np.hypot(sums[0] * w / 2, sums[1] * h / 2))
