"""Feature channels of a frame (include/splat.h, "Feature channels of a frame"; csrc/composite_features.hip) restated three ways
over the pairs that tests/ellipsoid_grad_ref.decisions records, on the four scenes of tests/composite_grad_terms_ref.scene:

features64()  torch float64, differentiable in rec, col and the features, as ellipsoid_grad_ref.composite64 is: F[k] = sum_i w_i
              f_i[k], no background, no division.  autograd of it is the reference the closed forms are held to.
terms64()     the closed forms in float64, pair by pair: the 6 + K numbers a (pixel, splat) pair adds to the splat's gradient
              (c.x, c.y, B00, B01, B11, opacity, then w G_F[k]), their per-splat signed sums and absolute sums m[s, k] = sum
              |term| (the scale of a per-splat bound: composite_grad_terms_ref's docstring), and per pixel the forward's F and
              m_px[k] = sum w_i |f_i[k]|.
terms32()     the kernels' own formulas in binary32, one rounding per operation, under either update order ("quadrant" /
              "px"), the sums accumulated pair by pair in binary32.  It never calls a kernel.  What it cannot mirror:
              contraction, v_exp_f32's ulp, the kernels' addition order.
restated()    terms32 against terms64 on a scene: c_scene = max |sum32 - sum64| / m over reached splats and numbers, c_fwd =
              max |F32 - F64| / m_px over unmasked pixels and channels, both floored at 2^-24; per-number relative L2.

Test inputs: features uniform(-2, 2), seeded per (scene, K); an upstream G_F uniform in [-1, 1], zeroed on rim | near pixels.
Everything is computed once per (scene[, order], K), shared and never written to.
"""
import functools

import numpy as np
import torch

from tests import composite_grad_terms_ref as CT
from tests import ellipsoid_grad_ref as GR

F = np.float32
D = torch.float64
NREC = 6                      # c.x, c.y, B00, B01, B11, opacity: the numbers before the channels
FLOOR = 2.0 ** -24
SCENES, ORDERS = CT.SCENES, CT.ORDERS


def names(K):
    return ("c.x", "c.y", "B00", "B01", "B11", "opacity") + tuple(f"f{k}" for k in range(K))


@functools.lru_cache(maxsize=None)
def inputs(name, K):
    """(features (n, K) float32 in (-2, 2), G_F (H, W, K) float32 in [-1, 1], zero on rim | near)."""
    s = CT.scene(name)
    seed = CT.make_scene_cloud(name)[6]
    rng = np.random.default_rng(1000 * seed + K)
    f = rng.uniform(-2, 2, (s["n"], K)).astype(F)
    g = rng.uniform(-1, 1, (s["h"], s["w"], K)).astype(F)
    g[s["dec"]["rim"] | s["dec"]["near"]] = 0
    f.setflags(write=False)
    g.setflags(write=False)
    return f, g


def masked(name):
    """(H, W) bool: rim | near, the pixels whose decisions binary32 and the reference may take differently."""
    d = CT.scene(name)["dec"]
    return d["rim"] | d["near"]


def features64(rec, col, feats, steps, width, height):
    """(H W, K) float64 over the recorded pairs, differentiable in rec (n, 8), col (n, 4) and feats (n, K)."""
    P = width * height
    flat = torch.arange(P)
    pix_x = (flat % width).to(D) + 0.5
    pix_y = torch.div(flat, width, rounding_mode="floor").to(D) + 0.5
    T = torch.ones(P, dtype=D)
    Fm = torch.zeros((P, feats.shape[1]), dtype=D)
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
        Fm = Fm.index_add(0, pix_t, (Tp * a)[:, None] * feats[s_t])
        T = T.index_put((pix_t,), Tp * (1 - a))
    return Fm


def autograd64(name, K):
    """(n, 6 + K) float64: dL/d(c.x, c.y, B00, B01, B11, opacity, f) of L = sum G_F . F by torch autograd over features64, and
    the (n, 3) gradient of col's colour columns (which must be zero)."""
    s = CT.scene(name)
    f, g = inputs(name, K)
    rec = torch.tensor(np.asarray(s["rec"], np.float64), requires_grad=True)
    col = torch.tensor(np.asarray(s["col"], np.float64), requires_grad=True)
    ft = torch.tensor(np.asarray(f, np.float64), requires_grad=True)
    Fm = features64(rec, col, ft, s["dec"]["steps"], s["w"], s["h"])
    (Fm * torch.as_tensor(np.asarray(g, np.float64).reshape(-1, K))).sum().backward()
    gr, gc = rec.grad.numpy(), col.grad.numpy()
    return np.concatenate([gr[:, CT.REC_COLS], gc[:, 3:4], ft.grad.numpy()], axis=1), gc[:, :3]


# ---- the walks, which do not depend on the features ---------------------------------------------------------------------------
def _steps(lay):
    """Per list rank k: (rows: the pixels of lay['start'] with more than k pairs, j: their k-th pair)."""
    start, K = lay["start"], lay["K"]
    out = []
    for k in range(int(K.max()) if start.shape[0] else 0):
        rows = np.nonzero(K > k)[0]
        out.append((rows, start[rows] + k))
    return out


@functools.lru_cache(maxsize=None)
def _walk64(name):
    s = CT.scene(name)
    lay = s["lay"]
    r, c, dx, dy, u, v, ge, alpha = CT._geometry(s["rec"], s["col"], lay, s["w"], np.float64)
    steps = _steps(lay)
    P = lay["start"].shape[0]
    Ti = np.empty(alpha.shape[0])
    T = np.ones(P)
    for rows, j in steps:
        Ti[j] = T[rows]
        T[rows] = T[rows] * (1.0 - alpha[j])
    return dict(r=r, dx=dx, dy=dy, u=u, v=v, ge=ge, alpha=alpha, Ti=Ti, steps=steps, pid=np.repeat(np.arange(P), lay["K"]))


@functools.lru_cache(maxsize=None)
def _walk32(name, order):
    """Binary32: the geometry, walk 1 under `order` (T before each pair, the forward's weight of each pair) and walk 2's
    recovered T_i (T_{L-1} kept at a pixel's last consumed entry, T_{i+1} / (1 - alpha_i) elsewhere)."""
    assert order in ORDERS
    s = CT.scene(name)
    lay = s["lay"]
    r, c, dx, dy, u, v, ge, alpha = CT._geometry(s["rec"], s["col"], lay, s["w"], F)
    op = c[:, 3]
    steps = _steps(lay)
    P = lay["start"].shape[0]
    Tb, wf = np.empty(alpha.shape[0], F), np.empty(alpha.shape[0], F)
    T = np.ones(P, F)
    for rows, j in steps:
        Tb[j] = T[rows]
        if order == "px":
            w = T[rows] * ge[j]
            wf[j] = w * op[j]
            T[rows] = (T[rows].astype(np.float64) - op[j].astype(np.float64) * w.astype(np.float64)).astype(F)
        else:
            wf[j] = T[rows] * alpha[j]
            T[rows] = T[rows] - wf[j]
    Tn = T.copy()
    Ti = np.empty(alpha.shape[0], F)
    keeps = lay["keeps"]
    for rows, j in reversed(steps):
        Ti[j] = np.where(keeps[j], Tb[j], Tn[rows] / (F(1) - alpha[j]))
        Tn[rows] = Ti[j]
    assert Ti.dtype == F and wf.dtype == F
    return dict(r=r, dx=dx, dy=dy, u=u, v=v, ge=ge, alpha=alpha, Ti=Ti, wf=wf, steps=steps, pid=np.repeat(np.arange(P), lay["K"]))


def _record_terms(wk, dA, dt):
    """The six numbers before the channels of every pair from dA = T_i (s - S), in the kernel's order."""
    r, u, v, alpha = wk["r"], wk["u"], wk["v"], wk["alpha"]
    dd2 = dt(-4.5) * alpha * dA
    du, dv = dt(2) * u * dd2, dt(2) * v * dd2
    return [-du * r[:, 2], -(du * r[:, 3] + dv * r[:, 5]), du * wk["dx"], du * wk["dy"], dv * wk["dy"], wk["ge"] * dA]


@functools.lru_cache(maxsize=None)
def terms64(name, K):
    """dict(sum, m (n, 6 + K): signed and absolute sums per splat of the pairs' float64 terms; F, m_px (H W, K): the forward and
    sum w |f| per pixel; L_px (H W,) int: the pairs of each pixel)."""
    s = CT.scene(name)
    lay, n, npx = s["lay"], s["n"], s["w"] * s["h"]
    wk = _walk64(name)
    f32, g32 = inputs(name, K)
    f = np.asarray(f32, np.float64)[lay["spl"]]
    G = np.asarray(g32, np.float64).reshape(-1, K)[lay["upix"]]
    pid, alpha, Ti = wk["pid"], wk["alpha"], wk["Ti"]
    sdot = (G[pid] * f).sum(axis=1)
    S = np.zeros(G.shape[0])
    dA = np.empty(alpha.shape[0])
    for rows, j in reversed(wk["steps"]):
        dA[j] = Ti[j] * (sdot[j] - S[rows])
        S[rows] = alpha[j] * sdot[j] + (1.0 - alpha[j]) * S[rows]
    wgt = Ti * alpha
    cols = _record_terms(wk, dA, np.float64) + [wgt * G[pid, k] for k in range(K)]
    spl = lay["spl"]
    total = np.stack([np.bincount(spl, weights=t, minlength=n) for t in cols], axis=1)
    m = np.stack([np.bincount(spl, weights=np.abs(t), minlength=n) for t in cols], axis=1)
    Fm, m_px = forward64(name, f32)
    L_px = np.bincount(lay["pix"], minlength=npx)
    return CT._freeze(dict(sum=total, m=m, F=Fm, m_px=m_px, L_px=L_px))


def forward64(name, feats):
    """(F, m_px) (H W, K) float64 of any (n, K) features on a scene: sum w f and sum w |f| over each pixel's pairs."""
    s = CT.scene(name)
    lay, npx = s["lay"], s["w"] * s["h"]
    wk = _walk64(name)
    f = np.asarray(feats, np.float64)[lay["spl"]]
    wgt = wk["Ti"] * wk["alpha"]
    Fm, m_px = np.zeros((npx, f.shape[1])), np.zeros((npx, f.shape[1]))
    for k in range(f.shape[1]):
        Fm[:, k] = np.bincount(lay["pix"], weights=wgt * f[:, k], minlength=npx)
        m_px[:, k] = np.bincount(lay["pix"], weights=wgt * np.abs(f[:, k]), minlength=npx)
    return Fm, m_px


@functools.lru_cache(maxsize=None)
def terms32(name, order, K):
    """dict(sum (n, 6 + K) float32: the per-splat sums of the pairs' binary32 terms, accumulated pair by pair in (pixel, list
    position) order; F (H W, K) float32: the forward, accumulated per pixel in list order)."""
    s = CT.scene(name)
    lay, n, npx = s["lay"], s["n"], s["w"] * s["h"]
    wk = _walk32(name, order)
    f32, g32 = inputs(name, K)
    f = f32[lay["spl"]]
    G = g32.reshape(-1, K)[lay["upix"]]
    pid, alpha, Ti = wk["pid"], wk["alpha"], wk["Ti"]
    Gp = G[pid]
    sdot = np.zeros(alpha.shape[0], F)
    for k in range(K):
        sdot = sdot + Gp[:, k] * f[:, k]
    S = np.zeros(G.shape[0], F)
    dA = np.empty(alpha.shape[0], F)
    acc = np.zeros((G.shape[0], K), F)
    for rows, j in wk["steps"]:
        acc[rows] = acc[rows] + wk["wf"][j][:, None] * f[j]
    for rows, j in reversed(wk["steps"]):
        dA[j] = Ti[j] * (sdot[j] - S[rows])
        S[rows] = alpha[j] * sdot[j] + (F(1) - alpha[j]) * S[rows]
    wgt = Ti * alpha
    cols = _record_terms(wk, dA, F) + [wgt * Gp[:, k] for k in range(K)]
    total = np.zeros((n, NREC + K), F)
    for k, t in enumerate(cols):
        assert t.dtype == F
        np.add.at(total[:, k], lay["spl"], t)
    Fm = np.zeros((npx, K), F)
    Fm[lay["upix"]] = acc
    assert acc.dtype == F and S.dtype == F and sdot.dtype == F
    return CT._freeze(dict(sum=total, F=Fm))


@functools.lru_cache(maxsize=None)
def restated(name, order, K):
    """dict(c_scene, c_fwd (floored at 2^-24), l2 (per number: sum32's relative L2 against sum64))."""
    s = CT.scene(name)
    t64, t32 = terms64(name, K), terms32(name, order, K)
    q = CT.ratios(t32["sum"], t64["sum"], t64["m"])[s["reached"]]
    ok = ~masked(name).reshape(-1)
    qf = CT.ratios(t32["F"], t64["F"], t64["m_px"])[ok]
    return CT._freeze(dict(c_scene=max(float(q.max()), FLOOR), c_fwd=max(float(qf.max()), FLOOR),
                           l2=np.array([CT.rel_l2(t32["sum"][:, k], t64["sum"][:, k]) for k in range(NREC + K)])))
