"""The composite backward pair by pair (csrc/composite_grad.hip, k_composite_backward's second walk), in NumPy, over the pairs that
tests/ellipsoid_grad_ref.decisions records: what every (pixel, splat) pair adds to the splat's nine gradient numbers (c.x, c.y,
B00, B01, B11, r, g, b, opacity) and, with a depth map, to a tenth (dL/dz).

terms64()   the terms in float64, T taken from the forward product; per splat their signed sum and their absolute sum
            m[s, k] = sum over the splat's pairs of |term|.  m is the scale of a per-splat bound: a binary32 sum's error is
            proportional to it whatever the order of the additions, and it stays meaningful where a splat's terms cancel (|sum| / m
            goes down to about 4e-6 on the scenes below, so no bound relative to |sum| can hold for a correct kernel).
terms32()   the same in binary32, one rounding per operation in the kernel's order: the forward T under either update order
            ("quadrant": T -= T (g o), k_composite's; "px": T = fma(-o, T g, T), k_composite_px's, the product formed exactly in
            float64 and the sum rounded once), T_{L-1} kept at a pixel's last consumed entry and T_i = T_{i+1} / (1 - alpha_i)
            elsewhere, S blended back to front, and the per-splat sums accumulated in binary32 pair by pair.  What it cannot
            mirror: contraction, v_exp_f32's 1 ulp against NumPy's half ulp, and the kernel's addition order (a DPP tree per
            wave, four waves, atomics or the fixed-order gather).
scene()     four scenes with everything the tests need, computed once and shared read-only: `classic` (the other gradient
            tests' first case) and three that the suite had none of: `hazy` (opacity 0.004 .. 0.03: a pixel consumes hundreds of
            pairs and the early-out rarely fires), `veil` (hazy in front of an opaque backdrop: pixels stop deep in their lists,
            off the 64-entry chunk boundaries) and `needle` (two axes of 0.0005: cond(Sigma2) up to 1.6e4).

The depth variant carries D = sum w z / sum w as composite_grad.hip's header describes: a fifth channel of colour z_i - D, background 0 and
upstream G_D / ws, and the tenth number w_i G_D / ws.
"""
import functools

import numpy as np

from oracle import np_oracle as NO
from oracle import oracle as O
from tests import ellipsoid_depth_grad_ref as DR
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER

F = np.float32
NV = 9
REC_COLS = (0, 1, 2, 3, 5)           # the columns of grad_records that sums[:, 0:5] are; sums[:, 5:9] is grad_color_opacity
NAMES = ("c.x", "c.y", "B00", "B01", "B11", "r", "g", "b", "opacity", "z")
EXP2_SCALE = F(-6.492127684000335)   # composite.h's ELLIPSOID_EXP2_SCALE: exp(-4.5 d2) = exp2(d2 * this)
TILE = 16
GCH = 64                             # composite_grad.hip's chunk of staged entries
SCENES = ("hazy", "veil", "needle", "classic")
ORDERS = ("quadrant", "px")


# ---- the pairs of a frame, pixel by pixel ----------------------------------------------------------------------------------
def pair_layout(steps, counts, width, tile=TILE):
    """decisions()' steps as flat arrays sorted by (pixel, list position): dict(pix, spl, pos, start (first pair of each pixel
    that has one), K (pairs per such pixel), upix (its flat index), rank (a pair's number within its pixel), keeps (per pair:
    it is the pixel's last CONSUMED entry, where the kernel keeps T_{L-1} from walk 1 instead of dividing: the entry the
    early-out stopped at, or the last entry of a list the pixel never stopped in), L (per such pixel, the consumed count when
    it stopped, else 0))."""
    pix = np.concatenate([s[0] for s in steps] + [np.zeros(0, np.int64)]).astype(np.int64)
    spl = np.concatenate([s[1] for s in steps] + [np.zeros(0, np.int64)]).astype(np.int64)
    stop = np.concatenate([s[2] for s in steps] + [np.zeros(0, bool)]).astype(bool)
    pos = np.concatenate([np.full(s[0].shape[0], i, np.int64) for i, s in enumerate(steps)] + [np.zeros(0, np.int64)])
    o = np.lexsort((pos, pix))
    pix, spl, stop, pos = pix[o], spl[o], stop[o], pos[o]
    first = np.ones(pix.shape[0], bool)
    first[1:] = pix[1:] != pix[:-1]
    start = np.nonzero(first)[0]
    K = np.diff(np.append(start, pix.shape[0]))
    upix = pix[start]
    rank = np.arange(pix.shape[0]) - np.repeat(start, K)
    ntx = -(-width // tile)
    tile_of = (upix // width // tile) * ntx + (upix % width) // tile
    last = start + K - 1
    assert not stop[np.setdiff1d(np.arange(pix.shape[0]), last)].any(), "a pixel went on past its stop"
    keeps = np.zeros(pix.shape[0], bool)
    keeps[last] = stop[last] | (pos[last] == np.asarray(counts, np.int64)[tile_of] - 1)
    L = np.where(stop[last], pos[last] + 1, 0)
    return dict(pix=pix, spl=spl, pos=pos, start=start, K=K, upix=upix, rank=rank, keeps=keeps, L=L)


def _geometry(rec, col, lay, width, dt):
    """Per pair, in dtype dt with one rounding per operation in entry_alpha's order: dx, dy, u, v, ge, alpha."""
    s = lay["spl"]
    r, c = np.asarray(rec, dt)[s], np.asarray(col, dt)[s]
    pxf = (lay["pix"] % width).astype(dt) + dt(0.5)
    pyf = (lay["pix"] // width).astype(dt) + dt(0.5)
    dx, dy = pxf - r[:, 0], pyf - r[:, 1]
    u = r[:, 2] * dx + r[:, 3] * dy
    v = r[:, 5] * dy
    d2 = u * u + v * v
    ge = np.exp2(d2 * EXP2_SCALE).astype(dt) if dt is F else np.exp(-4.5 * d2)
    return r, c, dx, dy, u, v, ge, (ge * c[:, 3]).astype(dt)


def _pair_terms(r, c, G, dx, dy, u, v, ge, alpha, Ti, dA, GDn, dt):
    """The nine (ten) numbers of every pair from its T_i and dL/dalpha_i / T-less factor dA = T_i (G.c - S), in the kernel's order."""
    wgt = Ti * alpha
    dd2 = dt(-4.5) * alpha * dA
    du, dv = dt(2) * u * dd2, dt(2) * v * dd2
    out = [-du * r[:, 2], -(du * r[:, 3] + dv * r[:, 5]), du * dx, du * dy, dv * dy, wgt * G[:, 0], wgt * G[:, 1], wgt * G[:, 2], ge * dA]
    if GDn is not None:
        out.append(wgt * GDn)
    return np.stack(out, axis=1).astype(dt)


def _upstreams(lay, g, gd, dt):
    G = np.asarray(g, dt).reshape(-1, 4)[lay["upix"]]
    GD = None if gd is None else np.asarray(gd, dt).reshape(-1)[lay["upix"]]
    return G, GD


def terms64(rec, col, z, lay, width, g, gd=None):
    """dict(sum (n, 9 | 10) signed and m (n, 9 | 10) absolute sums of the pairs' float64 terms per splat, ws (per pixel of
    lay["upix"]: sum w)).  gd (H, W) or None: with the depth channel and the tenth number (gd is not read where ws = 0)."""
    D = np.float64
    n = np.asarray(rec).shape[0]
    r, c, dx, dy, u, v, ge, alpha = _geometry(rec, col, lay, width, D)
    start, K = lay["start"], lay["K"]
    G, GD = _upstreams(lay, g, gd, D)
    P = start.shape[0]
    zz = np.asarray(z, D)[lay["spl"]]
    Ti = np.empty(alpha.shape[0])
    T, ws, zw = np.ones(P), np.zeros(P), np.zeros(P)
    for k in range(int(K.max()) if P else 0):
        rows = np.nonzero(K > k)[0]
        j = start[rows] + k
        Ti[j] = T[rows]
        w = T[rows] * alpha[j]
        ws[rows] += w
        zw[rows] += w * zz[j]
        T[rows] = T[rows] * (1.0 - alpha[j])
    GDn = Dp = None
    if gd is not None:
        some = ws > 0
        Dp = np.where(some, zw / np.where(some, ws, 1.0), 0.0)
        GDn = np.where(some, GD / np.where(some, ws, 1.0), 0.0)
    pid = np.repeat(np.arange(P), K)
    cg = (G[pid, 0] * c[:, 0] + G[pid, 1] * c[:, 1] + G[pid, 2] * c[:, 2]) + G[pid, 3]
    if gd is not None:
        cg = cg + GDn[pid] * (zz - Dp[pid])
    S = G[:, 0] * GR.BG[0] + G[:, 1] * GR.BG[1] + G[:, 2] * GR.BG[2]
    dA = np.empty(alpha.shape[0])
    for k in range(int(K.max()) - 1 if P else -1, -1, -1):
        rows = np.nonzero(K > k)[0]
        j = start[rows] + k
        dA[j] = Ti[j] * (cg[j] - S[rows])
        S[rows] = alpha[j] * cg[j] + (1.0 - alpha[j]) * S[rows]
    t = _pair_terms(r, c, G[pid], dx, dy, u, v, ge, alpha, Ti, dA, None if gd is None else GDn[pid], D)
    total, m = np.zeros((n, t.shape[1])), np.zeros((n, t.shape[1]))
    np.add.at(total, lay["spl"], t)
    np.add.at(m, lay["spl"], np.abs(t))
    return dict(sum=total, m=m, ws=ws)


def terms32(rec, col, z, lay, width, g, gd=None, order="quadrant"):
    """(n, 9 | 10) float32: the per-splat sums of the pairs' binary32 terms, every operation rounded once in the kernel's
    order, the sums accumulated pair by pair in (pixel, list position) order."""
    assert order in ORDERS
    n = np.asarray(rec).shape[0]
    r, c, dx, dy, u, v, ge, alpha = _geometry(rec, col, lay, width, F)
    start, K, keeps = lay["start"], lay["K"], lay["keeps"]
    G, GD = _upstreams(lay, g, gd, F)
    P = start.shape[0]
    zz = np.asarray(z, F)[lay["spl"]]
    op = c[:, 3]
    Tb = np.empty(alpha.shape[0], F)   # walk 1's T before each pair
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
    t = _pair_terms(r, c, G[pid], dx, dy, u, v, ge, alpha, Ti, dA, None if gd is None else GDn[pid], F)
    assert t.dtype == F and Ti.dtype == F and S.dtype == F
    total = np.zeros((n, t.shape[1]), F)
    np.add.at(total, lay["spl"], t)
    return total


# ---- the figures a bound is made of ----------------------------------------------------------------------------------------
def ratios(got, want, m):
    """|got - want| / m per (splat, number); 0 where both are 0 (no pair, or every term exactly zero)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    with np.errstate(all="ignore"):
        return np.where(m > 0, err / np.where(m > 0, m, 1.0), np.where(err > 0, np.inf, 0.0))


def rel_l2(got, want):
    nr = np.linalg.norm(want)
    return np.linalg.norm(np.asarray(got, np.float64) - want) / nr if nr > 0 else np.linalg.norm(got)


# ---- scenes ----------------------------------------------------------------------------------------------------------------
def camera_u(w, h):
    vp, eye = O.camera(aspect=w / h)
    return O.uniforms(vp, eye, w, h)


def _hazy(n, seed):
    pos, scl, rot, col = ER.make_cloud(n, seed, 0.4, 0.15, degenerate=False)
    col[:, 3] = np.random.default_rng(107).uniform(0.004, 0.03, n)
    return pos, scl, rot, col


def make_scene_cloud(name):
    """(pos, scl, rot, col, w, h, seed of the upstream gradients)."""
    if name == "hazy":
        return (*_hazy(600, 7), 64, 48, 7)
    if name == "veil":  # the hazy recipe, its last fifth an opaque backdrop behind the rest
        n = 700
        pos, scl, rot, col = _hazy(n, 11)
        k = n // 5
        rng = np.random.default_rng(311)
        col[n - k:, 3] = rng.uniform(0.7, 1.0, k)
        scl[n - k:, :3] = 0.25
        pos[n - k:, :3] = rng.uniform(-0.5, 0.5, (k, 3)) * np.array([1.0, 1.0, 0.1]) - 0.6 * np.array([0.9, 1.0, 1.6])
        return pos, scl, rot, col, 64, 48, 11
    if name == "needle":
        n = 400
        pos, scl, rot, col = ER.make_cloud(n, 8, 0.5, 0.03, degenerate=False)
        rng = np.random.default_rng(208)
        axis = rng.integers(0, 3, n)
        scl[:, :3] = 0.0005
        scl[np.arange(n), axis] = np.exp(rng.uniform(np.log(0.1), np.log(3.0), n))
        return pos, scl, rot, col, 96, 64, 8
    if name == "classic":
        return (*ER.make_cloud(3000, 1, 1.0, 0.03), 160, 120, 1)
    raise KeyError(name)


def _freeze(d):
    for v in d.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def scene(name):
    """One scene's cloud, oracle lists, decisions, pair layout, upstreams, float64 terms (colour and depth) and torch autograd
    gradients (want: (n, 9), want_depth: (n, 10), in terms' column order), cond (cond(Sigma2) per splat, inf where culled).  Computed once, shared, never written to."""
    pos, scl, rot, col, w, h, seed = make_scene_cloud(name)
    n = pos.shape[0]
    u = camera_u(w, h)
    rec, proj, keys = ER.project(u, pos, scl, rot)
    _, order = NO.sort_pairs(keys, np.arange(keys.shape[0], dtype=np.uint32))
    counts, offsets, idx = NO.bin_sorted(proj, order, w, h, TILE)
    z = np.ascontiguousarray(proj[:, 4])
    dec = GR.decisions(rec, col, idx, counts, offsets, w, h)
    lay = pair_layout(dec["steps"], counts, w)
    g = GR.upstream(w, h, dec["rim"], dec["near"], seed)
    t64 = terms64(rec, col, z, lay, w, g)
    ws = np.zeros(w * h)
    ws[lay["upix"]] = t64["ws"]
    gd = DR.upstream_depth(ws.reshape(h, w), dec["rim"], dec["near"], seed)
    t64d = terms64(rec, col, z, lay, w, g, gd)
    wr, wc = GR.composite_grads(rec, col, dec["steps"], w, h, g)
    dr, dc, dz = DR.composite_depth_grads(rec, col, z, dec["steps"], w, h, g, gd)
    reached = np.zeros(n, bool)
    reached[lay["spl"]] = True
    cond = GR.sigma2_cond(u, pos, scl, rot)
    return _freeze(dict(name=name, n=n, w=w, h=h, u=u, pos=pos, scl=scl, rot=rot, col=col, rec=rec, proj=proj, z=z, counts=counts,
                        offsets=offsets, idx=idx, dec=dec, lay=_freeze(lay), g=g, gd=gd, reached=reached, cond=cond,
                        sum64=t64["sum"], m=t64["m"], sum64_depth=t64d["sum"], m_depth=t64d["m"],
                        want=np.concatenate([wr[:, REC_COLS], wc], axis=1),
                        want_depth=np.concatenate([dr[:, REC_COLS], dc, dz[:, None]], axis=1)))


@functools.lru_cache(maxsize=None)
def restated(name, order, depth):
    """terms32 on a scene under one update order: dict(sum32, c (the scene's constant: the largest |sum32 - autograd| / m over
    reached splats and numbers), l2 (per number, sum32's relative L2 against autograd))."""
    s = scene(name)
    want, m = (s["want_depth"], s["m_depth"]) if depth else (s["want"], s["m"])
    s32 = terms32(s["rec"], s["col"], s["z"], s["lay"], s["w"], s["g"], s["gd"] if depth else None, order)
    q = ratios(s32, want, m)
    return _freeze(dict(sum32=s32, c=float(q.max()), worst=int(np.argmax(q.max(axis=0))),
                        l2=np.array([rel_l2(s32[:, k], want[:, k]) for k in range(want.shape[1])])))
