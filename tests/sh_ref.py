"""The SH colour kernels' test scene, float32 restatements and error measures (splat_sh_colors, splat_sh_colors_backward and
splat_sh_colors_backward_camera of include/splat.h).  No GPU.

The float64 references are the suite's own: ER.sh_colors (forward), GR.sh_colors64 and CR.sh_colors64 differentiated by
torch.autograd (backward).  What is added here:

  scene()      inputs at trained-scene magnitudes and distances, the six axis directions among them;
  forward32()  the forward and the backward restated in NumPy float32 in the kernels' operation order, one rounding per
  backward32() operator.  They serve only to size the bounds: a GPU test allows the kernel 3 times what the restatement loses on
               the same inputs (FMA contraction, another rounding of 1 / len);
  *_units()    the error measures, formed in float64, in units of 2^-24 (one binary32 rounding) of each output's own
               conditioning:
                 colour           |d| / (0.5 + sum_k |Y_k| |sh_kc|)
                 grad_sh[k, c]    |d| / (|g_c| (|Y_k| + |grad Y_k|))         (|Y_k| alone vanishes at Y_k's zero crossings, where
                                                                              the direction's rounding still moves Y_k)
                 grad_positions   max_xyz |d| / ((1 / |p - eye|) sum_k (sum_c |g_c| |sh_kc|) |grad Y_k|)   per splat
               with g_c zeroed where the forward clamped.  Where a denominator is 0 (a clamped channel; degree 0's positions) the
               output must be +-0: the measure is 0 there if it is and inf if it is not.

grad Y_k is the gradient of the basis polynomial in R^3, by complex-step differentiation of ER.sh_basis (exact for a
polynomial), so the measures depend on no second typed-in copy of the basis."""
import numpy as np
import torch

from tests import ellipsoid_camera_grad_ref as CR
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER

F = np.float32
UNIT = 2.0 ** -24
EYE = np.array([0.3, -0.2, 0.5], F)
AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], np.float64)
N_AXIS_ROWS = 600
EDGE_GAP = 64.0  # scene(): no channel closer than this many colour units to the clamp's edge (the edge is test (d)'s)


class Scene:
    """eye (3,), pos (n, 3), sh (n, nb, 3), op (n,), g (n, 4): float32."""

    def __init__(self, degree, eye, pos, sh, op, g):
        self.degree, self.eye, self.pos, self.sh, self.op, self.g = degree, eye, pos, sh, op, g
        self.n, self.nb = pos.shape[0], (degree + 1) ** 2

    def rows(self, n):
        return Scene(self.degree, self.eye, self.pos[:n], self.sh[:n], self.op[:n], self.g[:n])


def direction64(eye, pos):
    """(dir (n, 3), len (n,)) of the binary32 inputs in float64; (0, 0, 0) where the kernels see no direction."""
    v = np.asarray(pos, np.float64)[:, :3] - np.asarray(eye, np.float64)[None, :3]
    ln = np.sqrt((v * v).sum(axis=1))
    ok = ER.has_direction(eye, pos)
    with np.errstate(all="ignore"):
        d = np.where(ok[:, None], v / np.where(ok, ln, 1.0)[:, None], 0.0)
    return d, ln


def basis64(d, degree):
    """(Y (n, nb), |grad Y| (n, nb)) at directions d (n, 3): ER.sh_basis and the norm of its gradient in R^3 (complex step)."""
    d = np.asarray(d, np.float64)
    Y = ER.sh_basis(d, degree)
    h = 1e-30
    G = np.zeros(Y.shape + (3,))
    for j in range(3):
        dc = d.astype(np.complex128)
        dc[:, j] += 1j * h
        G[:, :, j] = ER.sh_basis(dc, degree, dtype=np.complex128).imag / h
    return Y, np.sqrt((G * G).sum(axis=2))


def scene(degree, n, seed):
    """The SH tests' inputs: directions uniform on the sphere (the first 600 rows the six axis directions, where several basis
    functions and their derivatives are exactly zero), |p - eye| log-uniform in [1e-3, 1e3], coefficients N(0, 1) exp(N(-1, 1.5))
    per splat, opacity uniform in [0, 1], upstream uniform in [-1, 1]^4.  A channel whose float64 colour lies within EDGE_GAP units
    of the clamp's edge gets its constant coefficient moved by 0.01, so every forward agrees on the clamp."""
    rng = np.random.default_rng([seed, degree, 1234])
    nb = (degree + 1) ** 2
    d = rng.standard_normal((n, 3))
    d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
    k = min(n, N_AXIS_ROWS)
    d[:k] = AXES[np.arange(k) % 6]
    r = np.exp(rng.uniform(np.log(1e-3), np.log(1e3), n))
    pos = (EYE.astype(np.float64)[None, :] + d * r[:, None]).astype(F)
    pos[:k][d[:k] == 0] = np.broadcast_to(EYE, (k, 3))[d[:k] == 0]  # exactly on the axis through the eye
    sh = (rng.standard_normal((n, nb, 3)) * np.exp(rng.normal(-1.0, 1.5, (n, 1, 1)))).astype(F)
    op = rng.uniform(0, 1, n).astype(F)
    g = rng.uniform(-1, 1, (n, 4)).astype(F)
    sc = Scene(degree, EYE.copy(), pos, sh, op, g)
    for _ in range(4):
        near = np.abs(edge_distance_units(sc)) < EDGE_GAP
        if not near.any():
            break
        sc.sh[:, 0, :][near] += F(0.01)
    assert not (np.abs(edge_distance_units(sc)) < EDGE_GAP).any()
    return sc


def edge_distance_units(sc):
    """(n, 3) signed distance of the float64 colour 0.5 + sum_k Y_k sh_kc from the clamp's edge, in colour units."""
    Y, _ = basis64(direction64(sc.eye, sc.pos)[0], sc.degree)
    s = sc.sh.astype(np.float64)
    return (0.5 + np.einsum("nk,nkc->nc", Y, s)) / (0.5 + np.einsum("nk,nkc->nc", np.abs(Y), np.abs(s))) / UNIT


def edge_scene(degree, seed):
    """Channels on the clamp's edge, max(0.5 + sum, 0) at sum = -0.5.  Degree 0: 3 600 rows whose sh_0c is the binary32 nearest
    -0.5 / C0 and its neighbours +-1 .. +-4 ulp.  Degrees 1-3: rows of scene() (those whose sum has not cancelled below a tenth of
    its terms), one channel's coefficients rescaled so that the float64 sum is -0.5 (1 + j 2^-23), j in [-8, 8], before the
    coefficients are rounded to binary32."""
    if degree == 0:
        sc = scene(0, 3600, seed)
        s0 = np.array(-0.5 / ER.SH_C0, F)
        j = (np.arange(sc.n * 3) % 9 - 4).reshape(sc.n, 3)
        sc.sh[:, 0, :] = (s0.view(np.uint32).astype(np.int64) + j).astype(np.uint32).view(F)
        return sc
    sc = scene(degree, 6000, seed)
    Y, _ = basis64(direction64(sc.eye, sc.pos)[0], degree)
    s = sc.sh.astype(np.float64)
    c = np.arange(sc.n) % 3
    col = s[np.arange(sc.n), :, c]  # (n, nb): the chosen channel's coefficients
    S, A = (Y * col).sum(axis=1), (np.abs(Y) * np.abs(col)).sum(axis=1)
    keep = np.abs(S) >= 0.1 * A
    j = np.arange(sc.n) % 17 - 8
    t = -0.5 * (1 + j * 2.0 ** -23) / np.where(keep, S, 1.0)
    sc.sh[np.arange(sc.n), :, c] = (col * t[:, None]).astype(F)
    k = np.nonzero(keep)[0]
    return Scene(degree, sc.eye, sc.pos[k], sc.sh[k], sc.op[k], sc.g[k])


def edge_counts(sc, units=4.0):
    """(channels above the edge, channels below it) among those whose float64 colour is within `units` of it."""
    d = edge_distance_units(sc)
    return int(((d > 0) & (d <= units)).sum()), int(((d < 0) & (d >= -units)).sum())


# ---- float64 references ---------------------------------------------------------------------------------------------------------
def colors64(sc):
    """(n, 4) float64: ER.sh_colors."""
    return ER.sh_colors(sc.eye, sc.pos, sc.sh, sc.degree, sc.op)


def backward64(sc, passed):
    """(grad_sh (n, nb, 3), grad_positions (n, 3), grad_opacity (n,)) float64: GR.sh_colors64 under torch.autograd, the clamp held
    at `passed` (n, 3)."""
    P = torch.tensor(sc.pos.astype(np.float64), requires_grad=True)
    SH = torch.tensor(sc.sh.astype(np.float64), requires_grad=True)
    OP = torch.tensor(sc.op.astype(np.float64), requires_grad=True)
    out = GR.sh_colors64(sc.eye.astype(np.float64), P, SH, sc.degree, OP, np.asarray(passed))
    (out * torch.as_tensor(sc.g.astype(np.float64))).sum().backward()
    gp = P.grad.numpy() if P.grad is not None else np.zeros((sc.n, 3))
    return SH.grad.numpy(), gp, OP.grad.numpy()


def grad_eye64(sc, passed):
    """(3,) float64 dL/deye: CR.sh_colors64 under torch.autograd."""
    E = torch.tensor(sc.eye.astype(np.float64), requires_grad=True)
    out = CR.sh_colors64(E, torch.as_tensor(sc.pos.astype(np.float64)), torch.as_tensor(sc.sh.astype(np.float64)), sc.degree,
                         torch.as_tensor(sc.op.astype(np.float64)), np.asarray(passed))
    (out * torch.as_tensor(sc.g.astype(np.float64))).sum().backward()
    return E.grad.numpy()


# ---- float32 restatements (to size the bounds) ---------------------------------------------------------------------------------
def _direction32(eye, pos):
    with np.errstate(all="ignore"):
        v = [pos[:, j] - eye[j] for j in range(3)]
        ln = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        ok = (ln > 0) & (ln < np.inf)
        il = np.where(ok, F(1) / np.where(ok, ln, F(1)), F(0)).astype(F)
        return [np.where(ok, c * il, F(0)).astype(F) for c in v], il


def _basis32(x, y, z, degree):
    """Y and dY/dx, dY/dy, dY/dz, lists of (n,) float32, in sh.hip's and splat_grad.hip's operation order."""
    c = F
    C0, C1, C2, C3 = c(ER.SH_C0), c(ER.SH_C1), [c(v) for v in ER.SH_C2], [c(v) for v in ER.SH_C3]
    o = np.zeros_like(x)
    full = lambda v: np.full_like(x, v)  # noqa: E731
    Y, X, Yy, Z = [full(C0)], [o], [o], [o]
    if degree > 0:
        Y += [-C1 * y, C1 * z, -C1 * x]
        X += [o, o, full(-C1)]
        Yy += [full(-C1), o, o]
        Z += [o, full(C1), o]
    if degree > 1:
        xx, yy, zz = x * x, y * y, z * z
        Y += [C2[0] * (x * y), C2[1] * (y * z), C2[2] * ((c(2) * zz - xx) - yy), C2[3] * (x * z), C2[4] * (xx - yy)]
        X += [C2[0] * y, o, c(-2) * C2[2] * x, C2[3] * z, c(2) * C2[4] * x]
        Yy += [C2[0] * x, C2[1] * z, c(-2) * C2[2] * y, o, c(-2) * C2[4] * y]
        Z += [o, C2[1] * y, c(4) * C2[2] * z, C2[3] * x, o]
    if degree > 2:
        Y += [C3[0] * (y * (c(3) * xx - yy)), C3[1] * ((x * y) * z), C3[2] * (y * ((c(4) * zz - xx) - yy)),
              C3[3] * (z * ((c(2) * zz - c(3) * xx) - c(3) * yy)), C3[4] * (x * ((c(4) * zz - xx) - yy)), C3[5] * (z * (xx - yy)),
              C3[6] * (x * (xx - c(3) * yy))]
        X += [C3[0] * c(6) * x * y, C3[1] * y * z, c(-2) * C3[2] * x * y, c(-6) * C3[3] * x * z, C3[4] * ((c(4) * zz - c(3) * xx) - yy),
              c(2) * C3[5] * x * z, C3[6] * c(3) * (xx - yy)]
        Yy += [C3[0] * c(3) * (xx - yy), C3[1] * x * z, C3[2] * ((c(4) * zz - xx) - c(3) * yy), c(-6) * C3[3] * y * z, c(-2) * C3[4] * x * y,
               c(-2) * C3[5] * y * z, c(-6) * C3[6] * x * y]
        Z += [o, C3[1] * x * y, c(8) * C3[2] * y * z, C3[3] * ((c(6) * zz - c(3) * xx) - c(3) * yy), c(8) * C3[4] * x * z, C3[5] * (xx - yy), o]
    return Y, X, Yy, Z


def _sums32(Y, sh):
    s = np.zeros((sh.shape[0], 3), F)
    for k, Yk in enumerate(Y):
        s = s + Yk[:, None] * sh[:, k, :]
    return s + F(0.5)


def sums32(sc):
    """(n, 3) float32: 0.5 + sum_k Y_k sh_kc before the clamp, the forward kernel's operations, one rounding each."""
    (x, y, z), _ = _direction32(sc.eye, sc.pos)
    return _sums32(_basis32(x, y, z, sc.degree)[0], sc.sh)


def forward32(sc):
    """(n, 4) float32: max(sums32, 0) and the opacity."""
    return np.concatenate([np.maximum(sums32(sc), F(0)), sc.op[:, None]], axis=1).astype(F)


def backward32(sc, passed=None):
    """(grad_sh (n, nb, 3), grad_positions (n, 3)) float32: the backward kernel's operations, one rounding each; the clamp is its
    own float32 forward's unless `passed` (n, 3) is given."""
    (x, y, z), il = _direction32(sc.eye, sc.pos)
    Y, X, Yy, Z = _basis32(x, y, z, sc.degree)
    if passed is None:
        passed = _sums32(Y, sc.sh) > 0
    gm = np.where(passed, sc.g[:, :3], F(0)).astype(F)
    gsh = np.stack([Yk[:, None] * gm for Yk in Y], axis=1)
    gx, gy, gz = np.zeros_like(x), np.zeros_like(x), np.zeros_like(x)
    for k in range(sc.nb):
        gY = (gm[:, 0] * sc.sh[:, k, 0] + gm[:, 1] * sc.sh[:, k, 1]) + gm[:, 2] * sc.sh[:, k, 2]
        gx, gy, gz = gx + gY * X[k], gy + gY * Yy[k], gz + gY * Z[k]
    dg = (x * gx + y * gy) + z * gz
    gp = np.stack([(gx - x * dg) * il, (gy - y * dg) * il, (gz - z * dg) * il], axis=1)
    return gsh.astype(F), gp.astype(F)


# ---- error measures ---------------------------------------------------------------------------------------------------------------
def _units(err, den):
    with np.errstate(all="ignore"):
        return np.where(den > 0, err / np.where(den > 0, den, 1.0), np.where(err == 0, 0.0, np.inf)) / UNIT


def color_units(sc, got, ref):
    """(n, 3): |got - ref| / (0.5 + sum_k |Y_k| |sh_kc|) in units of 2^-24."""
    Y, _ = basis64(direction64(sc.eye, sc.pos)[0], sc.degree)
    den = 0.5 + np.einsum("nk,nkc->nc", np.abs(Y), np.abs(sc.sh.astype(np.float64)))
    return _units(np.abs(np.asarray(got, np.float64)[:, :3] - np.asarray(ref, np.float64)[:, :3]), den)


def grad_sh_units(sc, got, ref, passed):
    """(n, nb, 3): |got - ref| / (|g_c| (|Y_k| + |grad Y_k|)), g_c zeroed where not `passed`."""
    Y, Gn = basis64(direction64(sc.eye, sc.pos)[0], sc.degree)
    gm = np.where(passed, np.abs(sc.g[:, :3].astype(np.float64)), 0.0)
    den = (np.abs(Y) + Gn)[:, :, None] * gm[:, None, :]
    return _units(np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64)), den)


def grad_pos_units(sc, got, ref, passed):
    """(n,): max_xyz |got - ref| / ((1 / |p - eye|) sum_k (sum_c |g_c| |sh_kc|) |grad Y_k|), g_c zeroed where not `passed`."""
    d, ln = direction64(sc.eye, sc.pos)
    _, Gn = basis64(d, sc.degree)
    gm = np.where(passed, np.abs(sc.g[:, :3].astype(np.float64)), 0.0)
    w = np.einsum("nc,nkc->nk", gm, np.abs(sc.sh.astype(np.float64)))
    with np.errstate(all="ignore"):
        den = np.where(ER.has_direction(sc.eye, sc.pos), (w * Gn).sum(axis=1) / ln, 0.0)
    return _units(np.abs(np.asarray(got, np.float64)[:, :3] - np.asarray(ref, np.float64)[:, :3]).max(axis=1), den)
