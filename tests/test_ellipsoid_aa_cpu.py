"""The 2D Mip filter's factor rho (include/splat.h, "antialiased frames") on the CPU: the binary32 restatement the GPU tests
compare against (tests/ellipsoid_aa_ref.py) is itself checked here, against closed forms and against float64."""
import numpy as np
import torch

from oracle import oracle as O
from tests import ellipsoid_aa_ref as AR
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER

F = np.float32


def camera_u(w, h):
    vp, eye = O.camera(aspect=w / h)
    return O.uniforms(vp, eye, w, h)


def _t64(a):
    return torch.tensor(np.asarray(a, np.float64))


def test_restatement_shares_the_projectors_sums():
    """a0 + 0.3, b, c0 + 0.3 rebuild ellipsoid_ref.records()'s B bit for bit: rho is formed from the record's own numbers."""
    pos, scl, rot, _ = ER.make_cloud(3000, 1)
    u = camera_u(160, 120)
    a0, b, c0 = AR.abc32(u, pos, scl, rot)
    rec = ER.records(u, pos, scl, rot)
    live = (rec != 0).any(axis=1)
    with np.errstate(all="ignore"):
        a, c = a0 + F(0.3), c0 + F(0.3)
        det = a * c - b * b
        b00, b01, b11 = np.sqrt(c / det) / F(3), ((-b) / np.sqrt(c * det)) / F(3), (F(1) / np.sqrt(c)) / F(3)
    for k, v in ((2, b00), (3, b01), (5, b11)):
        assert np.array_equal(rec[live, k].view(np.uint32), v[live].astype(F).view(np.uint32))


def test_isotropic_splat_on_the_axis():
    """rho = v / (v + 0.3), v = (focal s / depth)^2 the screen variance of an isotropic splat on the optical axis."""
    w, h = 64, 64
    u = camera_u(w, h)
    m = np.asarray(u, np.float64)
    focal = 0.5 * w * np.sqrt(m[0] ** 2 + m[4] ** 2 + m[8] ** 2)
    depth = m[15]  # clip w of the origin, which the camera looks at
    for v in (0.02, 0.1, 0.3, 1.0, 4.0, 20.0):
        s = np.sqrt(v) * depth / focal
        pos = np.array([[0, 0, 0, 1]], F)
        scl = np.array([[s, s, s, 0]], F)
        rot = np.array([[0.3, -0.5, 0.2, 0.7]], F)
        got = float(AR.rho32(u, pos, scl, rot)[0])
        assert abs(got - v / (v + 0.3)) <= 2e-5 * v / (v + 0.3), (v, got)
        got64 = float(AR.rho64(u, _t64(pos), _t64(scl), _t64(rot), np.ones(1, bool))[0])
        assert abs(got64 - v / (v + 0.3)) <= 1e-6


def test_rho_is_at_most_one_and_zero_where_culled():
    for n, seed, spread, scale in ((3000, 1, 1.0, 0.03), (20000, 2, 1.0, 0.02), (500, 3, 0.5, 0.2), (10000, 4, 1.5, 0.01)):
        pos, scl, rot, _ = ER.make_cloud(n, seed, spread, scale)
        u = camera_u(160, 120)
        rho = AR.rho32(u, pos, scl, rot)
        assert np.isfinite(rho).all() and (rho >= 0).all() and (rho <= 1).all()
        cull = GR.culled(u, pos, scl, rot)
        assert cull[[2, 3, 4, 5]].all() and (rho[cull] == 0).all()
        assert rho[0] == 0 and rho[7] == 0  # a point and a flat splat: nothing under the dilation
        assert (rho[~cull] > 0).sum() > n // 2


def test_binary32_agrees_with_float64_on_well_conditioned_splats():
    pos, scl, rot, _ = ER.make_cloud(3000, 1)
    u = camera_u(160, 120)
    rho = AR.rho32(u, pos, scl, rot)
    cull = GR.culled(u, pos, scl, rot)
    good = (GR.sigma2_cond(u, pos, scl, rot) <= 1e4) & ~cull & (rho > 0)
    assert good.sum() > 1000
    r64 = AR.rho64(u, _t64(pos), _t64(scl), _t64(rot), ~cull).numpy()
    # det0 = a0 c0 - b^2 loses up to log2(cond) bits to cancellation: at cond <= 1e4 a relative 1e4 * 2^-24 per rounding, four
    # roundings, halved by the square root: 1.2e-3 of rho <= 1; 3e-3 is that with margin
    assert np.abs(rho[good] - r64[good]).max() <= 3e-3
    assert np.median(np.abs(rho[good] - r64[good]) / r64[good]) <= 1e-6


def test_energy_identity():
    """rho sqrt(det Sigma2) = sqrt(det(Sigma2 - 0.3 I)): the compensated splat holds the undilated one's energy."""
    pos, scl, rot, _ = ER.make_cloud(3000, 1)
    u = camera_u(160, 120)
    a0, b, c0 = (x.astype(np.float64) for x in AR.abc32(u, pos, scl, rot))
    rho = AR.rho32(u, pos, scl, rot).astype(np.float64)
    det = (a0 + 0.3) * (c0 + 0.3) - b * b
    det0 = a0 * c0 - b * b
    ok = rho > 0
    lhs, rhs = rho[ok] * np.sqrt(det[ok]), np.sqrt(np.maximum(det0[ok], 0))
    good = GR.sigma2_cond(u, pos, scl, rot)[ok] <= 1e4
    assert (np.abs(lhs[good] - rhs[good]) <= 3e-3 * np.sqrt(det[ok][good])).all()  # (the bound above, times sqrt(det))
    assert np.median(np.abs(lhs[good] - rhs[good]) / rhs[good]) <= 1e-6


def test_sampling_rate_restatement():
    """A centred pinhole of focal f sees a point at depth z on its axis at rate f / z; behind near and outside the margin it
    does not."""
    w, h = 64, 48
    u = camera_u(w, h)
    m = np.asarray(u, np.float64)
    focal = 0.5 * w * np.sqrt(m[0] ** 2 + m[4] ** 2 + m[8] ** 2)
    eye = m[16:19]
    pos = np.array([[0, 0, 0, 1], list(eye + (eye - 0) * 0.5) + [1], [40, 0, 0, 1], [np.nan, 0, 0, 1]], F)
    rate, seen = AR.sampling_rate(u, focal, 0.2, 0.15, pos, np.zeros(4, F))
    assert seen.tolist() == [True, False, False, False]
    assert abs(rate[0] - focal / m[15]) <= 1e-5 * focal / m[15] and (rate[1:] == 0).all()
    again, _ = AR.sampling_rate(u, 0.5 * focal, 0.2, 0.15, pos, rate)
    assert np.array_equal(again, rate)  # a smaller rate does not lower the maximum
