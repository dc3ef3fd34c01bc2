"""CPU tests of the camera set (tests/cameras.py): the references the GPU tests of tests/test_gpu_ellipsoid_cameras.py hold the
kernels to are proven under every camera first — the binary32 restatement against the float64 finite-difference derivation,
torch.autograd.gradcheck of the float64 records and depth — and the set is held to its purpose: one camera without a zero among
the 12 VP entries the frame reads, and per camera and scene the caps that keep a GPU test from passing on nothing (pixels the
image tests skip, rows the gradient tests keep, splats on screen, a tile list longer than the composite backward's chunk)."""
import numpy as np
import pytest
import torch

from oracle import np_oracle as NO
from tests import cameras as CAMS
from tests import ellipsoid_camera_grad_ref as CR
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER
from tests.test_ellipsoid_cpu import screen64, sigma2_64

W, H = 160, 120
MAX_EXCLUDED = 0.10   # of the frame's pixels may be rim | near (skipped by the image tests)
MIN_ON_SCREEN = 400   # splats whose 3 sigma box meets the screen
GCH = 64              # composite_grad.hip's staged chunk: one tile list must be longer, so the composite backward's chunk loop turns over
# the scenes tests/test_gpu_ellipsoid_cameras.py renders and differentiates: name -> (n, w, h, seed, spread, scale, degenerate)
SCENES = {
    "frames": (3000, W, H, 1, 1.0, 0.03, True),
    "chain": (3000, W, H, 7, 1.0, 0.03, False),
}
# the clouds its projector and backward tests run on beside "frames" (no image: the row conditions only)
ROW_SCENES = {"large": (20000, 333, 200, 2, 1.0, 0.02, True)}


def _t64(a):
    return torch.as_tensor(np.asarray(a, np.float64))


def test_the_set_is_the_named_one_and_its_blocks_are_finite():
    cams = CAMS.cameras(W, H)
    assert tuple(cams) == CAMS.NAMES
    for name, u in cams.items():
        assert u.shape == (22,) and u.dtype == np.float32 and np.isfinite(u).all(), name
        assert u[20] == W and u[21] == H and u[19] == 0, name
    assert set(CAMS.pinhole_params(W, H)) == set(CAMS.PINHOLES)
    # COLMAP's first camera: the eye is the origin, negative zeros as -(R^T t) gives them
    e = cams["pinhole_at_origin"][16:19]
    assert (e == 0).all() and np.signbit(e).all()


def test_the_default_orbit_is_blind_where_another_camera_is_not():
    """The reason for the set: the default block has zeros among the 12 entries of VP the frame reads (rows 0, 1, 3), and at
    least one other camera has none."""
    cams = CAMS.cameras(W, H)
    zeros = {name: [k for k in CR.VP_ROWS_013 if abs(float(u[k])) < 1e-12] for name, u in cams.items()}
    print("VP entries that are zero:", zeros)
    assert set(zeros["orbit_default"]) >= {4, 12, 13}
    full = [name for name, z in zeros.items() if name != "orbit_default" and not z]
    assert full, zeros
    assert "pinhole_rolled_offaxis" in full and "general_vp" in full
    # general_vp is no rigid pose: its upper 3 x 3 of rows 0, 1, 3 does not have the pinhole's orthogonal rows
    m = cams["general_vp"][:16].astype(np.float64).reshape(4, 4).T
    assert abs(float(m[0, :3] @ m[3, :3])) > 1e-3 * np.linalg.norm(m[0, :3]) * np.linalg.norm(m[3, :3])


@pytest.mark.parametrize("name", CAMS.NAMES)
def test_records_against_float64_derivation(name):
    """tests/test_ellipsoid_cpu.py's check under every camera, with its bounds: the quadratic form within 1e-4 relative of the
    float64 finite-difference one, the centre within 1e-3 px — on the splats whose centre is on the screen or within one screen
    of it (a binary32 centre 2^13 px out has an ulp of 1e-3 px itself; the camera inside the cloud has those)."""
    u = CAMS.camera(name, W, H)
    n, _, _, seed, spread, scale, _ = SCENES["frames"]
    pos, scl, rot, _ = ER.make_cloud(n, seed, spread, scale)
    rec = ER.records(u, pos, scl, rot)
    live = (rec != 0).any(axis=1) & (scl[:, :3].max(axis=1) <= 1)
    near_screen = (rec[:, 0] > -W) & (rec[:, 0] < 2 * W) & (rec[:, 1] > -H) & (rec[:, 1] < 2 * H)
    rows = np.nonzero(live & near_screen)[0][:150]
    assert rows.size >= 100, rows.size
    rng = np.random.default_rng(0)
    worst_q = worst_c = 0.0
    for i in rows:
        p64 = pos[i, :3].astype(np.float64)
        S2 = sigma2_64(u, p64, scl[i, :3], rot[i])
        c = screen64(u, p64)
        worst_c = max(worst_c, float(np.abs(rec[i, :2] - c).max()))
        B = np.array([[rec[i, 2], rec[i, 3]], [rec[i, 4], rec[i, 5]]], np.float64)
        inv = np.linalg.inv(S2)
        for d in rng.normal(0, 5, (8, 2)):
            want = d @ inv @ d
            worst_q = max(worst_q, abs(9 * np.sum((B @ d) ** 2) - want) / want)
            assert abs(9 * np.sum((B @ d) ** 2) - want) <= 1e-4 * want + 1e-9, (name, i)
    print(f"{name}: {rows.size} splats, quadratic form within {worst_q:.3g} relative, centre within {worst_c:.3g} px")
    assert worst_c <= 1e-3, (name, worst_c)


def _handful(u, count, seed=5):
    """`count` splats the camera keeps and whose Sigma2 is well conditioned."""
    pos, scl, rot, _ = ER.make_cloud(400, seed, 1.0, 0.04, degenerate=False)
    rows = np.nonzero(~GR.culled(u, pos, scl, rot) & (GR.sigma2_cond(u, pos, scl, rot) <= 1e4))[0][:count]
    assert rows.size == count
    return pos[rows], scl[rows], rot[rows]


@pytest.mark.parametrize("name", CAMS.NAMES)
def test_gradcheck_of_the_records_with_respect_to_the_splats(name):
    """test_gradcheck_records_and_sh's check of GR.records64, with its tolerances, under every camera."""
    u = CAMS.camera(name, W, H)
    pos, scl, rot = _handful(u, 6)
    keep = np.ones(6, bool)
    P = torch.tensor(pos[:, :3], dtype=torch.float64, requires_grad=True)
    S = torch.tensor(scl[:, :3], dtype=torch.float64, requires_grad=True)
    Q = torch.tensor(rot, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda p, s, q: GR.records64(u, GR._v(p, 4, 1.0), GR._v(s), q, keep), (P, S, Q), eps=1e-7, atol=1e-4,
                                    rtol=1e-4)


@pytest.mark.parametrize("name", CAMS.NAMES)
def test_gradcheck_of_the_records_and_depth_with_respect_to_the_camera(name):
    """test_ellipsoid_camera_grad_cpu.py's check of CR.records64 and CR.depth64, with its tolerances, under every camera; and
    under the camera with no zero entry every one of the 12 entries receives a gradient."""
    u = CAMS.camera(name, W, H)
    pos, scl, rot = _handful(u, 6)
    P, S, Q = _t64(pos), _t64(scl), _t64(rot)
    k = np.ones(6, bool)
    U = CR.utensor(u)

    def f(uu):
        return CR.records64(uu, P, S, Q, k)[:, [0, 1, 2, 3, 5]], CR.depth64(uu, P)
    head = U.detach()[:20].clone().requires_grad_()
    assert torch.autograd.gradcheck(lambda v: f(torch.cat([v, U.detach()[20:]])), (head,), eps=1e-6, atol=1e-6, rtol=1e-5)
    rec, z = f(U)
    g_rec, = torch.autograd.grad(rec.sum(), U, retain_graph=True)
    g_z, = torch.autograd.grad(z.sum(), U)
    assert (g_rec[CR.VP_ROW_2] == 0).all() and (g_rec[16:] == 0).all() and (g_rec[CR.VP_ROWS_013] != 0).all()
    assert (g_z[:16] == 0).all() and (g_z[19:] == 0).all() and (g_z[16:19] != 0).all()
    # the constant-camera restatement is the same function
    assert torch.equal(CR.records64(CR.utensor(u, False), P, S, Q, k), GR.records64(u, P, S, Q, k))


def conditions(u, pos, scl, rot, col, w, h, image=True):
    """The figures section 4 of the camera tests' contract caps, from the references alone."""
    n = pos.shape[0]
    rec, proj, keys = ER.project(u, pos, scl, rot)
    cull = GR.culled(u, pos, scl, rot)
    assert np.array_equal(cull, ~(rec != 0).any(axis=1))
    good = (GR.sigma2_cond(u, pos, scl, rot) <= 1e4) & ~cull
    bnd, ok = NO.disc_bounds(rec)
    on = ok & (bnd[:, 2] > 0) & (bnd[:, 0] < w) & (bnd[:, 3] > 0) & (bnd[:, 1] < h)
    out = dict(n=n, live=int((~cull).sum()), culled=int(cull.sum()), good=int(good.sum()), on_screen=int(on.sum()))
    if image:
        _, order = NO.sort_pairs(keys, np.arange(n, dtype=np.uint32))
        counts, offsets, idx = NO.bin_sorted(proj, order, w, h, 16)
        c = ER.composite(rec, col, proj[:, 4], idx, counts, offsets, w, h, 16, True)
        out.update(pairs=int(idx.shape[0]), longest=int(counts.max()), excluded=float((c["rim"] | c["near"]).mean()))
    return out


@pytest.mark.parametrize("scene", list(SCENES))
@pytest.mark.parametrize("name", CAMS.NAMES)
def test_conditions_of_the_rendered_scenes(name, scene):
    n, w, h, seed, spread, scale, degenerate = SCENES[scene]
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale, degenerate)
    c = conditions(CAMS.camera(name, w, h), pos, scl, rot, col, w, h)
    print(f"{name} / {scene}: {c}")
    assert c["excluded"] <= MAX_EXCLUDED, c
    assert c["good"] >= n / 3, c
    assert c["on_screen"] >= MIN_ON_SCREEN and c["longest"] > GCH, c


@pytest.mark.parametrize("scene", list(ROW_SCENES))
@pytest.mark.parametrize("name", CAMS.NAMES)
def test_conditions_of_the_projected_clouds(name, scene):
    n, w, h, seed, spread, scale, degenerate = ROW_SCENES[scene]
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale, degenerate)
    c = conditions(CAMS.camera(name, w, h), pos, scl, rot, col, w, h, image=False)
    print(f"{name} / {scene}: {c}")
    assert c["good"] >= n / 3 and c["on_screen"] >= MIN_ON_SCREEN, c


# ---- the splat at the eye ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_a_splat_at_the_eye_has_no_direction_in_the_references(degree, dtype):
    """ER.sh_colors, GR.sh_colors64 and CR.sh_colors64 restate the rule: direction (0, 0, 0) where |p - eye| is not a positive
    finite number; every other row as before; no gradient through the direction of that row."""
    n, row = 40, 17
    rng = np.random.default_rng(degree)
    pos, _, _, _ = ER.make_cloud(n, 3, degenerate=False)
    nb = (degree + 1) ** 2
    sh = rng.normal(0, 0.5, (n, nb, 3)).astype(np.float32)
    op = rng.uniform(0, 1, n).astype(np.float32)
    for eye in (np.array([-0.0, -0.0, -0.0], np.float32), np.array([1.3, 1.4, 2.3], np.float32)):
        away = ER.sh_colors(eye, pos, sh, degree, op, dtype=dtype)
        at = pos.copy()
        at[row, :3] = eye + 0.0
        assert not ER.has_direction(eye, at)[row] and ER.has_direction(eye, at).sum() == n - 1
        got = ER.sh_colors(eye, at, sh, degree, op, dtype=dtype)
        assert np.isfinite(got).all()
        others = np.arange(n) != row
        assert np.array_equal(got[others], away[others])
        want = np.maximum(0.5 + ER.SH_C0 * sh[row, 0].astype(np.float64), 0)
        assert np.allclose(got[row, :3], want, rtol=0, atol=1e-6) and got[row, 3] == op[row]
        # the float64 references: the same values, finite gradients, zeros for that row's position and nothing for the eye from it
        passed = ER.sh_colors(eye, at, sh, degree, op, dtype=np.float32)[:, :3] > 0
        P = torch.tensor(at[:, :3].astype(np.float64), requires_grad=True)
        SH = torch.tensor(sh.astype(np.float64), requires_grad=True)
        E = torch.tensor(eye.astype(np.float64), requires_grad=True)
        g = _t64(rng.uniform(-1, 1, (n, 4)))
        out_g = GR.sh_colors64(eye.astype(np.float64), P, SH, degree, _t64(op), passed)
        out_c = CR.sh_colors64(E, P.detach(), SH.detach(), degree, _t64(op), passed)
        assert torch.equal(out_g.detach(), out_c.detach()) and torch.isfinite(out_g).all()
        (out_g * g).sum().backward()
        assert torch.isfinite(SH.grad).all() and (SH.grad[row, 1:] == 0).all()
        assert torch.allclose(SH.grad[row, 0], ER.SH_C0 * g[row, :3] * torch.as_tensor(passed[row], dtype=torch.float64))
        if degree > 0:
            assert torch.isfinite(P.grad).all() and (P.grad[row] == 0).all()
            (out_c * g).sum().backward()
            keep = torch.as_tensor(others)
            assert torch.isfinite(E.grad).all() and torch.allclose(E.grad, -P.grad[keep].sum(dim=0), rtol=1e-12, atol=1e-14)
