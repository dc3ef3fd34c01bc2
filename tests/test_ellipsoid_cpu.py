"""CPU tests of the anisotropic Gaussian footprint's contract (SPLAT_FOOTPRINT_ELLIPSOID): the NumPy restatement
(tests/ellipsoid_ref.py) against independent float64 derivations, the SH basis, the PLY loader, and the declarations."""
import math
import os
import re

import numpy as np
import pytest

from oracle import np_oracle as NO
from tests import ellipsoid_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cam(w=320, h=240):
    vp, eye = NO.camera(aspect=w / h)
    u = np.zeros(22, np.float32)
    u[:16], u[16:19], u[20], u[21] = vp, eye, w, h
    return u


def quat_mat(q):
    w, x, y, z = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def screen64(u, p):
    m = np.asarray(u[:16], np.float64).reshape(4, 4).T  # column-major VP
    c = m @ np.append(p, 1.0)
    return np.array([0.5 * u[20] * (1 + c[0] / c[3]), 0.5 * u[21] * (1 - c[1] / c[3])])


def sigma2_64(u, p, s, q):
    """Sigma2 from a central-difference Jacobian of the screen map, in float64."""
    J = np.zeros((2, 3))
    for k in range(3):
        e = np.zeros(3)
        e[k] = 1e-4
        J[:, k] = (screen64(u, p + e) - screen64(u, p - e)) / 2e-4
    R = quat_mat(q)
    S3 = R @ np.diag(np.asarray(s, np.float64) ** 2) @ R.T
    return J @ S3 @ J.T + 0.3 * np.eye(2)


def test_records_against_float64_derivation():
    u = cam()
    pos, scl, rot, _ = ER.make_cloud(400, seed=5, degenerate=False)
    rec = ER.records(u, pos, scl, rot)
    bnd, ok = NO.disc_bounds(rec)
    rng = np.random.default_rng(0)
    checked = 0
    for i in np.nonzero(ok)[0][:200]:
        S2 = sigma2_64(u, pos[i, :3].astype(np.float64), scl[i, :3], rot[i])
        c = screen64(u, pos[i, :3].astype(np.float64))
        assert np.allclose(rec[i, :2], c, rtol=0, atol=1e-3)
        B = np.array([[rec[i, 2], rec[i, 3]], [rec[i, 4], rec[i, 5]]], np.float64)
        inv = np.linalg.inv(S2)
        for d in rng.normal(0, 5, (8, 2)):
            want = d @ inv @ d
            assert abs(9 * np.sum((B @ d) ** 2) - want) <= 1e-4 * want + 1e-9
        ex, ey = 3 * math.sqrt(S2[0, 0]), 3 * math.sqrt(S2[1, 1])
        assert np.allclose(bnd[i], [c[0] - ex, c[1] - ey, c[0] + ex, c[1] + ey], rtol=0, atol=2e-3 * max(1.0, ex, ey))
        checked += 1
    assert checked >= 150


def test_unit_sphere_at_the_screen_centre_is_a_circle():
    u = cam(256, 256)
    eye = u[16:19].astype(np.float64)
    dist = float(np.linalg.norm(eye))
    s = 0.05
    rec = ER.records(u, np.array([[0, 0, 0, 1]], np.float32), np.array([[s, s, s, 0]], np.float32), np.array([[1, 0, 0, 0]], np.float32))
    focal = 0.5 * 256 / math.tan(math.radians(45) / 2)
    sigma = math.sqrt((focal * s / dist) ** 2 + 0.3)  # weak perspective at the centre: J = focal / depth
    assert np.allclose(rec[0, :2], [128, 128], atol=1e-3)
    assert abs(rec[0, 3]) < 1e-6 * rec[0, 2]
    assert np.isclose(rec[0, 2], rec[0, 5], rtol=1e-5)
    assert np.isclose(1 / (3 * rec[0, 2]), sigma, rtol=2e-3)


def test_quaternion_sign_and_scale_and_roll():
    u = cam()
    pos, scl, rot, _ = ER.make_cloud(64, seed=1, degenerate=False)
    a = ER.records(u, pos, scl, rot)
    for q2 in (-rot, 2 * rot, -0.5 * rot):
        assert np.array_equal(a.view(np.uint32), ER.records(u, pos, scl, q2).view(np.uint32))
    # an ellipsoid long along the view axis's normal plane, rolled 90 degrees about the view axis: the ellipse axes swap
    uc = cam(256, 256)
    eye = uc[16:19].astype(np.float64)
    fwd = -eye / np.linalg.norm(eye)
    right = np.cross(fwd, [0, 1, 0]); right /= np.linalg.norm(right)
    up = np.cross(right, fwd)
    R = np.stack([right, up, -fwd], axis=1)  # local x = screen right, y = screen up

    def quat(Rm):
        w = math.sqrt(max(0.0, 1 + Rm[0, 0] + Rm[1, 1] + Rm[2, 2])) / 2
        return np.array([w, (Rm[2, 1] - Rm[1, 2]) / (4 * w), (Rm[0, 2] - Rm[2, 0]) / (4 * w), (Rm[1, 0] - Rm[0, 1]) / (4 * w)], np.float32)
    roll = np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1]], np.float64)
    p = np.array([[0, 0, 0, 1]], np.float32)
    s = np.array([[0.2, 0.02, 0.02, 0]], np.float32)
    b1, _ = NO.disc_bounds(ER.records(uc, p, s, quat(R)[None]))
    b2, _ = NO.disc_bounds(ER.records(uc, p, s, quat(R @ roll)[None]))
    w1, h1 = b1[0, 2] - b1[0, 0], b1[0, 3] - b1[0, 1]
    w2, h2 = b2[0, 2] - b2[0, 0], b2[0, 3] - b2[0, 1]
    assert w1 > 5 * h1 and np.isclose(w1, h2, rtol=1e-3) and np.isclose(h1, w2, rtol=1e-3)


def test_every_culling_rule():
    u = cam()
    one = lambda p=(0, 0, 0), s=(0.05, 0.05, 0.05), q=(1, 0, 0, 0): ER.records(  # noqa: E731
        u, np.array([list(p) + [1]], np.float32), np.array([list(s) + [0]], np.float32), np.array([q], np.float32))[0]
    assert (one() != 0).any()
    eye = u[16:19]
    assert (one(p=tuple(2.5 * eye)) == 0).all()            # clip w <= 0: behind the camera
    assert (one(s=(30, 30, 30)) == 0).all()                # the 3-sigma ellipsoid reaches w = 0
    assert (one(q=(0, 0, 0, 0)) == 0).all()                # a zero quaternion: not finite
    assert (one(p=(np.nan, 0, 0)) == 0).all()              # not finite
    assert (one(s=(np.inf, 0.05, 0.05)) == 0).all()        # not finite
    assert (one(s=(0, 0, 0)) != 0).any()                   # a point keeps the 0.3 px dilation


def test_sh_basis_is_orthonormal():
    nt, nph = 400, 800
    th = (np.arange(nt) + 0.5) * math.pi / nt
    ph = (np.arange(nph) + 0.5) * 2 * math.pi / nph
    T, P = np.meshgrid(th, ph, indexing="ij")
    d = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], axis=-1).reshape(-1, 3)
    wgt = (np.sin(T) * (math.pi / nt) * (2 * math.pi / nph)).reshape(-1)
    Y = ER.sh_basis(d, 3)
    G = (Y * wgt[:, None]).T @ Y
    assert np.abs(G - np.eye(16)).max() <= 1e-6 * 16 + 1e-5  # (the midpoint rule's own error on degree-6 products)
    assert np.abs(np.diag(G) - 1).max() <= 1e-4


def test_sh_degree0():
    rng = np.random.default_rng(1)
    pos = rng.normal(size=(10, 4)).astype(np.float32)
    dc = rng.normal(size=(10, 1, 3)).astype(np.float32)
    got = ER.sh_colors(np.zeros(3), pos, dc, 0, np.full(10, 0.5))
    assert np.allclose(got[:, :3], np.maximum(0.5 + ER.SH_C0 * dc[:, 0], 0)) and np.all(got[:, 3] == 0.5)


def write_ply(path, xyz, log_scale, rot, logit_opacity, sh, extra_normals=True, fmt="binary_little_endian"):
    """A 3DGS-layout PLY: f_rest channel-major.  sh: (n, K, 3) basis-major."""
    n, K = sh.shape[0], sh.shape[1]
    names = ["x", "y", "z"] + (["nx", "ny", "nz"] if extra_normals else []) + ["f_dc_0", "f_dc_1", "f_dc_2"]
    names += [f"f_rest_{j}" for j in range(3 * (K - 1))] + ["opacity", "scale_0", "scale_1", "scale_2", "rot_0", "rot_1", "rot_2", "rot_3"]
    rest = sh[:, 1:, :].transpose(0, 2, 1).reshape(n, -1)
    cols = [xyz] + ([np.zeros((n, 3))] if extra_normals else []) + [sh[:, 0, :], rest, np.asarray(logit_opacity).reshape(n, 1),
                                                                    log_scale, rot]
    data = np.concatenate([np.asarray(c, np.float32).reshape(n, -1) for c in cols], axis=1).astype("<f4")
    head = f"ply\nformat {fmt} 1.0\nelement vertex {n}\n" + "".join(f"property float {k}\n" for k in names) + "end_header\n"
    with open(path, "wb") as f:
        f.write(head.encode())
        if fmt == "ascii":
            f.write("\n".join(" ".join(str(v) for v in row) for row in data).encode())
        else:
            f.write(data.tobytes())


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_ply_round_trip(tmp_path, degree):
    from splat_renderer_amd.ply import load_gaussian_ply
    rng = np.random.default_rng(degree)
    n, K = 50, (degree + 1) ** 2
    xyz = rng.normal(size=(n, 3))
    ls = rng.normal(-3, 1, (n, 3))
    rot = rng.normal(size=(n, 4))
    lo = rng.normal(size=n)
    sh = rng.normal(size=(n, K, 3)).astype(np.float32)
    p = tmp_path / "a.ply"
    write_ply(p, xyz, ls, rot, lo, sh)
    g = load_gaussian_ply(str(p))
    assert g["degree"] == degree and g["sh"].shape == (n, K, 3)
    assert np.array_equal(g["sh"], sh)
    assert np.allclose(g["positions"], xyz.astype(np.float32))
    assert np.allclose(g["scales"], np.exp(ls.astype(np.float32)), rtol=1e-6)
    assert np.allclose(g["opacity"], 1 / (1 + np.exp(-lo.astype(np.float32))), rtol=1e-6)
    assert np.array_equal(g["rotations"], rot.astype(np.float32))


def test_ply_rejects_other_files(tmp_path):
    from splat_renderer_amd import SplatError
    from splat_renderer_amd.ply import load_gaussian_ply
    bad = tmp_path / "x.ply"
    bad.write_bytes(b"not a ply file\n")
    with pytest.raises(SplatError):
        load_gaussian_ply(str(bad))
    a = tmp_path / "ascii.ply"
    write_ply(a, np.zeros((2, 3)), np.zeros((2, 3)), np.ones((2, 4)), np.zeros(2), np.zeros((2, 1, 3), np.float32), fmt="ascii")
    with pytest.raises(SplatError):
        load_gaussian_ply(str(a))
    odd = tmp_path / "odd.ply"
    write_ply(odd, np.zeros((2, 3)), np.zeros((2, 3)), np.ones((2, 4)), np.zeros(2), np.zeros((2, 2, 3), np.float32))  # 3 f_rest
    with pytest.raises(SplatError):
        load_gaussian_ply(str(odd))


def test_entry_points_are_declared_everywhere():
    names = ["splat_project_ellipsoid", "splat_sh_colors", "splat_render_frame_ellipsoids"]
    header = open(os.path.join(ROOT, "include", "splat.h")).read()
    assert re.search(r"#define SPLAT_FOOTPRINT_ELLIPSOID 2\b", header)
    from splat_renderer_amd import _lib
    assert _lib.FOOTPRINT_ELLIPSOID == 2
    lib = _lib.load()
    napi = open(os.path.join(ROOT, "splat_renderer_amd", "napi", "splat_napi.c")).read()
    for nm in names:
        assert re.search(nm + r"\s*\(", header), nm
        assert nm in _lib.SIGNATURES and hasattr(lib, nm), nm
        assert f"EXPORT({nm[len('splat_'):]})" in napi, nm
    import splat_renderer_amd as sr
    assert hasattr(sr, "GaussianCloud") and hasattr(sr, "load_gaussian_ply")


def test_restated_bounds_match_the_c_oracle():
    from oracle import oracle as O
    u = cam()
    pos, scl, rot, _ = ER.make_cloud(200, seed=9)
    rec = ER.records(u, pos, scl, rot)
    nb, nok = NO.disc_bounds(rec)
    for i in range(rec.shape[0]):
        ok, b = O.disc_bounds(rec[i])
        assert bool(ok) == bool(nok[i])
        assert np.array_equal(np.asarray(b, np.float32).view(np.uint32), nb[i].view(np.uint32))
