"""CPU tests of fitting 2D Gaussian surfels (include/splat.h, "Density control for 2D Gaussian surfels"; splat_renderer_amd.fit's
SurfelFit; ply.load_surfel_ply / save_surfel_ply): the declarations, the restated visibility rule against a brute-force image of
the surfel's 3-sigma circle, 2DGS's in-plane split in float64, and the PLY round trip.  No GPU.  Every test prints the figures it
asserts on.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import np_oracle as NO
from oracle import oracle as O
from tests import density_ref as DR
from tests import ellipsoid_ref as ER
from tests import surfel_density_ref as SDR
from tests import surfel_ref as SR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("splat_density_accumulate_surfel", "splat_densify_plan_surfel", "splat_densify_geometry_surfel")


def test_library_header_binding_and_addon_declare_the_entry_points():
    import __graft_entry__ as g
    from splat_renderer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    dll = C.CDLL(_lib.LIB_PATH)
    assert [s for s in NEW_SYMBOLS if not hasattr(dll, s)] == []
    assert [s for s in NEW_SYMBOLS if s not in _lib.SIGNATURES] == []
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "splat.h")).read(), flags=re.S)
    assert [s for s in NEW_SYMBOLS if not re.search(r"\bint\s+" + s + r"\s*\(", header)] == []
    assert "#define SPLAT_ABI_VERSION 3" in header
    addon = open(os.path.join(ROOT, "splat_renderer_amd", "napi", "splat_napi.c")).read().split("napi_property_descriptor d[]")[1]
    assert [s for s in NEW_SYMBOLS if f"EXPORT({s[len('splat_'):]})" not in addon] == []
    # the peers' signatures: the same arguments in the same order
    for s in NEW_SYMBOLS:
        assert _lib.SIGNATURES[s] == _lib.SIGNATURES[s[:-len("_surfel")]], s
    assert _lib.load().splat_abi_version() == 3


def surfel_cloud(n, seed, w, h):
    """make_cloud read as surfels under the default camera, plus tilted surfels close to the eye: steep perspective, q and B10
    far from zero.  Returns (u, records (n, 8) float32)."""
    vp, eye = O.camera(aspect=w / h)
    u = O.uniforms(vp, eye, w, h)
    pos, scl, rot, _ = ER.make_cloud(n, seed, 1.0, 0.05, degenerate=True)
    rng = np.random.default_rng(seed + 1)
    k = n // 4
    eye = np.asarray(eye, np.float64)[:3]
    toward = -eye / np.linalg.norm(eye)  # the camera looks at the origin
    pos[16:16 + k, :3] = (eye + toward * rng.uniform(0.5, 1.0, (k, 1)) + rng.normal(0, 0.12, (k, 3))).astype(np.float32)
    scl[16:16 + k, :3] = rng.uniform(0.03, 0.09, (k, 3)).astype(np.float32)
    rec, _ = SR.records(u, pos, scl, rot)
    return u, rec


def circle_image(rec, angles):
    """(n, len(angles), 2) float64: the screen points of the record's unit circle, d = (B - t q^T)^-1 t ... solved from
    (u, v) = B d / (1 - q.d):  (B + t q^T) d = t for t = (cos, sin)."""
    r = np.asarray(rec, np.float64)
    B = r[:, 2:6].reshape(-1, 1, 2, 2)
    q = r[:, 6:8].reshape(-1, 1, 1, 2)
    t = np.stack([np.cos(angles), np.sin(angles)], axis=1).reshape(1, -1, 2, 1)
    d = np.linalg.solve(B + t * q, t)[..., 0]
    return r[:, None, 0:2] + d


def test_visibility_rule_against_the_brute_force_circle():
    """disc_bounds' box against the image of the 3-sigma circle sampled at 720 angles through the inverse of (u, v) = B d / (1 - q.d).
    The box contains every sample (to the binary32 rounding of the box: 1e-4 of its size), and every side is touched to within
    1e-3 of the box's size: 720 samples leave at most 1 - cos(0.25 deg) ~ 1e-5 of the extent between a tangent point and its
    nearest sample, the rest is the box's binary32 rounding.  And the ellipsoid's rule (density_ref.visible: q = 0, B10 = 0) is
    wrong on these records: it disagrees with the surfel rule on some of them."""
    w, h = 200, 120
    u, rec = surfel_cloud(4000, 5, w, h)
    on, radius = SDR.visible(rec, w, h)
    bnd, ok = NO.disc_bounds(rec)
    culled = ~(rec != 0).any(axis=1)
    assert culled.any() and not ok[culled].any() and not on[culled].any()
    steep = np.hypot(rec[:, 6], rec[:, 7]) * radius
    print(f"{int(ok.sum())} records with bounds of {rec.shape[0]}, {int(on.sum())} visible, {int(culled.sum())} culled; "
          f"|q| radius up to {float(steep[ok].max()):.3g}, |B10 / B00| up to {float(np.abs(rec[ok, 4] / rec[ok, 2]).max()):.3g}")
    assert (steep[ok] > 0.5).sum() >= 20 and on.sum() > 1000 and (ok & ~on).sum() > 10
    pts = circle_image(rec[ok], np.arange(720) * (2 * np.pi / 720))
    b = bnd[ok].astype(np.float64)
    size = np.maximum(b[:, 2] - b[:, 0], b[:, 3] - b[:, 1])
    lo, hi = pts.min(axis=1), pts.max(axis=1)
    outside = np.maximum.reduce([b[:, 0] - lo[:, 0], b[:, 1] - lo[:, 1], hi[:, 0] - b[:, 2], hi[:, 1] - b[:, 3]]) / size
    gap = np.maximum.reduce([lo[:, 0] - b[:, 0], lo[:, 1] - b[:, 1], b[:, 2] - hi[:, 0], b[:, 3] - hi[:, 1]]) / size
    print(f"samples outside the box by at most {float(outside.max()):.3g} of its size; a side is missed by at most {float(gap.max()):.3g}")
    assert outside.max() <= 1e-4
    assert gap.max() <= 1e-3
    assert np.array_equal(radius[ok], (np.float32(0.5) * np.fmax(bnd[ok, 2] - bnd[ok, 0], bnd[ok, 3] - bnd[ok, 1])))
    # the visible mask by brute force, away from the screen's edges by the slack above
    slack = 2e-3 * size
    surely_on = (hi[:, 0] > slack) & (lo[:, 0] < w - slack) & (hi[:, 1] > slack) & (lo[:, 1] < h - slack)
    surely_off = (hi[:, 0] < -slack) | (lo[:, 0] > w + slack) | (hi[:, 1] < -slack) | (lo[:, 1] > h + slack)
    assert on[ok][surely_on].all() and not on[ok][surely_off].any() and (surely_on | surely_off).mean() > 0.99
    old, _ = DR.visible(rec, w, h)
    differ = int((old != on).sum())
    print(f"the ellipsoid rule disagrees with the surfel rule on {differ} of {rec.shape[0]} records")
    assert differ >= 1


def test_split_children_stay_in_the_plane_and_are_standard_normal_when_whitened():
    n = 10_000                         # two children each: 20 000
    rng = np.random.default_rng(11)
    means = rng.normal(size=(n, 3))
    log_scales = rng.normal(np.log(0.05), 0.5, (n, 2))
    rot = rng.normal(size=(n, 4))
    parents = np.arange(n, dtype=np.uint32)
    rows = np.stack([parents | np.uint32(2 << 30), parents | np.uint32(3 << 30)], axis=1).reshape(-1)
    seed = 0x1234_5678_9ABC
    mu, ls = SDR.apply_geometry(rows, means, log_scales, rot, seed=seed)
    assert ls.shape == (2 * n, 2) and np.allclose(ls, np.repeat(log_scales, 2, axis=0) - np.log(1.6), rtol=0, atol=1e-15)
    R = DR.rotation_matrices(np.repeat(rot, 2, axis=0))
    local = np.einsum("nji,nj->ni", R, mu - np.repeat(means, 2, axis=0))
    sig = np.exp(np.repeat(log_scales, 2, axis=0))
    off_plane = float((np.abs(local[:, 2]) / sig.max(axis=1)).max())
    white = local[:, :2] / sig
    N = white.shape[0]
    assert N == 20_000
    mean, cov = white.mean(axis=0), np.cov(white.T, bias=True)
    print(f"|n.(child - mu)| / sigma_max <= {off_plane:.3g}; whitened children: mean {mean}, covariance {cov.tolist()} over {N}")
    assert off_plane <= 1e-12
    assert (np.abs(mean) <= 5.0 / np.sqrt(N)).all(), mean
    assert (np.abs(cov - np.eye(2)) <= 5.0 / np.sqrt(N)).all(), cov
    # the ellipsoid's first two normals, the same draw
    xi = DR.split_normals(parents, np.zeros(n, np.uint32), seed)[:, :2]
    assert np.allclose(white[0::2], xi, rtol=0, atol=1e-9)
    assert not np.allclose(mu[0::2], mu[1::2])
    assert not np.allclose(SDR.apply_geometry(rows[:100], means, log_scales, rot, seed=5)[0], mu[:100])


SURFEL_PROPS = lambda nrest: (["x", "y", "z", "nx", "ny", "nz", "f_dc_0", "f_dc_1", "f_dc_2"] + [f"f_rest_{j}" for j in range(nrest)]  # noqa: E731
                              + ["opacity", "scale_0", "scale_1", "rot_0", "rot_1", "rot_2", "rot_3"])


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_surfel_ply_round_trip(tmp_path, degree):
    import splat_renderer_amd as sr
    n, nb = 257, (degree + 1) ** 2
    rng = np.random.default_rng(degree)
    pos = rng.normal(size=(n, 3)).astype(np.float32)
    ls = rng.normal(np.log(0.05), 0.5, (n, 2)).astype(np.float32)
    rot = rng.normal(size=(n, 4)).astype(np.float32)
    lo = rng.normal(0, 2, n).astype(np.float32)
    sh = rng.normal(0, 0.3, (n, nb, 3)).astype(np.float32)
    path = str(tmp_path / "surfels.ply")
    sr.save_surfel_ply(path, pos, None, rot, None, sh, log_scales=ls, opacity_logits=lo)
    raw = open(path, "rb").read()
    head, body = raw.split(b"end_header\n", 1)
    props = [line.split()[2] for line in head.decode("ascii").splitlines() if line.startswith("property")]
    assert props == SURFEL_PROPS(3 * (nb - 1)) and len(body) == 4 * n * len(props)
    assert all(line.split()[1] == "float" for line in head.decode("ascii").splitlines() if line.startswith("property"))
    table = np.frombuffer(body, "<f4").reshape(n, len(props))
    col = {k: j for j, k in enumerate(props)}
    bits = lambda a: np.ascontiguousarray(a, np.float32).view(np.uint32)  # noqa: E731
    assert np.array_equal(bits(table[:, [col["scale_0"], col["scale_1"]]]), bits(ls)), "the raw log-scales changed"
    assert np.array_equal(bits(table[:, col["opacity"]]), bits(lo)), "the raw logits changed"
    g = sr.load_surfel_ply(path)
    assert g["degree"] == degree and g["scales"].shape == (n, 2) and g["sh"].shape == (n, nb, 3)
    for key, want in (("positions", pos), ("rotations", rot), ("sh", sh)):
        assert np.array_equal(bits(g[key]), bits(want)), key
    assert np.array_equal(bits(g["scales"]), bits(np.exp(ls.astype(np.float64)).astype(np.float32)))
    assert np.array_equal(bits(g["opacity"]), bits((1 / (1 + np.exp(-lo.astype(np.float64)))).astype(np.float32)))
    # from activated values: log and logit in float64, rounded once
    path2 = str(tmp_path / "activated.ply")
    sr.save_surfel_ply(path2, pos, g["scales"], rot, g["opacity"], sh)
    t2 = np.frombuffer(open(path2, "rb").read().split(b"end_header\n", 1)[1], "<f4").reshape(n, len(props))
    o = g["opacity"].astype(np.float64)
    assert np.array_equal(bits(t2[:, [col["scale_0"], col["scale_1"]]]), bits(np.log(g["scales"].astype(np.float64)).astype(np.float32)))
    assert np.array_equal(bits(t2[:, col["opacity"]]), bits((np.log(o) - np.log1p(-o)).astype(np.float32)))
    # each loader refuses the other's file, and says which reads it
    with pytest.raises(sr.SplatError, match=r"missing properties \['scale_2'\]"):
        sr.load_gaussian_ply(path)
    path3 = str(tmp_path / "gaussians.ply")
    sr.save_gaussian_ply(path3, pos, None, rot, None, sh, log_scales=np.concatenate([ls, ls[:, :1]], axis=1), opacity_logits=lo)
    with pytest.raises(sr.SplatError, match=r"scale_2.*load_gaussian_ply"):
        sr.load_surfel_ply(path3)
    with pytest.raises(sr.SplatError, match=r"scales \(n, 2\)"):
        sr.save_surfel_ply(path3, pos, None, rot, None, sh, log_scales=np.concatenate([ls, ls[:, :1]], axis=1), opacity_logits=lo)


@pytest.mark.parametrize("flag", ["deterministic", "antialiased", "absgrad"])
def test_surfel_fit_refuses_the_flags_it_does_not_build(flag):
    """The constructor refuses them before it touches a device."""
    import splat_renderer_amd as sr
    z = np.zeros((4, 3), np.float32)
    with pytest.raises(sr.SplatError, match=rf"SurfelFit\({flag}=True\): not built for surfels"):
        sr.SurfelFit(z, np.ones((4, 2), np.float32), np.ones((4, 4), np.float32), np.full(4, 0.5, np.float32), z, **{flag: True})
