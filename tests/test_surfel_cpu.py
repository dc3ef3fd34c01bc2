"""CPU tests of the 2D Gaussian surfel footprint's restatements (tests/surfel_ref.py) and of what the library built here
exports for it (include/splat.h, "2D Gaussian surfels").  No GPU."""
import ctypes as C
import os

import numpy as np
import torch

from oracle import np_oracle as NO
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER
from tests import surfel_ref as SR

NEW_SYMBOLS = ("splat_project_surfel", "splat_composite_surfel_depth", "splat_project_surfel_backward")


def camera_u(w, h):
    vp, eye = NO.camera(aspect=w / h)
    u = np.zeros(22, np.float32)
    u[:16], u[16:19], u[20], u[21] = vp, eye, w, h
    return u


def _kept(u, pos, scl, rot):
    rec, cw = SR.records(u, pos, scl, rot)
    return rec, cw, (rec != 0).any(axis=1)


def test_library_exports_and_binding_declares_the_surfel_entry_points():
    import __graft_entry__ as g
    from splat_renderer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    dll = C.CDLL(_lib.LIB_PATH)
    assert [s for s in NEW_SYMBOLS if not hasattr(dll, s)] == []
    assert [s for s in NEW_SYMBOLS if s not in _lib.SIGNATURES] == []
    assert _lib.FOOTPRINT_SURFEL == 3
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "splat.h")).read()
    assert "#define SPLAT_FOOTPRINT_SURFEL 3" in header


def test_degenerate_rows_are_culled():
    u = camera_u(160, 120)
    pos, scl, rot, _ = ER.make_cloud(3000, 1, 1.0, 0.03)
    rec, cw, kept = _kept(u, pos, scl, rot)
    # zero scale, w = 0 crossing, zero quaternion, NaN, behind the camera, a zero x / y scale: all zeros, and clip w 0
    assert not kept[[0, 2, 3, 4, 5, 7]].any() and (cw[~kept] == 0).all() and (cw[kept] > 0).all()
    assert np.isfinite(rec).all() and kept.sum() > 2500


def test_record_reprojects_and_depth_identity():
    """The float64 record at a pixel gives (u, v); the plane point p + u e0 + v e1 projects back onto that pixel, and its clip w
    is cw rd with rd = 1 / (1 - q.d)."""
    w, h = 64, 64
    u = camera_u(w, h)
    pos, scl, rot, _ = ER.make_cloud(500, 3, 0.5, 0.2)
    _, _, kept = _kept(u, pos, scl, rot)
    geo = SR.geometry64(u, pos, scl, rot)
    rec, cw = SR.records64(u, torch.as_tensor(pos, dtype=SR.D), torch.as_tensor(scl, dtype=SR.D), torch.as_tensor(rot, dtype=SR.D), kept)
    rec, cw = rec.numpy(), cw.numpy()
    rows = np.asarray(u, np.float64)[:16].reshape(4, 4).T
    rng = np.random.default_rng(0)
    checked = 0
    for i in np.nonzero(kept & (geo["cond"] <= 100))[0]:
        for _ in range(4):
            # a pixel inside the footprint: the image of a plane point inside the unit circle, then rounded to a pixel centre
            a, b = rng.uniform(-0.6, 0.6, 2)
            c = rows @ np.append(pos[i, :3].astype(np.float64) + a * geo["e0"][i] + b * geo["e1"][i], 1.0)
            px = np.floor(0.5 * w * (c[0] / c[3] + 1)) + 0.5
            py = np.floor(0.5 * h * (1 - c[1] / c[3])) + 0.5
            uu, vv = NO.disc_uv(rec[i], px, py)
            if not (np.isfinite(uu) and uu * uu + vv * vv <= 1):
                continue
            P = pos[i, :3].astype(np.float64) + uu * geo["e0"][i] + vv * geo["e1"][i]
            c = rows @ np.append(P, 1.0)
            sx, sy = 0.5 * w * (c[0] / c[3] + 1), 0.5 * h * (1 - c[1] / c[3])
            assert abs(sx - px) <= 1e-7 * max(w, 1) and abs(sy - py) <= 1e-7 * max(h, 1), (i, sx - px, sy - py)
            rd = 1 / (1 - (rec[i, 6] * (px - rec[i, 0]) + rec[i, 7] * (py - rec[i, 1])))
            assert abs(cw[i] * rd - c[3]) <= 1e-9 * abs(c[3]), (i, cw[i] * rd, c[3])
            checked += 1
    assert checked >= 500


def test_perspective_condition():
    """The clouds the GPU tests use exercise the perspective term q, not only the affine part."""
    for (n, w, h, seed, spread, scale, thresh, least) in ((500, 64, 64, 3, 0.5, 0.2, 0.2, 150), (3000, 160, 120, 1, 1.0, 0.03, 0.05, 300)):
        u = camera_u(w, h)
        pos, scl, rot, _ = ER.make_cloud(n, seed, spread, scale)
        _, _, kept = _kept(u, pos, scl, rot)
        geo = SR.geometry64(u, pos, scl, rot)
        c = geo["centre"]
        on = (c[:, 0] >= 0) & (c[:, 0] < w) & (c[:, 1] >= 0) & (c[:, 1] < h)
        good = kept & on & (geo["cond"] <= 100) & (geo["persp"] >= thresh)
        print(f"n={n}: kept {kept.sum()}, well-conditioned on-screen with hypot(ctw, cbw) / cw >= {thresh}: {good.sum()}")
        assert good.sum() >= least


def _small_scene(n=40, w=48, h=32, seed=5):
    u = camera_u(w, h)
    pos, scl, rot, col = ER.make_cloud(n, seed, 0.4, 0.12, degenerate=False)
    rec, cw, counts, offsets, idx = SR.lists(u, pos, scl, rot, w, h)
    dec = SR.composite(rec, col, cw, idx, counts, offsets, w, h)
    return u, rec, col, cw, dec, w, h


def test_composite_gradients_match_central_differences():
    u, rec, col, cw, dec, w, h = _small_scene()
    assert sum(s[0].size for s in dec["steps"]) > 2000 and (np.abs(rec[:, 6:]) > 1e-4).any()
    g = GR.upstream(w, h, dec["rim"], dec["near"], 5)
    rng = np.random.default_rng(6)
    gd = rng.uniform(-1, 1, (h, w))
    gd[dec["rim"] | dec["near"]] = 0
    grec, gcol, gz = SR.composite_grads(rec, col, dec["steps"], w, h, g, cw, gd)

    def L(r, c, z):
        with torch.no_grad():
            return float(SR.loss64(SR.composite64(torch.as_tensor(r), torch.as_tensor(c), dec["steps"], w, h, torch.as_tensor(z)), g, gd))
    r0, c0, z0 = rec.astype(np.float64), col.astype(np.float64), cw.astype(np.float64)
    for trial in range(6):
        dr = rng.normal(size=r0.shape) * np.maximum(np.abs(r0), 1e-3)
        dc, dz = rng.normal(size=c0.shape), rng.normal(size=z0.shape)
        if trial < 3:  # one block at a time, then all together
            dr, dc, dz = dr * (trial == 0), dc * (trial == 1), dz * (trial == 2)
        eps = 1e-6
        fd = (L(r0 + eps * dr, c0 + eps * dc, z0 + eps * dz) - L(r0 - eps * dr, c0 - eps * dc, z0 - eps * dz)) / (2 * eps)
        an = (grec * dr).sum() + (gcol * dc).sum() + (gz * dz).sum()
        assert abs(fd - an) <= 1e-6 * max(abs(an), abs(fd), 1e-3), (trial, fd, an)


def test_q_zero_upper_triangular_is_the_ellipsoid_reference():
    """With q = 0 and B10 = 0 the surfel restatement is ellipsoid_grad_ref's, to the last bit."""
    w, h, n = 64, 48, 300
    u = camera_u(w, h)
    pos, scl, rot, col = ER.make_cloud(n, 9, 0.5, 0.08)
    rec, proj, keys = ER.project(u, pos, scl, rot)
    _, order = NO.sort_pairs(keys, np.arange(n, dtype=np.uint32))
    counts, offsets, idx = NO.bin_sorted(proj, order, w, h, 16)
    dec_e = GR.decisions(rec, col, idx, counts, offsets, w, h)
    dec_s = SR.composite(rec, col, np.zeros(n, np.float32), idx, counts, offsets, w, h)
    assert np.array_equal(dec_e["rim"], dec_s["rim"]) and np.array_equal(dec_e["near"], dec_s["near"])
    assert len(dec_e["steps"]) == len(dec_s["steps"])
    for a, b in zip(dec_e["steps"], dec_s["steps"]):
        assert all(np.array_equal(x, y) for x, y in zip(a, b))
    ref = ER.composite(rec, col, np.zeros(n, np.float32), idx, counts, offsets, w, h)
    assert np.array_equal(ref["img"], dec_s["img"]) and np.array_equal(ref["alpha"], dec_s["alpha"])
    g = GR.upstream(w, h, dec_e["rim"], dec_e["near"], 9)
    want_rec, want_col = GR.composite_grads(rec, col, dec_e["steps"], w, h, g)
    got_rec, got_col = SR.composite_grads(rec, col, dec_s["steps"], w, h, g)
    assert np.array_equal(got_col, want_col)
    for k in (0, 1, 2, 3, 5):
        assert np.array_equal(got_rec[:, k], want_rec[:, k]), k


def test_surfel_normals():
    from splat_renderer_amd import autograd as AG
    pos, scl, rot, _ = ER.make_cloud(100, 45, 0.5, 0.1, degenerate=False)
    u = camera_u(64, 64)
    nrm = AG.surfel_normals(torch.tensor(rot), torch.tensor(pos[:, :3]), u[16:19]).numpy().astype(np.float64)
    geo = SR.geometry64(u, pos, scl, rot)
    want = np.cross(geo["e0"], geo["e1"])
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    want *= np.where(((pos[:, :3] - u[16:19]) * want).sum(axis=1, keepdims=True) > 0, -1.0, 1.0)
    assert np.abs(nrm - want).max() <= 1e-5
