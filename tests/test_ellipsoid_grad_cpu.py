"""CPU tests of the gradient contract of ellipsoid frames: the torch float64 restatement (tests/ellipsoid_grad_ref.py) against
the binary32 one (tests/ellipsoid_ref.py), torch.autograd.gradcheck on it, the division argument of include/splat.h, and the
bindings of the three backward entry points."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import np_oracle as NO
from oracle import oracle as O
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("splat_composite_backward", "splat_project_ellipsoid_backward", "splat_sh_colors_backward")


def camera_u(w, h):
    vp, eye = O.camera(aspect=w / h)
    return O.uniforms(vp, eye, w, h)


def scene(n, w, h, seed, spread=1.0, scale=0.03, degenerate=True):
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale, degenerate)
    u = camera_u(w, h)
    rec, proj, keys = ER.project(u, pos, scl, rot)
    _, order = NO.sort_pairs(keys, np.arange(n, dtype=np.uint32))
    counts, offsets, idx = NO.bin_sorted(proj, order, w, h, 16)
    return u, pos, scl, rot, col, rec, counts, offsets, idx


@pytest.mark.parametrize("seed", [1, 2])
def test_restatement_matches_binary32(seed):
    n, w, h = 1500, 96, 80
    u, pos, scl, rot, col, rec, counts, offsets, idx = scene(n, w, h, seed)
    keep = ~GR.culled(u, pos, scl, rot)
    r64 = GR.records64(u, torch.tensor(pos, dtype=torch.float64), torch.tensor(scl, dtype=torch.float64),
                       torch.tensor(rot, dtype=torch.float64), keep).numpy()
    cols = [0, 1, 2, 3, 5]
    cond = GR.sigma2_cond(u, pos, scl, rot)
    good = cond <= 1e4
    # relative to the record's scale (B01 = -b / ... cancels in b = T0 . T1; its error is one of B00 / B11's size)
    scale = np.abs(r64[good][:, cols])
    scale[:, :2] = np.maximum(scale[:, :2], max(w, h))  # (a centre near 0 is as exact as one across the screen)
    scale[:, 2:] = np.maximum(scale[:, 2:], np.abs(r64[good][:, [2, 5]]).max(axis=1, keepdims=True))
    rel = np.abs(r64[good][:, cols] - rec[good][:, cols]) / np.maximum(scale, 1e-30)
    # binary32 rounds det = a c - b^2 with an error of cond(Sigma2) ulps: 1e-6 where Sigma2 is well conditioned
    assert rel[cond[good] <= 100].max() <= 1e-6 and rel.max() <= 1e-4, (rel[cond[good] <= 100].max(), rel.max())
    assert (r64[~keep] == 0).all()
    dec = GR.decisions(rec, col, idx, counts, offsets, w, h)
    ref = ER.composite(rec, col, np.zeros(n, np.float32), idx, counts, offsets, w, h)
    assert np.array_equal(dec["rim"], ref["rim"]) and np.array_equal(dec["near"], ref["near"])
    rgb, alpha = GR.composite64(torch.tensor(rec, dtype=torch.float64), torch.tensor(col, dtype=torch.float64), dec["steps"], w, h)
    assert np.abs(rgb.numpy().reshape(h, w, 3) - ref["img"][..., :3]).max() <= 1e-5
    assert np.abs(alpha.numpy().reshape(h, w) - ref["alpha"]).max() <= 1e-5


def test_composite_grads_on_a_sparse_pixel_set():
    """composite_grads over a sparse pixel set (pixels=) equals the whole-frame one with g zero elsewhere, and steps at pixels
    outside the set are not needed."""
    n, w, h = 800, 64, 48
    u, pos, scl, rot, col, rec, counts, offsets, idx = scene(n, w, h, 3)
    dec = GR.decisions(rec, col, idx, counts, offsets, w, h)
    rng = np.random.default_rng(3)
    pixels = np.sort(rng.choice(w * h, 150, replace=False))
    g = np.zeros((h, w, 4), np.float32)
    g.reshape(-1, 4)[pixels] = rng.uniform(-1, 1, (pixels.size, 4))
    want_rec, want_col = GR.composite_grads(rec, col, dec["steps"], w, h, g)
    sub = []
    for pix, s, stop in dec["steps"]:
        m = np.isin(pix, pixels)
        sub.append((pix[m], s[m], stop[m]))
    got_rec, got_col = GR.composite_grads(rec, col, sub, w, h, g, pixels=pixels)
    assert np.abs(want_col).max() > 0
    np.testing.assert_allclose(got_rec, want_rec, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(got_col, want_col, rtol=1e-12, atol=1e-14)


def test_gradcheck_composite():
    n, w, h = 60, 32, 32
    u, pos, scl, rot, col, rec, counts, offsets, idx = scene(n, w, h, 5, spread=0.3, scale=0.08, degenerate=False)
    dec = GR.decisions(rec, col, idx, counts, offsets, w, h)
    assert sum(s[0].size for s in dec["steps"]) > 100
    r = torch.tensor(rec, dtype=torch.float64, requires_grad=True)
    c = torch.tensor(col, dtype=torch.float64, requires_grad=True)
    g = torch.tensor(GR.upstream(w, h, dec["rim"], dec["near"], 0).reshape(-1, 4), dtype=torch.float64)

    def f(r, c):
        rgb, alpha = GR.composite64(r, c, dec["steps"], w, h)
        return (rgb * g[:, :3]).sum(dim=1) + alpha * g[:, 3]
    assert torch.autograd.gradcheck(f, (r, c), eps=1e-6, atol=1e-5, rtol=1e-4)


def test_gradcheck_records_and_sh():
    n, w, h = 24, 64, 64
    pos, scl, rot, _ = ER.make_cloud(n, 9, 0.5, 0.05, degenerate=False)
    u = camera_u(w, h)
    keep = ~GR.culled(u, pos, scl, rot)
    P = torch.tensor(pos[:, :3], dtype=torch.float64, requires_grad=True)
    S = torch.tensor(scl[:, :3], dtype=torch.float64, requires_grad=True)
    Q = torch.tensor(rot, dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda p, s, q: GR.records64(u, GR._v(p, 4, 1.0), GR._v(s), q, keep), (P, S, Q), eps=1e-7, atol=1e-4,
                                    rtol=1e-4)
    rng = np.random.default_rng(3)
    SH = torch.tensor(rng.normal(0, 0.3, (n, 16, 3)), requires_grad=True)
    OP = torch.tensor(rng.uniform(0.2, 1, n), requires_grad=True)
    passed = np.ones((n, 3), bool)
    assert torch.autograd.gradcheck(lambda p, sh, op: GR.sh_colors64(u[16:19], p, sh, 3, op, passed), (P, SH, OP), eps=1e-7, atol=1e-5)


@pytest.mark.parametrize("kind", ["random", "opaque", "coincident"])
def test_every_non_last_consumed_entry_leaves_more_than_one_percent(kind):
    """1 - alpha > 0.01 for every consumed entry but a pixel's stopping one: T_{i+1} > 0.01 and T_{i+1} <= 1 - alpha_i."""
    n, w, h = 800, 64, 64
    pos, scl, rot, col = ER.make_cloud(n, 13, 0.4, 0.06, degenerate=False)
    if kind in ("opaque", "coincident"):
        col[:, 3] = 1.0
    if kind == "coincident":
        pos[: n // 2, :3] = pos[0, :3]
        scl[: n // 2] = scl[0]
    u = camera_u(w, h)
    rec, proj, keys = ER.project(u, pos, scl, rot)
    _, order = NO.sort_pairs(keys, np.arange(n, dtype=np.uint32))
    counts, offsets, idx = NO.bin_sorted(proj, order, w, h, 16)
    dec = GR.decisions(rec, col, idx, counts, offsets, w, h)
    stops = 0
    for (_pix, _s, stop), a in zip(dec["steps"], dec["alpha"]):
        assert (np.float32(1) - a[~stop] > 0.01).all()
        stops += int(stop.sum())
    assert stops > 0
    if kind != "random":
        assert max(float(a[stop].max(initial=0)) for (_p, _s, stop), a in zip(dec["steps"], dec["alpha"])) > 0.99


def test_bindings_declare_the_backward_entry_points():
    from splat_renderer_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES
    src = open(os.path.join(ROOT, "splat_renderer_amd", "napi", "splat_napi.c")).read()
    exported = set(re.findall(r"EXPORT\(([a-z0-9_]+)\)", src.split("napi_property_descriptor d[]")[1]))
    assert {n[len("splat_"):] for n in NEW} <= exported
    header = open(os.path.join(ROOT, "include", "splat.h")).read()
    assert all(re.search(rf"\bint {n}\(", header) for n in NEW)


def test_render_gaussians_refuses_cpu_tensors():
    import splat_renderer_amd as sr
    from splat_renderer_amd import autograd as AG
    u = camera_u(64, 64)
    x = torch.zeros((4, 3))
    with pytest.raises(sr.SplatError):
        AG.render_gaussians(u, x, x, torch.zeros((4, 4)), torch.zeros(4), colors=x, width=64, height=64)
    with pytest.raises(sr.SplatError):
        AG.project_ellipsoids(u, x, x, torch.zeros((4, 4)), 64, 64)
