"""CPU tests of the depth-map gradient contract of ellipsoid frames: the float64 depth map (tests/ellipsoid_depth_grad_ref.py)
against the binary32 one, torch.autograd.gradcheck on it, the second walk's centred depth channel against autograd, and the
bindings of the three depth entry points."""
import os
import re

import numpy as np
import pytest
import torch

from oracle import np_oracle as NO
from oracle import oracle as O
from tests import ellipsoid_depth_grad_ref as DR
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("splat_composite_aov_depth", "splat_composite_backward_depth", "splat_project_ellipsoid_backward_depth")


def scene(n, w, h, seed, spread=1.0, scale=0.03, degenerate=True):
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale, degenerate)
    vp, eye = O.camera(aspect=w / h)
    u = O.uniforms(vp, eye, w, h)
    rec, proj, keys = ER.project(u, pos, scl, rot)
    _, order = NO.sort_pairs(keys, np.arange(n, dtype=np.uint32))
    counts, offsets, idx = NO.bin_sorted(proj, order, w, h, 16)
    return u, pos, scl, rot, col, rec, proj, counts, offsets, idx


def test_depth_map_matches_binary32():
    n, w, h = 1500, 96, 80
    u, pos, scl, rot, col, rec, proj, counts, offsets, idx = scene(n, w, h, 3)
    z = proj[:, 4]
    ref = ER.composite(rec, col, z, idx, counts, offsets, w, h)
    dec = GR.decisions(rec, col, idx, counts, offsets, w, h)
    _, _, _, ws, D = DR.composite_depth64(torch.tensor(rec, dtype=torch.float64), torch.tensor(col, dtype=torch.float64),
                                          torch.tensor(z, dtype=torch.float64), dec["steps"], w, h)
    D, ws = D.numpy().reshape(h, w), ws.numpy().reshape(h, w)
    assert np.array_equal(np.isposinf(D), np.isposinf(ref["depth"]))
    m = np.isfinite(D) & (ws > 1e-3)
    assert m.sum() > w * h // 4
    assert np.abs(D[m] - ref["depth"][m]).max() <= 1e-5 * np.abs(ref["depth"][m]).max()
    assert np.abs(ws - ref["alpha"]).max() <= 1e-5
    # the ProjectedSplat depth is |p - eye|
    z64 = DR.depth64(u, torch.tensor(pos, dtype=torch.float64)).numpy()
    kept = ~GR.culled(u, pos, scl, rot)
    assert np.abs(z64[kept] - z[kept]).max() <= 1e-6 * np.abs(z64[kept]).max()


def test_gradcheck_depth():
    n, w, h = 60, 32, 32
    u, pos, scl, rot, col, rec, proj, counts, offsets, idx = scene(n, w, h, 5, spread=0.3, scale=0.08, degenerate=False)
    dec = GR.decisions(rec, col, idx, counts, offsets, w, h)
    assert sum(s[0].size for s in dec["steps"]) > 100
    r = torch.tensor(rec, dtype=torch.float64, requires_grad=True)
    c = torch.tensor(col, dtype=torch.float64, requires_grad=True)
    z = torch.tensor(proj[:, 4], dtype=torch.float64, requires_grad=True)
    rng = np.random.default_rng(0)
    gd = torch.tensor(rng.uniform(-1, 1, w * h))

    def f(r, c, z):
        _, _, _, ws, D = DR.composite_depth64(r, c, z, dec["steps"], w, h)
        some = ws > 0
        return torch.where(some, D, torch.zeros_like(D)) * gd
    # (fast mode: random projections of the Jacobian, not all of its 780 columns one by one)
    assert torch.autograd.gradcheck(f, (r, c, z), eps=1e-6, atol=1e-5, rtol=1e-4, fast_mode=True)


def test_gradcheck_depth64():
    n = 20
    pos, _, _, _ = ER.make_cloud(n, 9, 0.5, 0.05, degenerate=False)
    vp, eye = O.camera(aspect=1.0)
    u = O.uniforms(vp, eye, 64, 64)
    P = torch.tensor(pos[:, :3], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda p: DR.depth64(u, p), (P,), eps=1e-6, atol=1e-8, rtol=1e-6)


def _lists(kind, rng):
    L = int(rng.integers(1, 24))
    col = rng.uniform(0, 1, (L, 3))
    if kind == "random":
        alpha = rng.uniform(0, 0.6, L)
        z = rng.uniform(1, 10, L)
    elif kind == "opaque":  # the stop entry has alpha 1: T_L = 0, and the walk must not divide by 1 - alpha there
        alpha = rng.uniform(0, 0.5, L)
        alpha[-1] = 1.0
        z = rng.uniform(1, 10, L)
    else:  # coincident depths: D = z_i, the centred channel is exactly 0
        alpha = rng.uniform(0, 0.6, L)
        z = np.full(L, rng.uniform(1, 10))
    return alpha, col, z


@pytest.mark.parametrize("kind", ["random", "opaque", "coincident"])
def test_walk2_centred_channel_is_autograds(kind):
    rng = np.random.default_rng({"random": 1, "opaque": 2, "coincident": 3}[kind])
    for _ in range(40):
        alpha, col, z = _lists(kind, rng)
        G = rng.uniform(-1, 1, 4)
        GD = float(rng.uniform(-1, 1))
        got = DR.walk2(alpha, col, z, G, GD)
        want = DR.pixel64(alpha, col, z, G, GD)
        for a, b in zip(got, want):
            assert np.abs(a - b).max() <= 1e-10 * max(1.0, np.abs(b).max()), (kind, np.abs(a - b).max())
        if kind == "coincident":  # no depth term reaches alpha: G_D's gradient there is G_D w_i / ws alone
            dA0, _, _ = DR.walk2(alpha, col, z, G, 0.0)
            assert np.abs(got[0] - dA0).max() <= 1e-12


def _header_text():
    text = open(os.path.join(ROOT, "include", "splat.h")).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_depth_entry_points_are_declared_and_bound():
    text = _header_text()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), f"{name} not declared in splat.h"
    from splat_renderer_amd import _lib
    for name in NEW:
        assert name in _lib.SIGNATURES, name
    assert len(_lib.SIGNATURES["splat_composite_aov_depth"][1]) == len(_lib.SIGNATURES["splat_composite_aov"][1]) + 2
    assert len(_lib.SIGNATURES["splat_composite_backward_depth"][1]) == len(_lib.SIGNATURES["splat_composite_backward"][1]) + 4
    assert len(_lib.SIGNATURES["splat_project_ellipsoid_backward_depth"][1]) == len(_lib.SIGNATURES["splat_project_ellipsoid_backward"][1]) + 1
    src = open(os.path.join(ROOT, "splat_renderer_amd", "napi", "splat_napi.c")).read()
    exported = set(re.findall(r"EXPORT\(([a-z0-9_]+)\)", src.split("napi_property_descriptor d[]")[1]))
    for name in NEW:
        assert name[len("splat_"):] in exported, name


def test_depth_entry_points_are_exported():
    import ctypes as C
    import __graft_entry__ as g
    from splat_renderer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    lib = C.CDLL(_lib.LIB_PATH)
    assert [n for n in NEW if not hasattr(lib, n)] == []
