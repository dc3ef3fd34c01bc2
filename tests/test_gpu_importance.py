"""GPU tests of the importance path through Python: splat_renderer_amd.autograd.contribution against the C ABI, and
GaussianFit.accumulate_importance / importance / prune_by_importance on an occlusion scene (what no view sees scores 0, and
pruning it changes no pixel), on the rows they keep, and through tools/compact_ply.py."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from splat_renderer_amd import _lib
from splat_renderer_amd import autograd as AG
from splat_renderer_amd.fit import PLANES, GaussianFit
from splat_renderer_amd.ply import load_gaussian_ply, save_gaussian_ply
from tests import cameras as CAM
from tests import contribution_ref as CR
from tests import ellipsoid_ref as ER
from tests import test_gpu_ellipsoid_grad as TG

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _frame(n, w, h, seed, u=None):
    pos, scl, rot, col, _ = TG._torch_scene(n, w, h, seed)
    u = TG.camera_u(w, h) if u is None else u
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")  # noqa: E731
    rec, aux = AG.project_ellipsoids(u, t(pos), t(scl), t(rot))
    return rec, t(col), aux


def test_contribution_is_the_c_abi(device):
    n, w, h = 3000, 160, 120
    rec, col, aux = _frame(n, w, h, 7)
    mask = torch.rand((h, w), device="cuda")
    got = AG.contribution(rec, col, aux, w, h, pixel_weight=mask, min_weight=0.01)
    assert isinstance(got, AG.Contribution) and got._fields == ("hits", "weight_max", "weight_sum")
    assert (got.hits.dtype, got.weight_max.dtype, got.weight_sum.dtype) == (torch.int32, torch.float32, torch.int64)
    assert all(tuple(t.shape) == (n,) for t in got)
    cx = aux.ctx
    cx.bin(aux, w, h)
    idx, cnt, off = cx.lists()
    hits = torch.zeros(n, dtype=torch.int32, device="cuda")
    wmax = torch.zeros(n, dtype=torch.float32, device="cuda")
    wsum = torch.zeros(n, dtype=torch.int64, device="cuda")
    _lib.check(cx.lib.splat_composite_contribution(cx.ctx, C.byref(TG.cfg()), col.data_ptr(), 1, rec.data_ptr(), idx, cnt, off, w, h,
                                                   mask.data_ptr(), 0.01, n, hits.data_ptr(), wmax.data_ptr(), wsum.data_ptr()), cx.ctx)
    torch.cuda.synchronize()
    want = (hits.cpu().numpy(), wmax.cpu().numpy(), wsum.cpu().numpy())
    for g, x in zip(got, want):
        assert _same_bytes(g.cpu().numpy(), x)
    assert int(want[0].astype(np.int64).sum()) > 10000 and want[1].max() > 0.1 and (want[2] > 0).sum() > 100
    # out= accumulates: a second view into the first's result
    u2 = CAM.orbit(w, h, azimuth=2.3, elevation=-0.4)
    rec2, col2, aux2 = _frame(n, w, h, 7, u2)
    alone = AG.contribution(rec2, col2, aux2, w, h, min_weight=0.01)
    alone = tuple(t.cpu().numpy() for t in alone)
    both = AG.contribution(rec2, col2, aux2, w, h, min_weight=0.01, out=got)
    assert all(b is g for b, g in zip(both, got))
    assert np.array_equal(both.hits.cpu().numpy(), want[0] + alone[0]) and np.array_equal(both.weight_sum.cpu().numpy(), want[2] + alone[2])
    assert np.array_equal(both.weight_max.cpu().numpy(), np.maximum(want[1], alone[1]))
    # no gradient is offered, and tensors that require grad are accepted
    r = AG.contribution(rec.clone().requires_grad_(), col.clone().requires_grad_(), aux, w, h)
    assert not any(t.requires_grad for t in r)
    with pytest.raises(sr.SplatError):
        AG.contribution(rec, col, aux, w, h, min_weight=-1.0)
    with pytest.raises(sr.SplatError):
        AG.contribution(rec, col, aux, w, h, pixel_weight=mask[:-1])


def test_contribution_leaves_a_pending_backward_correct(device):
    """Render, score another camera (which bins another frame's lists), then backward: the gradients of the run without the
    scoring call, bit for bit under deterministic=True."""
    n, w, h = 2000, 160, 120
    pos, scl, rot, col, sh = TG._torch_scene(n, w, h, 12)
    g_rgb = torch.rand((h, w, 3), device="cuda") * 2 - 1
    u = TG.camera_u(w, h)
    grads = []
    for score in (False, True):
        leaves = [TG._leaf(a) for a in (pos, scl, rot, col[:, 3].copy(), sh)]
        rgb, alpha = AG.render_gaussians(u, *leaves[:4], sh=leaves[4], width=w, height=h, deterministic=True)
        loss = (rgb * g_rgb).sum() + alpha.sum()
        if score:
            rec2, col2, aux2 = _frame(2500, w, h, 13, CAM.orbit(w, h, azimuth=2.3, elevation=-0.4))
            AG.contribution(rec2, col2, aux2, w, h)
        loss.backward()
        torch.cuda.synchronize()
        grads.append([t.grad.cpu().numpy().copy() for t in leaves])
    for a, b in zip(*grads):
        assert np.abs(a).max() > 0 and _same_bytes(a, b)


# ---- GaussianFit ----------------------------------------------------------------------------------------------------------------
W, H = 96, 64


def occlusion_scene():
    """An opaque wall of splats between the camera and a small cluster at the origin, and splats no camera sees: (arrays of a
    GaussianFit, kinds (n,): 0 wall, 1 hidden, 2 off screen, the two cameras)."""
    u1, u2 = CAM.orbit(W, H), CAM.orbit(W, H, azimuth=0.56, elevation=0.46)
    eye = u1[16:19].astype(np.float64)
    d = -eye / np.linalg.norm(eye)
    a = np.cross(d, [0.0, 1.0, 0.0])
    a /= np.linalg.norm(a)
    b = np.cross(d, a)
    rng = np.random.default_rng(3)
    g = (np.arange(14) - 6.5) * 0.06
    wall = (0.5 * eye)[None, :] + (g[:, None, None] * a[None, None, :] + g[None, :, None] * b[None, None, :]).reshape(-1, 3)
    hidden = rng.uniform(-0.05, 0.05, (60, 3))
    off = np.concatenate([rng.uniform(-1, 1, (20, 3)) + [40.0, 0.0, 0.0], 2.0 * eye[None, :] + rng.uniform(-0.3, 0.3, (24, 3))])
    pos = np.concatenate([wall, hidden, off]).astype(np.float32)
    kinds = np.concatenate([np.zeros(len(wall), int), np.ones(len(hidden), int), np.full(len(off), 2)])
    n = pos.shape[0]
    scl = np.where(kinds[:, None] == 0, 0.07, 0.012).astype(np.float32) * np.exp(rng.uniform(-0.1, 0.1, (n, 3))).astype(np.float32)
    rot = rng.normal(size=(n, 4)).astype(np.float32)
    op = np.where(kinds == 0, 0.999, 0.8).astype(np.float32)
    sh = rng.normal(0, 0.3, (n, 4, 3)).astype(np.float32)
    return (pos, scl, rot, op, sh), kinds, (u1, u2)


def test_what_no_view_sees_scores_zero_and_pruning_it_changes_no_pixel(device):
    arrays, kinds, cams = occlusion_scene()
    fit = GaussianFit(*arrays)
    n = fit.n
    assert 280 <= n <= 320
    for kind in ("max", "sum"):
        with pytest.raises(sr.SplatError):
            fit.importance(kind)
    with pytest.raises(sr.SplatError):
        fit.prune_by_importance(threshold=0.01)
    with torch.no_grad():
        before = [fit.render(u, W, H)[0].cpu().numpy().copy() for u in cams]
    for k, u in enumerate(cams):
        assert fit.accumulate_importance(u, W, H) == k + 1
    score = {kind: fit.importance(kind).cpu().numpy() for kind in ("max", "sum", "hits", "lightgaussian")}
    for kind, s in score.items():
        assert s.dtype == np.float32 and s.shape == (n,)
        assert (s[kinds != 0] == 0).all(), f"{kind}: a hidden or off-screen splat scored"
        assert (s[kinds == 0] > 0).sum() > 100, f"{kind}: the wall did not score"
    assert score["max"].max() <= 1.0 and score["max"].max() > 0.5
    # "sum" is weight_sum 2^-24 rounded once; "lightgaussian" its formula on the fit's own activations
    hits, wmax, wsum = (t.cpu().numpy() for t in fit._importance)
    assert np.array_equal(score["sum"], (wsum.astype(np.float64) * CR.Q).astype(np.float32)) and np.array_equal(score["max"], wmax)
    assert np.array_equal(score["hits"], hits.astype(np.uint32).astype(np.float32))
    scales, opacity = (t.detach().cpu().numpy().astype(np.float64) for t in fit._activated())
    vol = scales.prod(axis=1)
    want = hits.astype(np.float64) * opacity * np.clip(vol / np.quantile(vol, 0.9), 0, 1) ** 0.1
    assert (np.abs(score["lightgaussian"] - want) <= 1e-6 * want).all() and want.max() > 0
    no_pair = hits == 0
    assert no_pair[kinds != 0].all()
    counts = fit.prune_by_importance(threshold=float(np.nextafter(0, 1)))
    assert counts == {"pruned": int(no_pair.sum()), "kept": int((~no_pair).sum()), "n": int((~no_pair).sum())} and fit.n == counts["n"]
    assert np.array_equal(fit.means.detach().cpu().numpy(), arrays[0][~no_pair])
    with torch.no_grad():
        after = [fit.render(u, W, H)[0].cpu().numpy().copy() for u in cams]
    for x, y in zip(before, after):
        assert _same_bytes(x, y), "pruning splats in no pair changed a pixel"


def _fitted(steps=3, seed=21, n=400):
    """A fit with non-zero Adam moments: a few steps towards a random target."""
    pos, scl, rot, col, sh = TG._torch_scene(n, W, H, seed)
    fit = GaussianFit(pos, scl, rot, col[:, 3].copy(), sh, sparse=False)
    u = CAM.orbit(W, H)
    target = torch.rand((H, W, 3), device="cuda")
    for _ in range(steps):
        rgb, _ = fit.render(u, W, H)
        AG.photometric_loss(rgb, target).backward()
        fit.step()
    return fit, (u, CAM.orbit(W, H, azimuth=2.3, elevation=-0.4))


def _snapshot(fit):
    c = lambda t: t.detach().cpu().numpy().copy()  # noqa: E731
    return {name: (c(getattr(fit, name)), c(fit.m[name]), c(fit.v[name])) for name in PLANES}


@pytest.mark.parametrize("keep", [0.5, 100])
def test_kept_rows(device, tmp_path, keep):
    fit, cams = _fitted()
    n = fit.n
    fit.update_filter_3d(cams, W, H)
    assert fit.filter_3d is not None
    for u in cams:
        fit.accumulate_importance(u, W, H, min_weight=0.01)
    score = fit.importance("max").cpu().numpy()
    rows = CR.select(score, keep=keep)
    assert rows.shape[0] == (n // 2 if keep == 0.5 else 100)
    old = _snapshot(fit)
    assert all(np.abs(old[name][1]).max() > 0 and np.abs(old[name][2]).max() > 0 for name in PLANES)
    assert float(fit.denom.sum()) > 0
    counts = fit.prune_by_importance(keep=keep)
    assert counts == {"pruned": n - rows.shape[0], "kept": rows.shape[0], "n": rows.shape[0]}
    new = _snapshot(fit)
    for name in PLANES:
        for k, what in enumerate(("parameter", "first moment", "second moment")):
            assert _same_bytes(new[name][k], old[name][k][rows]), f"{name}: {what} rows differ from the kept originals"
        assert getattr(fit, name).requires_grad and getattr(fit, name).is_leaf
    # what belonged to the old rows is reset
    k = fit.n
    for plane in (fit.grad_accum, fit.denom, fit.max_radius, fit.visible):
        assert tuple(plane.shape) == (k,) and float(plane.float().abs().sum()) == 0
    assert fit._importance is None and fit.importance_views == 0 and fit.filter_3d is None and fit._frame is None
    with pytest.raises(sr.SplatError):
        fit.importance()
    # the fit goes on
    rgb, _ = fit.render(cams[0], W, H)
    AG.photometric_loss(rgb, torch.rand((H, W, 3), device="cuda")).backward()
    fit.step()
    assert all(torch.isfinite(getattr(fit, name)).all() for name in PLANES)
    path = str(tmp_path / "pruned.ply")
    fit.save_ply(path)
    assert load_gaussian_ply(path)["positions"].shape == (k, 3)


def test_structure_changes_clear_the_importance_planes(device):
    fit, cams = _fitted(steps=1)
    fit.accumulate_importance(cams[0], W, H)
    assert fit.importance_views == 1
    fit.reset_importance()
    assert fit._importance is None and fit.importance_views == 0
    for change in (lambda: fit.densify_and_prune(), lambda: fit.relocate(), lambda: fit.add_new(max_splats=fit.n + 10)):
        fit.accumulate_importance(cams[0], W, H)
        change()
        assert fit._importance is None and fit.importance_views == 0
    # between backward() and step(): the pending frame is left alone
    rgb, _ = fit.render(cams[0], W, H)
    AG.photometric_loss(rgb, torch.rand((H, W, 3), device="cuda")).backward()
    fit.accumulate_importance(cams[1], W, H)
    fit.step()


def test_compact_ply_tool(device, tmp_path):
    n = 500
    pos, scl, rot, col = ER.make_cloud(n, 31, 1.0, 0.05, degenerate=False)
    sh = np.random.default_rng(31).normal(0, 0.3, (n, 4, 3)).astype(np.float32)
    src, dst = str(tmp_path / "in.ply"), str(tmp_path / "out.ply")
    save_gaussian_ply(src, pos[:, :3], scl[:, :3], rot, col[:, 3], sh)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "compact_ply.py"), src, dst, "--keep", "0.5", "--views", "4", "--width",
                          "96", "--height", "64"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    m = re.search(r"(\d+) splats -> (\d+) splats .* PSNR of pruned against unpruned frames ([0-9.]+|inf) dB", out.stdout)
    assert m, out.stdout
    assert int(m.group(1)) == n and int(m.group(2)) == n // 2
    assert load_gaussian_ply(dst)["positions"].shape == (n // 2, 3)
    assert float(m.group(3)) > 10.0
