"""GPU tests of the depth map of ellipsoid frames and its gradients (splat_composite_aov_depth, splat_composite_backward_depth,
splat_project_ellipsoid_backward_depth and the depth paths of splat_renderer_amd.autograd) against the float64 restatement
(tests/ellipsoid_depth_grad_ref.py).

Upstream gradients are random in [-1, 1] and zero on the pixels ellipsoid_ref.composite marks rim or near, so both sides
differentiate the same function (the cut and the early-out stop held fixed); the depth's upstream is also zero where
sum w < 1e-3."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from splat_renderer_amd import _lib
from tests import ellipsoid_depth_grad_ref as DR
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER
from tests import test_gpu_ellipsoid as TE
from tests import test_gpu_ellipsoid_grad as TG

pytestmark = pytest.mark.gpu

CASES = TG.CASES
REC_COLS = TG.REC_COLS
rel_l2 = TG.rel_l2


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _scene(n, w, h, seed, spread, scale):
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale)
    u = TG.camera_u(w, h)
    _, proj, _ = ER.project(u, pos, scl, rot)
    rec, counts, offsets, idx = TG.lists(u, pos, scl, rot, w, h)
    return u, pos, scl, rot, col, rec, proj, counts, offsets, idx


def composite_backward_depth(device, rec, col, z, counts, offsets, idx, w, h, g, gd, c=None):
    d = device
    n = rec.shape[0]
    bufs = [d.createBufferFrom(np.ascontiguousarray(a)) for a in (rec, col, idx if idx.size else np.zeros(1, np.uint32), counts, offsets, g,
                                                                  z, gd)]
    grec, gcol, gz = d.createBuffer(n * 32), d.createBuffer(n * 16), d.createBuffer(n * 4)
    for b in (grec, gcol, gz):
        b.zero()
    rc = d.lib.splat_composite_backward_depth(d.ctx, C.byref(c or TG.cfg()), bufs[1].ptr, 1, bufs[0].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr,
                                              w, h, bufs[5].ptr, n, grec.ptr, gcol.ptr, bufs[6].ptr, 1, bufs[7].ptr, gz.ptr)
    out = (rc, grec.read(np.float32).reshape(n, 8), gcol.read(np.float32).reshape(n, 4), gz.read(np.float32)) if rc == 0 else \
        (rc, None, None, None)
    for b in bufs + [grec, gcol, gz]:
        b.destroy()
    return out


# ---- (a) the forward -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,w,h,seed,spread,scale", CASES)
def test_composite_aov_depth(device, n, w, h, seed, spread, scale):
    u, pos, scl, rot, col, rec, proj, counts, offsets, idx = _scene(n, w, h, seed, spread, scale)
    z = np.ascontiguousarray(proj[:, 4])
    ref = ER.composite(rec, col, z, idx, counts, offsets, w, h)
    d = device
    bufs = [d.createBufferFrom(np.ascontiguousarray(a)) for a in (rec, col, idx if idx.size else np.zeros(1, np.uint32), counts, offsets, z,
                                                                  proj)]
    img0, img1, img2 = (d.createBuffer(w * h * 16) for _ in range(3))
    dep1, dep2, al, ids = (d.createBuffer(w * h * 4) for _ in range(4))
    c = TG.cfg()
    lists = (bufs[0].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, w, h, None)
    _lib.check(d.lib.splat_composite_aov(d.ctx, C.byref(c), bufs[1].ptr, 1, None, 1, *lists, img0.ptr, None, None), d.ctx)
    aov1 = _lib.Aov(dep1.ptr, al.ptr, ids.ptr)
    _lib.check(d.lib.splat_composite_aov_depth(d.ctx, C.byref(c), bufs[1].ptr, 1, None, 1, *lists, img1.ptr, None, C.byref(aov1),
                                               bufs[5].ptr, 1), d.ctx)
    # the ProjectedSplat records' own depth words: projected + 4 floats, stride 8
    aov2 = _lib.Aov(dep2.ptr, None, None)
    _lib.check(d.lib.splat_composite_aov_depth(d.ctx, C.byref(c), bufs[1].ptr, 1, None, 1, *lists, img2.ptr, None, C.byref(aov2),
                                               bufs[6].ptr + 16, 8), d.ctx)
    i0, i1, i2 = (b.read(np.float32) for b in (img0, img1, img2))
    depth1, depth2 = dep1.read(np.float32).reshape(h, w), dep2.read(np.float32).reshape(h, w)
    alpha, idv = al.read(np.float32).reshape(h, w), ids.read(np.uint32).reshape(h, w)
    for b in bufs + [img0, img1, img2, dep1, dep2, al, ids]:
        b.destroy()
    assert np.array_equal(bits(i1), bits(i0)) and np.array_equal(bits(i2), bits(i0)), "the image changed with the depth buffer"
    assert np.array_equal(bits(depth1), bits(depth2))
    TE.check_aov(alpha, idv, depth1, ref, f"aov_depth n={n}")


def _leaf(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda", requires_grad=True)


@pytest.mark.parametrize("records", ["projected", "lit"])
def test_rasterize_depth_is_the_renderers(device, records):
    from splat_renderer_amd import autograd as AG
    for (n, w, h, seed) in ((3000, 160, 120, 1), (40000, 640, 360, 5)):
        pos, scl, rot, col, _ = TG._torch_scene(n, w, h, seed)
        u = TG.camera_u(w, h)
        cloud = sr.GaussianCloud.fromArrays(device, pos, scl, rot, colors=col)
        r = sr.Renderer(device, None, "rgba8unorm", n, footprint="ellipsoid", writeProjected=True, records=records)
        r.render(u, cloud, None, None, w, h, wantFloat=True, wantAov=True)
        want_img, want_depth, want_alpha = r.readPixelsFloat(), r.readDepth(), r.readAlpha()
        r.destroy()
        cloud.destroy()
        rgb, alpha, depth = AG.render_gaussians(u, _leaf(pos), _leaf(scl), _leaf(rot), _leaf(col[:, 3]), colors=_leaf(col[:, :3]), width=w,
                                                height=h, return_depth=True)
        torch.cuda.synchronize()
        assert depth.shape == (h, w) and depth.requires_grad
        assert np.array_equal(bits(rgb.detach().cpu().numpy()), bits(want_img[..., :3])), f"n={n}: image differs"
        assert np.array_equal(bits(depth.detach().cpu().numpy()), bits(want_depth.reshape(h, w))), f"n={n}: depth differs"
        assert np.array_equal(bits(alpha.detach().cpu().numpy()), bits(want_alpha.reshape(h, w))), f"n={n}: alpha differs"
        assert np.isposinf(depth.detach().cpu().numpy()).any()
        # the depths project_ellipsoids returns are the ProjectedSplat depth word, bit for bit
        rec, depths, aux = AG.project_ellipsoids(u, _leaf(pos), _leaf(scl), _leaf(rot), return_depth=True)
        assert depths.shape == (n,) and depths.requires_grad
        assert np.array_equal(bits(depths.detach().cpu().numpy()), bits(aux.projected[:, 4].cpu().numpy()))


# ---- (b) the composite backward ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,w,h,seed,spread,scale", CASES)
def test_composite_backward_depth(device, n, w, h, seed, spread, scale):
    u, pos, scl, rot, col, rec, proj, counts, offsets, idx = _scene(n, w, h, seed, spread, scale)
    z = np.ascontiguousarray(proj[:, 4])
    dec = GR.decisions(rec, col, idx, counts, offsets, w, h)
    ref = ER.composite(rec, col, z, idx, counts, offsets, w, h)
    g = GR.upstream(w, h, dec["rim"], dec["near"], seed)
    gd = DR.upstream_depth(ref["alpha"], dec["rim"], dec["near"], seed)
    assert (gd != 0).sum() > 0
    rc, grec, gcol, gz = composite_backward_depth(device, rec, col, z, counts, offsets, idx, w, h, g, gd)
    assert rc == 0
    assert np.isfinite(grec).all() and np.isfinite(gcol).all() and np.isfinite(gz).all()
    want_rec, want_col, want_z = DR.composite_depth_grads(rec, col, z, dec["steps"], w, h, g, gd)
    checks = [(f"rec[{k}]", grec[:, k], want_rec[:, k]) for k in REC_COLS] + [(f"col[{k}]", gcol[:, k], want_col[:, k]) for k in range(4)] + \
             [("z", gz, want_z)]
    for name, got, want in checks:
        assert rel_l2(got, want) <= 1e-4, f"{name}: relative L2 {rel_l2(got, want):.3g}"
    assert (grec[:, [4, 6, 7]] == 0).all()
    # G_D = 0: the colour-only kernel's gradients (to the atomics' rounding), and no depth gradient
    rc0, grec0, gcol0 = TG.composite_backward(device, rec, col, counts, offsets, idx, w, h, g)
    rc1, grec1, gcol1, gz1 = composite_backward_depth(device, rec, col, z, counts, offsets, idx, w, h, g, np.zeros((h, w), np.float32))
    assert rc0 == 0 and rc1 == 0 and (gz1 == 0).all()
    for got, want in ((grec1, grec0), (gcol1, gcol0)):
        assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max() + 1e-30


# ---- (c) the projector -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,w,h,seed,spread,scale", CASES[:4])
def test_project_backward_depth(device, n, w, h, seed, spread, scale):
    pos, scl, rot, _ = ER.make_cloud(n, seed, spread, scale)
    u = TG.camera_u(w, h)
    rng = np.random.default_rng(seed)
    grec = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
    gz = rng.uniform(-1, 1, n).astype(np.float32)
    d = device
    up = np.ascontiguousarray(u, np.float32).ctypes.data_as(C.POINTER(C.c_float))
    bufs = [d.createBufferFrom(np.ascontiguousarray(a, np.float32)) for a in (pos, scl, rot, grec, gz, np.zeros(n, np.float32))]

    def run(depth_buf):
        outs = [d.createBuffer(n * 16) for _ in range(3)]
        args = (d.ctx, up, bufs[0].ptr, 1, bufs[1].ptr, 1, bufs[2].ptr, 1, n, bufs[3].ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr)
        rc = d.lib.splat_project_ellipsoid_backward(*args) if depth_buf is None else \
            d.lib.splat_project_ellipsoid_backward_depth(*args, depth_buf.ptr)
        assert rc == 0
        res = [o.read(np.float32).reshape(n, 4) for o in outs]
        for o in outs:
            o.destroy()
        return res
    gp, gs, gq = run(bufs[4])
    plain = run(None)
    zero = run(bufs[5])
    for b in bufs:
        b.destroy()
    for a, b in zip(zero, plain):  # grad_depth = 0: the existing entry's outputs bit for bit
        assert np.array_equal(bits(a), bits(b))
    assert np.isfinite(gp).all() and np.isfinite(gs).all() and np.isfinite(gq).all()
    cull = GR.culled(u, pos, scl, rot)
    assert cull[[2, 3, 4, 5]].all()
    assert (gp[cull] == 0).all() and (gs[cull] == 0).all() and (gq[cull] == 0).all()  # the depth term included
    P = torch.tensor(pos.astype(np.float64), requires_grad=True)
    S = torch.tensor(scl.astype(np.float64), requires_grad=True)
    Q = torch.tensor(rot.astype(np.float64), requires_grad=True)
    rec = GR.records64(u, P, S, Q, ~cull)
    z64 = DR.depth64(u, P)
    gz_kept = torch.as_tensor(np.where(cull, 0.0, gz.astype(np.float64)))
    ((rec * torch.as_tensor(grec.astype(np.float64))).sum() + (z64 * gz_kept).sum()).backward()
    good = GR.sigma2_cond(u, pos, scl, rot) <= 1e4
    assert good.sum() > n // 3
    for name, got, want in (("position", gp, P.grad.numpy()), ("scale", gs, S.grad.numpy()), ("rotation", gq, Q.grad.numpy())):
        for k in range(3 if name != "rotation" else 4):
            e = rel_l2(got[good, k], want[good, k])
            assert e <= 1e-5, f"{name}[{k}]: relative L2 {e:.3g}"
        if name != "rotation":
            assert (got[:, 3] == 0).all()
    # the depth term is there: the position gradient differs from the records-only one on kept splats
    assert np.abs(gp[~cull, :3] - plain[0][~cull, :3]).max() > 1e-3


# ---- (d) end to end --------------------------------------------------------------------------------------------------------
def _reference_chain_depth(u, pos, scl, rot, op, sh, degree, w, h, g, gd):
    rec32, counts, offsets, idx = TG.lists(u, pos, scl, rot, w, h)
    col32 = ER.sh_colors(u[16:19], pos, sh, degree, op, dtype=np.float32).astype(np.float32)
    dec = GR.decisions(rec32, col32, idx, counts, offsets, w, h)
    passed = col32[:, :3] > 0
    P = torch.tensor(pos.astype(np.float64), requires_grad=True)
    S = torch.tensor(scl.astype(np.float64), requires_grad=True)
    Q = torch.tensor(rot.astype(np.float64), requires_grad=True)
    OP = torch.tensor(op.astype(np.float64), requires_grad=True)
    SH = torch.tensor(sh.astype(np.float64), requires_grad=True)
    rec = GR.records64(u, GR._v(P, 4, 1.0), GR._v(S), Q, ~GR.culled(u, pos, scl, rot))
    col = GR.sh_colors64(u[16:19].astype(np.float64), P, SH, degree, OP, passed)
    z = DR.depth64(u, P)
    rgb, alpha, _zw, ws, D = DR.composite_depth64(rec, col, z, dec["steps"], w, h)
    gt = torch.as_tensor(g.astype(np.float64).reshape(-1, 4))
    gdt = torch.as_tensor(gd.astype(np.float64).reshape(-1))
    some = ws > 0
    Dz = torch.where(some, D, torch.zeros_like(D))
    ((rgb * gt[:, :3]).sum() + (alpha * gt[:, 3]).sum() + (Dz * torch.where(some, gdt, torch.zeros_like(gdt))).sum()).backward()
    return dict(means=P.grad.numpy(), scales=S.grad.numpy(), rotations=Q.grad.numpy(), opacities=OP.grad.numpy(), sh=SH.grad.numpy()), dec


def _upstreams(u, pos, scl, rot, col, w, h, seed):
    rec32, counts, offsets, idx = TG.lists(u, pos, scl, rot, w, h)
    _, proj, _ = ER.project(u, pos, scl, rot)
    dec = GR.decisions(rec32, col, idx, counts, offsets, w, h)
    ref = ER.composite(rec32, col, proj[:, 4], idx, counts, offsets, w, h)
    g = GR.upstream(w, h, dec["rim"], dec["near"], seed)
    gd = DR.upstream_depth(ref["alpha"], dec["rim"], dec["near"], seed)
    return g, gd


def _torch_loss(u, leaves, w, h, g, gd, degree):
    from splat_renderer_amd import autograd as AG
    rgb, alpha, depth = AG.render_gaussians(u, leaves["means"], leaves["scales"], leaves["rotations"], leaves["opacities"], sh=leaves["sh"],
                                            width=w, height=h, degree=degree, return_depth=True)
    gt, gdt = torch.as_tensor(g, device="cuda"), torch.as_tensor(gd, device="cuda")
    dz = torch.where(torch.isfinite(depth), depth, torch.zeros_like(depth))
    return (rgb * gt[..., :3]).sum() + (alpha * gt[..., 3]).sum() + (dz * gdt).sum()


def _scene_with_sh(n, w, h, seed, degree):
    pos, scl, rot, col, sh = TG._torch_scene(n, w, h, seed, degree=degree)
    # the colour the forward sees: SH towards the camera (decisions depend on the opacity only)
    return pos, scl, rot, col, sh, col[:, 3].copy()


def test_render_gaussians_depth_gradients(device):
    n, w, h, seed, degree = 3000, 160, 120, 7, 1
    pos, scl, rot, col, sh, op = _scene_with_sh(n, w, h, seed, degree)
    u = TG.camera_u(w, h)
    g, gd = _upstreams(u, pos, scl, rot, col, w, h, seed)
    want, _ = _reference_chain_depth(u, pos, scl, rot, op, sh, degree, w, h, g, gd)
    leaves = dict(means=_leaf(pos), scales=_leaf(scl), rotations=_leaf(rot), opacities=_leaf(op), sh=_leaf(sh))
    _torch_loss(u, leaves, w, h, g, gd, degree).backward()
    good = GR.sigma2_cond(u, pos, scl, rot) <= 1e4
    for name in ("means", "scales", "rotations", "opacities", "sh"):
        got = leaves[name].grad.detach().cpu().numpy()
        assert np.isfinite(got).all(), name
        rows = good if name in ("means", "scales", "rotations") else np.ones(n, bool)
        e = rel_l2(got[rows].reshape(-1), want[name][rows].reshape(-1))
        assert e <= 1e-4, f"{name}: relative L2 {e:.3g}"


# ---- (e) empty pixels --------------------------------------------------------------------------------------------------------
def test_nan_upstream_on_empty_pixels_is_not_read(device):
    from splat_renderer_amd import autograd as AG
    n, w, h = 500, 96, 64
    pos, scl, rot, col, _ = TG._torch_scene(n, w, h, 12, spread=0.5, scale=0.03)
    u = TG.camera_u(w, h)
    leaves = [_leaf(a) for a in (pos, scl, rot, col[:, 3], col[:, :3])]
    rgb, alpha, depth = AG.render_gaussians(u, *leaves[:4], colors=leaves[4], width=w, height=h, return_depth=True)
    empty = torch.isposinf(depth)
    assert 0 < int(empty.sum()) < w * h
    gd = torch.rand((h, w), device="cuda") * 2 - 1
    gd = torch.where(empty, torch.full_like(gd, float("nan")), gd)
    gd[empty.nonzero()[::2].unbind(1)] = float("inf")
    torch.autograd.backward([depth, rgb], [gd, torch.ones_like(rgb)])
    for leaf in leaves:
        assert leaf.grad is not None and torch.isfinite(leaf.grad).all()
    assert float(leaves[0].grad.abs().sum()) > 0


# ---- (f) interleaved frames ----------------------------------------------------------------------------------------------------
def test_two_forwards_then_two_backwards_with_depth(device):
    w, h, degree = 160, 120, 1
    u = TG.camera_u(w, h)
    scenes = []
    for seed, n in ((8, 2500), (9, 3500)):
        pos, scl, rot, col, sh, op = _scene_with_sh(n, w, h, seed, degree)
        g, gd = _upstreams(u, pos, scl, rot, col, w, h, seed)
        scenes.append((pos, scl, rot, op, sh, g, gd))
    runs = []
    for pos, scl, rot, op, sh, g, gd in scenes:  # two forwards: the second re-bins the shared binner
        leaves = dict(means=_leaf(pos), scales=_leaf(scl), rotations=_leaf(rot), opacities=_leaf(op), sh=_leaf(sh))
        runs.append((leaves, _torch_loss(u, leaves, w, h, g, gd, degree)))
    runs[1][1].backward()
    runs[0][1].backward()  # the first's lists are rebuilt, not the second's used
    for (pos, scl, rot, op, sh, g, gd), (leaves, _) in zip(scenes, runs):
        want, _ = _reference_chain_depth(u, pos, scl, rot, op, sh, degree, w, h, g, gd)
        good = GR.sigma2_cond(u, pos, scl, rot) <= 1e4
        for name in ("means", "opacities", "sh"):
            got = leaves[name].grad.detach().cpu().numpy()
            rows = good if name == "means" else np.ones(got.shape[0], bool)
            e = rel_l2(got[rows].reshape(-1), want[name][rows].reshape(-1))
            assert e <= 1e-4, f"{name}: relative L2 {e:.3g}"


# ---- (g) a depth-supervised fit ------------------------------------------------------------------------------------------------
def test_depth_fit_converges(device):
    """About 2 000 Gaussians at 256 x 256, their means pushed along their view rays (sigma 0.05 at a distance of about 3): 300
    Adam steps on a masked depth-only loss bring it down at least 30x, within 10 s (measured on one MI355X: 108x in 0.3 s)."""
    from splat_renderer_amd import autograd as AG
    n, w, h = 2000, 256, 256
    u = TG.camera_u(w, h)
    pos, scl, rot, col = ER.make_cloud(n, 31, 1.0, 0.04, degenerate=False)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")  # noqa: E731
    gt_pos, scales, rots, ops, cols = t(pos[:, :3]), t(scl[:, :3]), t(rot), t(col[:, 3]), t(col[:, :3])

    def frame(p):
        _, alpha, depth = AG.render_gaussians(u, p, scales, rots, ops, colors=cols, width=w, height=h, return_depth=True)
        return alpha, depth
    with torch.no_grad():
        t_alpha, t_depth = frame(gt_pos)
        mask = (t_alpha > 0.5) & torch.isfinite(t_depth)
        target = torch.where(mask, t_depth, torch.zeros_like(t_depth)).clone()
    assert int(mask.sum()) > w * h // 10
    eye = t(u[16:19])
    ray = gt_pos - eye[None, :]
    ray = ray / ray.norm(dim=1, keepdim=True)
    g = torch.Generator(device="cuda").manual_seed(6)
    means = (gt_pos + 0.05 * torch.randn((n, 1), device="cuda", generator=g) * ray).requires_grad_()
    opt = torch.optim.Adam([means], lr=2e-3)
    t0 = time.time()
    losses = []
    for _ in range(300):
        opt.zero_grad()
        _, depth = frame(means)
        diff = torch.where(mask & torch.isfinite(depth), depth - target, torch.zeros_like(depth))
        loss = (diff * diff).sum() / mask.sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    elapsed = time.time() - t0
    print(f"depth fit: loss {losses[0]:.4g} -> {losses[-1]:.4g} ({losses[0] / losses[-1]:.1f}x) in {elapsed:.1f} s")
    assert all(np.isfinite(losses)) and torch.isfinite(means).all()
    assert losses[-1] <= losses[0] / 30
    assert elapsed < 10


# ---- (h) rejections --------------------------------------------------------------------------------------------------------
def test_depth_rejections(device):
    n, w, h = 500, 64, 64
    u, pos, scl, rot, col, rec, proj, counts, offsets, idx = _scene(n, w, h, 3, 0.5, 0.05)
    z = np.ascontiguousarray(proj[:, 4])
    g = np.zeros((h, w, 4), np.float32)
    gd = np.zeros((h, w), np.float32)
    for bad in (dict(tile_size=8), dict(mode=_lib.MODE_REFERENCE_LITERAL), dict(early_out=0), dict(tile_row0=1), dict(tile_row1=2),
                dict(footprint=_lib.FOOTPRINT_DISC), dict(record_format=_lib.RECORDS_LIT32)):
        rc, _, _, _ = composite_backward_depth(device, rec, col, z, counts, offsets, idx, w, h, g, gd, TG.cfg(**bad))
        assert rc == -1, bad
    d = device
    bufs = [d.createBufferFrom(np.ascontiguousarray(a)) for a in (rec, col, idx, counts, offsets, g, z, gd)]
    out = d.createBuffer(n * 52 + 64)
    grec, gcol, gz = out.ptr, out.ptr + 32 * n, out.ptr + 48 * n
    head = (d.ctx, C.byref(TG.cfg()), bufs[1].ptr, 1, bufs[0].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, w, h, bufs[5].ptr, n, grec, gcol)
    for tail in ((None, 1, bufs[7].ptr, gz), (bufs[6].ptr + 2, 1, bufs[7].ptr, gz), (bufs[6].ptr, 0, bufs[7].ptr, gz),
                 (bufs[6].ptr, 1, None, gz), (bufs[6].ptr, 1, bufs[7].ptr + 1, gz), (bufs[6].ptr, 1, bufs[7].ptr, None),
                 (bufs[6].ptr, 1, bufs[7].ptr, gz + 2)):
        assert d.lib.splat_composite_backward_depth(*head, *tail) == -1, tail
    # the forward entry: a NULL or misaligned depth, stride 0, and splat_composite_aov's own refusals
    img, dep = d.createBuffer(w * h * 16), d.createBuffer(w * h * 4)
    aov = _lib.Aov(dep.ptr, None, None)
    lists = (bufs[0].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, w, h, None, img.ptr, None, C.byref(aov))
    for c, zp, zs in ((TG.cfg(), None, 1), (TG.cfg(), bufs[6].ptr + 2, 1), (TG.cfg(), bufs[6].ptr, 0),
                      (TG.cfg(mode=_lib.MODE_REFERENCE_LITERAL), bufs[6].ptr, 1), (TG.cfg(record_format=_lib.RECORDS_LIT32), bufs[6].ptr, 1)):
        assert d.lib.splat_composite_aov_depth(d.ctx, C.byref(c), bufs[1].ptr, 1, None, 1, *lists, zp, zs) == -1
    assert d.lib.splat_composite_aov_depth(d.ctx, C.byref(TG.cfg()), bufs[1].ptr, 1, None, 1, *lists, bufs[6].ptr, 1) == 0
    # the projector's: a misaligned or NULL grad_depth
    up = np.ascontiguousarray(u).ctypes.data_as(C.POINTER(C.c_float))
    p4 = [d.createBufferFrom(np.ascontiguousarray(a, np.float32)) for a in (pos, scl, rot)]
    for gzp in (bufs[6].ptr + 2, None):
        assert d.lib.splat_project_ellipsoid_backward_depth(d.ctx, up, p4[0].ptr, 1, p4[1].ptr, 1, p4[2].ptr, 1, n, out.ptr, out.ptr,
                                                            out.ptr, out.ptr, gzp) == -1
    torch.cuda.synchronize()
    for b in bufs + p4 + [out, img, dep]:
        b.destroy()
