"""GPU tests of the gradients of ellipsoid frames (splat_composite_backward, splat_project_ellipsoid_backward,
splat_sh_colors_backward and splat_renderer_amd.autograd) against the torch float64 restatement (tests/ellipsoid_grad_ref.py).

Upstream gradients are random in [-1, 1] and zero on the pixels ellipsoid_ref.composite marks rim or near, so both sides
differentiate the same function (the cut and the early-out stop held fixed)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from oracle import np_oracle as NO
from oracle import oracle as O
from splat_renderer_amd import _lib
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER


pytestmark = pytest.mark.gpu

CASES = [  # n, w, h, seed, spread, scale: test_gpu_ellipsoid.CASES, and a screen wider than 256 tiles
    (3000, 160, 120, 1, 1.0, 0.03),
    (20000, 333, 200, 2, 1.0, 0.02),
    (500, 64, 64, 3, 0.5, 0.2),
    (10000, 256, 256, 4, 1.5, 0.01),
    (40000, 640, 360, 5, 1.2, 0.015),
    (4000, 4200, 40, 6, 1.0, 0.03),
]
REC_COLS = (0, 1, 2, 3, 5)  # c.x, c.y, B00, B01, B11


def camera_u(w, h):
    vp, eye = O.camera(aspect=w / h)
    return O.uniforms(vp, eye, w, h)


def cfg(**kw):
    c = dict(mode=_lib.MODE_FRONT_TO_BACK, early_out=1, tile_size=16, tile_row0=0, tile_row1=_lib.U32_MAX,
             record_format=_lib.RECORDS_PROJECTED, prelit=1, footprint=_lib.FOOTPRINT_ELLIPSOID)
    c.update(kw)
    return _lib.CompositeCfg(*c.values())


def lists(u, pos, scl, rot, w, h):
    rec, proj, keys = ER.project(u, pos, scl, rot)
    _, order = NO.sort_pairs(keys, np.arange(keys.shape[0], dtype=np.uint32))
    counts, offsets, idx = NO.bin_sorted(proj, order, w, h, 16)
    return rec, counts, offsets, idx


def rel_l2(got, ref):
    nr = np.linalg.norm(ref)
    return np.linalg.norm(got - ref) / nr if nr > 0 else np.linalg.norm(got)


def composite_backward(device, rec, col, counts, offsets, idx, w, h, g, c=None):
    d = device
    n = rec.shape[0]
    bufs = [d.createBufferFrom(a) for a in (rec, col, idx if idx.size else np.zeros(1, np.uint32), counts, offsets, g)]
    grec, gcol = d.createBuffer(n * 32), d.createBuffer(n * 16)
    grec.zero()
    gcol.zero()
    rc = d.lib.splat_composite_backward(d.ctx, C.byref(c or cfg()), bufs[1].ptr, 1, bufs[0].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, w, h,
                                        bufs[5].ptr, n, grec.ptr, gcol.ptr)
    out = (rc, grec.read(np.float32).reshape(n, 8), gcol.read(np.float32).reshape(n, 4)) if rc == 0 else (rc, None, None)
    for b in bufs + [grec, gcol]:
        b.destroy()
    return out


@pytest.mark.parametrize("n,w,h,seed,spread,scale", CASES)
def test_composite_backward(device, n, w, h, seed, spread, scale):
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale)
    u = camera_u(w, h)
    rec, counts, offsets, idx = lists(u, pos, scl, rot, w, h)
    dec = GR.decisions(rec, col, idx, counts, offsets, w, h)
    ref = ER.composite(rec, col, np.zeros(n, np.float32), idx, counts, offsets, w, h)
    assert np.array_equal(dec["rim"], ref["rim"]) and np.array_equal(dec["near"], ref["near"])
    g = GR.upstream(w, h, dec["rim"], dec["near"], seed)
    rc, grec, gcol = composite_backward(device, rec, col, counts, offsets, idx, w, h, g)
    assert rc == 0
    want_rec, want_col = GR.composite_grads(rec, col, dec["steps"], w, h, g)
    assert np.isfinite(grec).all() and np.isfinite(gcol).all()
    for name, got, want in [(f"rec[{k}]", grec[:, k], want_rec[:, k]) for k in REC_COLS] + \
                           [(f"col[{k}]", gcol[:, k], want_col[:, k]) for k in range(4)]:
        assert rel_l2(got, want) <= 1e-4, f"{name}: relative L2 {rel_l2(got, want):.3g}"
        assert np.abs(got - want).max() <= 2e-3 * np.abs(want).max() + 1e-30, f"{name}: max {np.abs(got - want).max():.3g}"
    # splats no consumed pair reaches: exact zeros (and the columns no one writes)
    reached = np.zeros(n, bool)
    for _pix, s, _stop in dec["steps"]:
        reached[s] = True
    assert (grec[~reached] == 0).all() and (gcol[~reached] == 0).all()
    assert (grec[:, [4, 6, 7]] == 0).all()


def test_division_is_safe_on_adversarial_lists(device):
    """Opacity 1 and coincident centres: T reaches 0 at one entry; the backward never divides by it."""
    n, w, h = 600, 96, 64
    pos, scl, rot, col = ER.make_cloud(n, 11, 0.3, 0.05, degenerate=False)
    pos[: n // 2, :3] = pos[0, :3]
    col[:, 3] = 1.0
    u = camera_u(w, h)
    rec, counts, offsets, idx = lists(u, pos, scl, rot, w, h)
    dec = GR.decisions(rec, col, idx, counts, offsets, w, h)
    g = GR.upstream(w, h, dec["rim"], dec["near"], 11)
    rc, grec, gcol = composite_backward(device, rec, col, counts, offsets, idx, w, h, g)
    assert rc == 0 and np.isfinite(grec).all() and np.isfinite(gcol).all()
    want_rec, want_col = GR.composite_grads(rec, col, dec["steps"], w, h, g)
    for k in REC_COLS:
        assert rel_l2(grec[:, k], want_rec[:, k]) <= 1e-4
    for k in range(4):
        assert rel_l2(gcol[:, k], want_col[:, k]) <= 1e-4


@pytest.mark.parametrize("n,w,h,seed,spread,scale", CASES[:4])
def test_project_backward(device, n, w, h, seed, spread, scale):
    pos, scl, rot, _ = ER.make_cloud(n, seed, spread, scale)
    u = camera_u(w, h)
    rng = np.random.default_rng(seed)
    grec = rng.uniform(-1, 1, (n, 8)).astype(np.float32)
    d = device
    bufs = [d.createBufferFrom(np.ascontiguousarray(a, np.float32)) for a in (pos, scl, rot, grec)]
    outs = [d.createBuffer(n * 16) for _ in range(3)]
    check = d.lib.splat_project_ellipsoid_backward(d.ctx, np.ascontiguousarray(u, np.float32).ctypes.data_as(C.POINTER(C.c_float)),
                                                   bufs[0].ptr, 1, bufs[1].ptr, 1, bufs[2].ptr, 1, n, bufs[3].ptr, outs[0].ptr, outs[1].ptr,
                                                   outs[2].ptr)
    assert check == 0
    gp, gs, gq = (o.read(np.float32).reshape(n, 4) for o in outs)
    for b in bufs + outs:
        b.destroy()
    assert np.isfinite(gp).all() and np.isfinite(gs).all() and np.isfinite(gq).all()
    cull = GR.culled(u, pos, scl, rot)
    assert cull[[2, 3, 4, 5]].all()
    assert (gp[cull] == 0).all() and (gs[cull] == 0).all() and (gq[cull] == 0).all()
    P = torch.tensor(pos.astype(np.float64), requires_grad=True)
    S = torch.tensor(scl.astype(np.float64), requires_grad=True)
    Q = torch.tensor(rot.astype(np.float64), requires_grad=True)
    rec = GR.records64(u, P, S, Q, ~cull)
    (rec * torch.as_tensor(grec.astype(np.float64))).sum().backward()
    good = GR.sigma2_cond(u, pos, scl, rot) <= 1e4
    assert good.sum() > n // 3
    for name, got, want in (("position", gp, P.grad.numpy()), ("scale", gs, S.grad.numpy()), ("rotation", gq, Q.grad.numpy())):
        for k in range(3 if name != "rotation" else 4):
            e = rel_l2(got[good, k], want[good, k])
            assert e <= 1e-4, f"{name}[{k}]: relative L2 {e:.3g}"
        if name != "rotation":
            assert (got[:, 3] == 0).all()


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_sh_backward(device, degree):
    n = 5000
    rng = np.random.default_rng(degree + 20)
    pos, _, _, _ = ER.make_cloud(n, degree + 20, degenerate=False)
    nb = (degree + 1) ** 2
    sh = rng.normal(0, 0.5, (n, nb, 3)).astype(np.float32)
    op = rng.uniform(0, 1, n).astype(np.float32)
    gcol = rng.uniform(-1, 1, (n, 4)).astype(np.float32)
    eye = camera_u(64, 64)[16:19].astype(np.float32)
    d = device
    bufs = [d.createBufferFrom(a) for a in (pos, sh.reshape(n, -1), op, gcol)]
    gsh, gp, gop = d.createBuffer(n * nb * 12), d.createBuffer(n * 16), d.createBuffer(n * 4)
    rc = d.lib.splat_sh_colors_backward(d.ctx, eye.ctypes.data_as(C.POINTER(C.c_float)), bufs[0].ptr, 1, bufs[1].ptr, 3 * nb, degree,
                                        bufs[2].ptr, bufs[3].ptr, n, gsh.ptr, gp.ptr, gop.ptr)
    assert rc == 0
    got_sh, got_p, got_op = gsh.read(np.float32).reshape(n, nb, 3), gp.read(np.float32).reshape(n, 4), gop.read(np.float32)
    for b in bufs + [gsh, gp, gop]:
        b.destroy()
    passed = ER.sh_colors(eye, pos, sh, degree, op, dtype=np.float32)[:, :3] > 0
    P = torch.tensor(pos.astype(np.float64), requires_grad=True)
    SH = torch.tensor(sh.astype(np.float64), requires_grad=True)
    OP = torch.tensor(op.astype(np.float64), requires_grad=True)
    out = GR.sh_colors64(eye.astype(np.float64), P, SH, degree, OP, passed)
    (out * torch.as_tensor(gcol.astype(np.float64))).sum().backward()
    assert np.abs(got_sh - SH.grad.numpy()).max() <= 1e-5
    want_p = P.grad.numpy() if P.grad is not None else np.zeros_like(pos, np.float64)  # (degree 0 does not depend on the position)
    assert np.abs(got_p[:, :3] - want_p[:, :3]).max() <= 1e-5 and (got_p[:, 3] == 0).all()
    assert np.array_equal(got_op, gcol[:, 3])
    # where the forward clamped, no gradient reaches the coefficients of that channel
    clamped = ~passed
    assert clamped.any() or degree == 0
    assert (got_sh.transpose(0, 2, 1)[clamped] == 0).all()


# ---- the torch Functions ---------------------------------------------------------------------------------------------------
def _torch_scene(n, w, h, seed, spread=1.0, scale=0.03, degree=1):
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale, degenerate=False)
    rng = np.random.default_rng(seed)
    sh = rng.normal(0, 0.4, (n, (degree + 1) ** 2, 3)).astype(np.float32)
    return pos[:, :3].copy(), scl[:, :3].copy(), rot, col, sh


def _leaf(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda", requires_grad=True)


def test_rasterize_image_is_the_renderers(device):
    from splat_renderer_amd import autograd as AG
    for (n, w, h, seed) in ((3000, 160, 120, 1), (20000, 333, 200, 2), (40000, 640, 360, 5), (20000, 1024, 768, 6)):
        pos, scl, rot, col, _ = _torch_scene(n, w, h, seed)
        u = camera_u(w, h)
        cloud = sr.GaussianCloud.fromArrays(device, pos, scl, rot, colors=col)
        r = sr.Renderer(device, None, "rgba8unorm", n, footprint="ellipsoid")
        r.render(u, cloud, None, None, w, h, wantFloat=True)
        want = r.readPixelsFloat()
        r.destroy()
        cloud.destroy()
        rgb, alpha = AG.render_gaussians(u, _leaf(pos), _leaf(scl), _leaf(rot), _leaf(col[:, 3]), colors=_leaf(col[:, :3]), width=w, height=h)
        torch.cuda.synchronize()
        got = rgb.detach().cpu().numpy()
        assert np.array_equal(got.view(np.uint32), np.ascontiguousarray(want[..., :3]).view(np.uint32)), f"n={n}: image differs"
        assert alpha.shape == (h, w)


def _reference_chain(u, pos, scl, rot, op, sh, degree, w, h, g):
    rec32, counts, offsets, idx = lists(u, pos, scl, rot, w, h)
    col32 = ER.sh_colors(u[16:19], pos, sh, degree, op, dtype=np.float32).astype(np.float32)
    dec = GR.decisions(rec32, col32, idx, counts, offsets, w, h)
    passed = col32[:, :3] > 0
    P = torch.tensor(pos.astype(np.float64), requires_grad=True)
    S = torch.tensor(scl.astype(np.float64), requires_grad=True)
    Q = torch.tensor(rot.astype(np.float64), requires_grad=True)
    OP = torch.tensor(op.astype(np.float64), requires_grad=True)
    SH = torch.tensor(sh.astype(np.float64), requires_grad=True)
    rec = GR.records64(u, GR._v(P, 4, 1.0), GR._v(S), Q, ~GR.culled(u, pos, scl, rot))
    rec.retain_grad()
    col = GR.sh_colors64(u[16:19].astype(np.float64), P, SH, degree, OP, passed)
    rgb, alpha = GR.composite64(rec, col, dec["steps"], w, h)
    gt = torch.as_tensor(g.astype(np.float64).reshape(-1, 4))
    ((rgb * gt[:, :3]).sum() + (alpha * gt[:, 3]).sum()).backward()
    return dict(means=P.grad.numpy(), scales=S.grad.numpy(), rotations=Q.grad.numpy(), opacities=OP.grad.numpy(), sh=SH.grad.numpy(),
                rec=rec.grad.numpy()), dec


def _torch_grads(u, pos, scl, rot, op, sh, w, h, g, keep_rec=False):
    from splat_renderer_amd import autograd as AG
    leaves = dict(means=_leaf(pos), scales=_leaf(scl), rotations=_leaf(rot), opacities=_leaf(op), sh=_leaf(sh))
    rec, aux = AG.project_ellipsoids(u, leaves["means"], leaves["scales"], leaves["rotations"])
    rec.retain_grad()
    col = AG.sh_colors(u[16:19], leaves["means"], leaves["sh"], int(round(np.sqrt(sh.shape[1]))) - 1, leaves["opacities"])
    rgb, alpha = AG.rasterize(rec, col, aux, w, h)
    gt = torch.as_tensor(g, device="cuda")
    return leaves, rec, ((rgb * gt[..., :3]).sum() + (alpha * gt[..., 3]).sum())


def test_render_gaussians_gradients(device):
    n, w, h, seed, degree = 3000, 160, 120, 7, 1
    pos, scl, rot, col, sh = _torch_scene(n, w, h, seed, degree=degree)
    op = col[:, 3].copy()
    u = camera_u(w, h)
    rec32, counts, offsets, idx = lists(u, pos, scl, rot, w, h)
    dec = GR.decisions(rec32, col, idx, counts, offsets, w, h)
    g = GR.upstream(w, h, dec["rim"], dec["near"], seed)
    want, _ = _reference_chain(u, pos, scl, rot, op, sh, degree, w, h, g)
    leaves, rec, loss = _torch_grads(u, pos, scl, rot, op, sh, w, h, g)
    loss.backward()
    good = GR.sigma2_cond(u, pos, scl, rot) <= 1e4
    for name in ("means", "scales", "rotations", "opacities", "sh"):
        got = leaves[name].grad.detach().cpu().numpy()
        assert np.isfinite(got).all(), name
        rows = good if name in ("means", "scales", "rotations") else np.ones(n, bool)
        e = rel_l2(got[rows].reshape(-1), want[name][rows].reshape(-1))
        assert e <= 1e-4, f"{name}: relative L2 {e:.3g}"
    # the screen-space gradient 3DGS densification reads
    sg = rec.grad.detach().cpu().numpy()[:, :2]
    assert rel_l2(sg.reshape(-1), want["rec"][:, :2].reshape(-1)) <= 1e-4 and np.abs(sg).max() > 0


def test_two_forwards_then_two_backwards(device):
    w, h, degree = 160, 120, 1
    u = camera_u(w, h)
    scenes = []
    for seed, n in ((8, 2500), (9, 3500)):
        pos, scl, rot, col, sh = _torch_scene(n, w, h, seed, degree=degree)
        op = col[:, 3].copy()
        rec32, counts, offsets, idx = lists(u, pos, scl, rot, w, h)
        dec = GR.decisions(rec32, col, idx, counts, offsets, w, h)
        g = GR.upstream(w, h, dec["rim"], dec["near"], seed)
        scenes.append((pos, scl, rot, op, sh, g))
    first = [_torch_grads(u, *s[:5], w, h, s[5]) for s in scenes]  # two forwards: the second re-bins the shared binner
    first[1][2].backward()
    first[0][2].backward()                                          # the first's lists are rebuilt, not the second's used
    for (pos, scl, rot, op, sh, g), (leaves, _, _) in zip(scenes, first):
        want, _ = _reference_chain(u, pos, scl, rot, op, sh, degree, w, h, g)
        for name in ("opacities", "sh"):
            e = rel_l2(leaves[name].grad.detach().cpu().numpy().reshape(-1), want[name].reshape(-1))
            assert e <= 1e-4, f"{name}: relative L2 {e:.3g}"


def test_cpu_tensors_and_bad_calls_raise(device):
    from splat_renderer_amd import autograd as AG
    u = camera_u(64, 64)
    x = torch.zeros((4, 3))
    with pytest.raises(sr.SplatError):
        AG.render_gaussians(u, x, x, torch.zeros((4, 4)), torch.zeros(4), colors=x, width=64, height=64)
    with pytest.raises(sr.SplatError):
        AG.render_gaussians(u, x.cuda().double(), x.cuda(), torch.zeros((4, 4)).cuda(), torch.zeros(4).cuda(), colors=x.cuda(), width=64,
                            height=64)


def test_fitting_converges(device):
    """About 2 000 Gaussians at 256 x 256: 300 Adam steps from a perturbed cloud bring the L2 image loss down 10x."""
    from splat_renderer_amd import autograd as AG
    n, w, h = 2000, 256, 256
    u = camera_u(w, h)
    pos, scl, rot, col = ER.make_cloud(n, 31, 1.0, 0.04, degenerate=False)
    t = lambda a: torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")  # noqa: E731
    gt_pos, gt_ls, gt_rot = t(pos[:, :3]), torch.log(t(scl[:, :3])), t(rot)
    gt_ol, gt_cl = torch.logit(t(col[:, 3]).clamp(0.05, 0.95)), torch.logit(t(col[:, :3]).clamp(0.05, 0.95))

    def frame(p, ls, q, ol, cl):
        rgb, _ = AG.render_gaussians(u, p, torch.exp(ls), q, torch.sigmoid(ol), colors=torch.sigmoid(cl), width=w, height=h)
        return rgb
    with torch.no_grad():
        target = frame(gt_pos, gt_ls, gt_rot, gt_ol, gt_cl).clone()
    g = torch.Generator(device="cuda").manual_seed(5)
    params = [(gt_pos + 0.01 * torch.randn(gt_pos.shape, device="cuda", generator=g)).requires_grad_(),
              (gt_ls + 0.2 * torch.randn(gt_ls.shape, device="cuda", generator=g)).requires_grad_(),
              (gt_rot + 0.2 * torch.randn(gt_rot.shape, device="cuda", generator=g)).requires_grad_(),
              (gt_ol + 1.0 * torch.randn(gt_ol.shape, device="cuda", generator=g)).requires_grad_(),
              (gt_cl + 1.0 * torch.randn(gt_cl.shape, device="cuda", generator=g)).requires_grad_()]
    opt = torch.optim.Adam([{"params": [params[0]], "lr": 2e-4}, {"params": params[1:3], "lr": 1e-2},
                            {"params": params[3:], "lr": 5e-2}])
    t0 = time.time()
    losses = []
    for _ in range(300):
        opt.zero_grad()
        loss = ((frame(*params) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    elapsed = time.time() - t0
    print(f"fitting: loss {losses[0]:.4g} -> {losses[-1]:.4g} ({losses[0] / losses[-1]:.1f}x) in {elapsed:.1f} s")
    assert all(np.isfinite(losses)) and all(torch.isfinite(p).all() for p in params)
    assert losses[-1] <= losses[0] / 10
    assert elapsed < 30


def test_rejections(device):
    n, w, h = 500, 64, 64
    pos, scl, rot, col = ER.make_cloud(n, 3, 0.5, 0.05)
    u = camera_u(w, h)
    rec, counts, offsets, idx = lists(u, pos, scl, rot, w, h)
    g = np.zeros((h, w, 4), np.float32)
    for bad in (dict(tile_size=8), dict(mode=_lib.MODE_REFERENCE_LITERAL), dict(early_out=0), dict(tile_row0=1), dict(tile_row1=2),
                dict(footprint=_lib.FOOTPRINT_DISC), dict(record_format=_lib.RECORDS_LIT32)):
        rc, _, _ = composite_backward(device, rec, col, counts, offsets, idx, w, h, g, cfg(**bad))
        assert rc == -1, bad
    # a misaligned gradient buffer
    d = device
    bufs = [d.createBufferFrom(a) for a in (rec, col, idx, counts, offsets, g)]
    out = d.createBuffer(n * 48 + 64)
    rc = d.lib.splat_composite_backward(d.ctx, C.byref(cfg()), bufs[1].ptr, 1, bufs[0].ptr, bufs[2].ptr, bufs[3].ptr, bufs[4].ptr, w, h,
                                        bufs[5].ptr, n, out.ptr + 4, out.ptr + 32 * n + 16)
    assert rc == -1
    rc = d.lib.splat_project_ellipsoid_backward(d.ctx, np.ascontiguousarray(u).ctypes.data_as(C.POINTER(C.c_float)), bufs[0].ptr + 4, 1,
                                                bufs[0].ptr, 1, bufs[0].ptr, 1, n, bufs[0].ptr, out.ptr, out.ptr, out.ptr)
    assert rc == -1
    for b in bufs + [out]:
        b.destroy()
