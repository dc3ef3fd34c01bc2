"""GPU tests of feature channels in splat_renderer_amd.autograd and GaussianFit (autograd.composite_features; rasterize,
render_gaussians and GaussianFit.render with features=): the gradients against the raw C ABI on the same frame, linearity with
the image's backward, the reuse of the context's lists, strided views, the pass-throughs, the refusal of deterministic=True, and
a tiny fit of a feature tensor.  Bounds are tests/test_gpu_features.py's: two runs of the same atomic sums lie within
2 c_scene m of each other (m and c_scene from tests/features_ref.py on the `classic` scene)."""
import ctypes as C

import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from splat_renderer_amd import autograd as AG
from tests import composite_grad_terms_ref as CT
from tests import features_ref as FR
from tests import test_gpu_ellipsoid_grad as TG
from tests import test_gpu_grad_decisions as TDEC

pytestmark = pytest.mark.gpu

NAME, K = "classic", 3
DET_MARGIN = 2.0


def cuda(a, grad=False):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda", requires_grad=grad)


def classic(grad=True):
    """The classic scene as torch leaves: dict(P, S, Q, col, f), the upstream G_F (H, W, K), and the scene."""
    s = CT.scene(NAME)
    f, gf = FR.inputs(NAME, K)
    leaves = dict(P=cuda(s["pos"][:, :3], grad), S=cuda(s["scl"][:, :3], grad), Q=cuda(s["rot"], grad), col=cuda(s["col"], grad), f=cuda(f, grad))
    return leaves, cuda(gf), s


def frame(leaves, s):
    rec, aux = AG.project_ellipsoids(s["u"], leaves["P"], leaves["S"], leaves["Q"])
    if rec.requires_grad:
        rec.retain_grad()
    return rec, aux


def bound(s):
    """(m (n, 6 + K), c_scene) of the feature backward on classic under the order the autograd context draws with."""
    order = TDEC.route_order(-1, s["w"], s["h"])
    return FR.terms64(NAME, K)["m"], FR.restated(NAME, order, K)["c_scene"], order


def numbers(grec, gcol, gfeat):
    return np.concatenate([grec[:, CT.REC_COLS], gcol[:, 3:4], gfeat], axis=1)


def host(t):
    return t.detach().cpu().numpy()


def feature_grads(leaves, gf, s, feats=None):
    """One fresh backward of L = sum G_F . composite_features: (numbers (n, 6 + K), the map, rec, aux)."""
    for t in leaves.values():
        t.grad = None
    rec, aux = frame(leaves, s)
    Fm = AG.composite_features(rec, leaves["col"], aux, leaves["f"] if feats is None else feats)
    (Fm * gf).sum().backward()
    torch.cuda.synchronize()
    return rec, aux, Fm


def test_autograd_is_the_abi(device):
    leaves, gf, s = classic()
    m, c, _ = bound(s)
    rec, aux, Fm = feature_grads(leaves, gf, s)
    n, w, h = s["n"], s["w"], s["h"]
    assert Fm.shape == (h, w, K) and Fm.dtype == torch.float32
    got = numbers(host(rec.grad), host(leaves["col"].grad), host(leaves["f"].grad))
    assert (host(leaves["col"].grad)[:, :3] == 0).all() and (host(rec.grad)[:, [4, 6, 7]] == 0).all()
    # the raw calls on the same records, colours and lists
    cx = aux.ctx
    idx, cnt, off = cx.lists_for(aux, w, h)
    cfg = AG._ellipsoid_cfg()
    recd, cold, fd = rec.detach(), leaves["col"].detach(), leaves["f"].detach()
    out = torch.empty((h, w, K), device="cuda")
    grec, gcol, gfeat = (torch.zeros((n, k), device="cuda") for k in (8, 4, K))
    head = (cx.ctx, C.byref(cfg), cold.data_ptr(), 1, recd.data_ptr(), idx, cnt, off, w, h, fd.data_ptr(), K, K)
    AG.check(cx.lib.splat_composite_features(*head, n, out.data_ptr()), cx.ctx)
    AG.check(cx.lib.splat_composite_features_backward(*head, gf.data_ptr(), n, grec.data_ptr(), gcol.data_ptr(), gfeat.data_ptr(), K), cx.ctx)
    torch.cuda.synchronize()
    assert np.array_equal(host(out).view(np.uint32), host(Fm).view(np.uint32))  # (the forward has no atomics: the same bits)
    want = numbers(host(grec), host(gcol), host(gfeat))
    q = CT.ratios(got, want.astype(np.float64), m)
    print(f"autograd vs ABI: |difference| / m at most {q.max() * 2 ** 24:.1f} x 2^-24 = {q.max() / c:.2f} c_scene")
    assert np.abs(want).max() > 0 and (q <= DET_MARGIN * c).all()
    # and the reference itself, within the ABI test's bound
    q = CT.ratios(got, FR.terms64(NAME, K)["sum"], m)[s["reached"]]
    assert (q <= 4.0 * c).all()


def test_feature_and_image_losses_add(device):
    leaves, gf, s = classic()
    m, c, order = bound(s)
    g = cuda(s["g"])

    def run(image, feature):
        for t in leaves.values():
            t.grad = None
        rec, aux = frame(leaves, s)
        loss = 0
        if image:
            rgb, alpha = AG.rasterize(rec, leaves["col"], aux)
            loss = loss + (rgb * g[..., :3]).sum() + (alpha * g[..., 3]).sum()
        if feature:
            loss = loss + (AG.composite_features(rec, leaves["col"], aux, leaves["f"]) * gf).sum()
        loss.backward()
        torch.cuda.synchronize()
        return host(rec.grad).copy(), host(leaves["col"].grad).copy()

    both, img, feat = run(True, True), run(True, False), run(False, True)
    c_img = CT.restated(NAME, order, False)["c"]
    tol_rec = DET_MARGIN * (c * m[:, :5] + c_img * s["m"][:, :5])
    tol_op = DET_MARGIN * (c * m[:, 5] + c_img * s["m"][:, 8])
    err_rec = np.abs(both[0].astype(np.float64) - (img[0].astype(np.float64) + feat[0]))[:, CT.REC_COLS]
    err_op = np.abs(both[1][:, 3].astype(np.float64) - (img[1][:, 3].astype(np.float64) + feat[1][:, 3]))
    assert (err_rec <= tol_rec).all() and (err_op <= tol_op).all()
    assert np.abs(feat[0]).max() > 0 and np.abs(img[0]).max() > 0 and (feat[1][:, :3] == 0).all()


def test_lists_are_reused(device):
    leaves, gf, s = classic()
    m, c, _ = bound(s)
    rec, aux, _ = feature_grads(leaves, gf, s)
    first = numbers(host(rec.grad), host(leaves["col"].grad), host(leaves["f"].grad))
    cx = aux.ctx
    # rasterize bins; composite_features on the same projection and screen does not bin again; nor does its backward
    rec, aux = frame(leaves, s)
    gen = cx.generation
    AG.rasterize(rec, leaves["col"], aux)
    Fm = AG.composite_features(rec, leaves["col"], aux, leaves["f"])
    assert cx.generation == gen + 1
    for t in leaves.values():
        t.grad = None
    (Fm * gf).sum().backward()
    assert cx.generation == gen + 1
    # an unrelated frame replaces the lists: the backward of a pending map bins its own again, and matches
    rec, aux = frame(leaves, s)
    Fm = AG.composite_features(rec, leaves["col"], aux, leaves["f"])
    pos, scl, rot, col, _ = TG._torch_scene(2000, 96, 64, 4)
    with torch.no_grad():
        AG.render_gaussians(TG.camera_u(96, 64), cuda(pos), cuda(scl), cuda(rot), cuda(col[:, 3]), colors=cuda(col[:, :3]), width=96, height=64)
    gen = cx.generation
    for t in leaves.values():
        t.grad = None
    (Fm * gf).sum().backward()
    torch.cuda.synchronize()
    assert cx.generation == gen + 1
    late = numbers(host(rec.grad), host(leaves["col"].grad), host(leaves["f"].grad))
    q = CT.ratios(late, first.astype(np.float64), m)
    assert (q <= DET_MARGIN * c).all() and np.abs(late).max() > 0


def test_strided_view_is_read_in_place(device):
    leaves, gf, s = classic()
    m, c, _ = bound(s)
    rec, aux, Fm0 = feature_grads(leaves, gf, s)
    packed = host(leaves["f"].grad).copy()
    wide = torch.zeros((s["n"], 5), device="cuda")
    wide[:, 1:4] = leaves["f"].detach()
    wide.requires_grad_(True)
    lib = AG._context(wide).lib
    real, strides = lib.splat_composite_features, []

    def spy(*args):
        strides.append((args[10], args[11]))
        return real(*args)
    try:
        lib.splat_composite_features = spy
        _, _, Fm1 = feature_grads(leaves, gf, s, feats=wide[:, 1:4])
    finally:
        lib.splat_composite_features = real
    assert strides == [(wide.data_ptr() + 4, 5)]  # the view itself, by stride: no copy
    assert np.array_equal(host(Fm0).view(np.uint32), host(Fm1).view(np.uint32))
    g = host(wide.grad)
    assert (g[:, [0, 4]] == 0).all()
    q = CT.ratios(g[:, 1:4], packed.astype(np.float64), m[:, FR.NREC:])
    assert (q <= DET_MARGIN * c).all() and np.abs(packed).max() > 0
    # (n,) for K = 1
    one = AG.composite_features(rec.detach(), leaves["col"].detach(), aux, leaves["f"].detach()[:, 0])
    assert one.shape == (s["h"], s["w"], 1) and np.array_equal(host(one)[..., 0].view(np.uint32), host(Fm0)[..., 0].view(np.uint32))


def test_pass_throughs(device):
    n, w, h = 3000, 160, 120
    pos, scl, rot, col, _ = TG._torch_scene(n, w, h, 1)
    leaves = dict(means=cuda(pos, True), scales=cuda(scl, True), rotations=cuda(rot, True), opacities=cuda(col[:, 3], True))
    rng = np.random.default_rng(5)
    F = cuda(rng.uniform(-2, 2, (n, 4)), True)
    gf = cuda(rng.uniform(-1, 1, (h, w, 4)))
    u = TG.camera_u(w, h)
    out = AG.render_gaussians(u, *leaves.values(), colors=cuda(col[:, :3]), width=w, height=h, features=F)
    assert len(out) == 3 and out[0].shape == (h, w, 3) and out[1].shape == (h, w) and out[2].shape == (h, w, 4)
    plain = AG.render_gaussians(u, *leaves.values(), colors=cuda(col[:, :3]), width=w, height=h)
    assert len(plain) == 2 and torch.equal(plain[0], out[0]) and torch.equal(plain[1], out[1])
    (out[2] * gf).sum().backward()
    torch.cuda.synchronize()
    reached = np.abs(host(F.grad)).max(axis=1) > 1e-6
    assert reached.sum() > n // 4
    for name, t in list(leaves.items()) + [("features", F)]:
        g = host(t.grad).reshape(n, -1)
        assert np.isfinite(g).all(), name
        assert (np.abs(g[reached]).max(axis=1) > 0).all(), f"{name}: a reached splat without a gradient"
    four = AG.render_gaussians(u, *leaves.values(), colors=cuda(col[:, :3]), width=w, height=h, return_depth=True, features=F)
    assert len(four) == 4 and four[2].shape == (h, w) and four[3].shape == (h, w, 4)
    assert torch.equal(four[3], out[2]) and torch.isinf(four[2]).any()  # (depth: +inf where nothing contributed; the map: 0)
    fit = sr.GaussianFit(pos, scl, rot, np.clip(col[:, 3], 1e-3, 1 - 1e-3), np.zeros((n, 1, 3), np.float32))
    got = fit.render(u, w, h, features=F.detach())
    assert len(got) == 3 and got[2].shape == (h, w, 4) and np.isfinite(host(got[2])).all()


def test_deterministic_with_features_is_refused(device):
    n, w, h = 300, 64, 48
    pos, scl, rot, col, sh = TG._torch_scene(n, w, h, 2)
    u = TG.camera_u(w, h)
    F = cuda(np.ones((n, 2)))
    fit = sr.GaussianFit(pos, scl, rot, np.clip(col[:, 3], 1e-3, 1 - 1e-3), sh, deterministic=True)
    with pytest.raises(sr.SplatError, match="fixed-order"):
        fit.render(u, w, h, features=F)
    assert len(fit.render(u, w, h)) == 2
    rec, aux = AG.project_ellipsoids(u, cuda(pos), cuda(scl), cuda(rot))
    with pytest.raises(sr.SplatError, match="fixed-order"):
        AG.rasterize(rec, cuda(col), aux, deterministic=True, features=F)
    with pytest.raises(sr.SplatError, match="fixed-order"):
        AG.render_gaussians(u, cuda(pos), cuda(scl), cuda(rot), cuda(col[:, 3]), colors=cuda(col[:, :3]), width=w, height=h, deterministic=True,
                            features=F)


def test_a_tiny_fit_of_features(device):
    """The map is linear in f: 30 Adam steps on a learnable (n, 3) tensor towards a map rendered from a known one lower the
    loss.  The sign and the plumbing, not a rate."""
    n, w, h = 300, 64, 48
    pos, scl, rot, col, _ = TG._torch_scene(n, w, h, 3, spread=0.5, scale=0.1)
    rec, aux = AG.project_ellipsoids(TG.camera_u(w, h), cuda(pos), cuda(scl), cuda(rot))
    colt = cuda(col)
    known = cuda(np.random.default_rng(8).uniform(-1, 1, (n, 3)))
    with torch.no_grad():
        target = AG.composite_features(rec, colt, aux, known)
    assert target.abs().max() > 0.1
    f = torch.zeros((n, 3), device="cuda", requires_grad=True)
    opt = torch.optim.Adam([f], lr=0.05)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        loss = ((AG.composite_features(rec, colt, aux, f) - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"loss {losses[0]:.4g} -> {losses[-1]:.4g}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
