"""GPU tests of the fused image loss (splat_image_loss, splat_image_loss_backward, splat_renderer_amd.autograd.photometric_loss)
against the float64 restatement of tests/image_loss_ref.py.

Bounds (none of them taken from the code under test):
  scalars   |loss, l1, ssim - float64| <= 2e-5: three times the worst error (6.3e-6) of a float32 torch restatement on these scenes;
  gradient  relative L2 over the whole image <= 1e-4, the bound of every gradient test of this project; on the images no larger
            than the window (1 x 1, 3 x 7, 11 x 11) max |difference| <= 1e-4 max |reference| instead;
  near_equal is ill-conditioned by construction (x = y + 1e-3 noise: m is within 1e-3 of its maximum, its gradient a small
            difference of large terms): its gradient bound is max(1e-4, 2 x the error, in the same measure, of the float32
            torch restatement with the 2-D window on the same inputs), computed here.
Every test prints the figure it asserts on.
"""
import time

import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from splat_renderer_amd import autograd as AG
from tests import ellipsoid_ref as ER
from tests import image_loss_ref as LR
from tests import test_gpu_ellipsoid_grad as TG

pytestmark = pytest.mark.gpu

SCALAR_BOUND = 2e-5
GRAD_BOUND = 1e-4
SENT = np.uint32(0x7FC0BEEF)  # a quiet NaN with a payload: no kernel arithmetic produces these bits
TAIL = 8                      # floats past each image
LAMBDAS = (0.0, 0.2, 1.0)
STRIDES = [(a, b, c) for a in (3, 4) for b in (3, 4) for c in (3, 4)]  # image, target, gradient
# The fit of test_fit_with_the_fused_loss with the float32 torch conv2d loss in place of the fused one (the same loop, measured
# on an MI355X before the assertion was written): final / initial loss
R_TORCH = 0.0132  # (0.112842 -> 0.00149183)


def _pack(a, stride):
    """(H, W, 3) float32 -> a CUDA float vector of H W pixels `stride` floats apart, NaN in every other word and past the end."""
    h, w, _ = a.shape
    buf = np.full(h * w * stride + TAIL, np.nan, np.float32)
    buf[:h * w * stride].reshape(h * w, stride)[:, :3] = a.reshape(-1, 3)
    return torch.from_numpy(buf).cuda()


def abi_loss(x, y, lam, strides=(3, 3, 3), workspace=True, upstream=1.0, backward=True):
    """(rc, out4, grad (H, W, 3), raw gradient buffer as uint32) of splat_image_loss then splat_image_loss_backward on torch's
    current stream; the gradient buffer is pre-filled with SENT."""
    h, w, _ = x.shape
    xs, ys, gs = strides
    X, Y = (x, y) if isinstance(x, torch.Tensor) else (_pack(x, xs), _pack(y, ys))
    cx = AG._context(X)
    lib = cx.lib
    nbytes = int(lib.splat_image_loss_workspace_bytes(w, h))
    ws = torch.empty(nbytes // 4, device="cuda", dtype=torch.float32) if workspace else None
    out = torch.from_numpy(np.full(4 + TAIL, SENT, np.uint32).view(np.float32)).cuda()
    rc = lib.splat_image_loss(cx.ctx, X.data_ptr(), xs, Y.data_ptr(), ys, w, h, lam, ws.data_ptr() if workspace else None,
                              nbytes if workspace else 0, out.data_ptr())
    if rc != 0 or not backward:
        torch.cuda.synchronize()
        return rc, out.cpu().numpy(), None, None
    G = torch.from_numpy(np.full(h * w * gs + TAIL, SENT, np.uint32).view(np.float32)).cuda()
    up = torch.tensor([upstream], device="cuda", dtype=torch.float32)
    rc = lib.splat_image_loss_backward(cx.ctx, X.data_ptr(), xs, Y.data_ptr(), ys, w, h, lam, ws.data_ptr() if workspace else None,
                                       nbytes if workspace else 0, up.data_ptr(), G.data_ptr(), gs)
    torch.cuda.synchronize()
    raw = G.cpu().numpy().view(np.uint32)
    o = out.cpu().numpy()
    assert (o.view(np.uint32)[4:] == SENT).all(), "floats past out4 were written"
    grad = raw[:h * w * gs].reshape(h * w, gs)[:, :3].copy().view(np.float32).reshape(h, w, 3)
    return rc, o[:4], grad, raw


def _untouched(raw, h, w, gs):
    pad = raw[:h * w * gs].reshape(h * w, gs)[:, 3:]
    return (pad == SENT).all() and (raw[h * w * gs:] == SENT).all()


def _grad_error(got, ref, small):
    """The measure a gradient is held to: relative L2, or on the small images max |difference| / max |reference|."""
    if small:
        return float(np.abs(got.astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))
    return LR.rel_l2(got, ref)


def _check_case(name, hw, lambdas=LAMBDAS, strides=STRIDES):
    h, w = hw
    x, y = LR.scene(name, h, w)
    small = hw in LR.SMALL_SIZES
    worst = dict(loss=0.0, l1=0.0, ssim=0.0, grad=0.0, bound=GRAD_BOUND)
    for lam in lambdas:
        ref = LR.analytic_form(x, y, lam)
        bound = GRAD_BOUND
        if name == "near_equal" and lam > 0:
            t32 = LR.conv2d_form(x, y, lam, two_d=True, dtype=torch.float32, device="cuda")
            e32 = _grad_error(t32[3], ref[3], small)
            bound = max(GRAD_BOUND, 2.0 * e32)
            print(f"{name} {h}x{w} lambda={lam}: float32 torch restatement (2-D window) {e32:.3g} -> bound {bound:.3g}")
        for st in strides:
            rc, out, grad, raw = abi_loss(x, y, lam, st)
            assert rc == 0
            label = f"{name} {h}x{w} lambda={lam} strides={st}"
            assert np.isfinite(out).all() and np.isfinite(grad).all(), label
            assert out[3] == 0.0 and _untouched(raw, h, w, st[2]), f"{label}: padding words or the floats past the image were written"
            errs = [abs(float(out[k]) - ref[k]) for k in range(3)]
            e = _grad_error(grad, ref[3], small)
            for k, key in enumerate(("loss", "l1", "ssim")):
                worst[key] = max(worst[key], errs[k])
            if e / bound >= worst["grad"] / worst["bound"]:
                worst["grad"], worst["bound"] = e, bound
            assert max(errs) <= SCALAR_BOUND, f"{label}: |loss, l1, ssim - float64| = {errs}"
            assert e <= bound, f"{label}: gradient {'max-relative' if small else 'relative L2'} {e:.3g} > {bound:.3g}"
    print(f"{name} {h}x{w}: worst |dloss| {worst['loss']:.3g} |dl1| {worst['l1']:.3g} |dssim| {worst['ssim']:.3g}; "
          f"gradient {'max-relative' if small else 'relative L2'} {worst['grad']:.3g} (bound {worst['bound']:.3g})")


@pytest.mark.parametrize("hw", LR.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", LR.SCENES)
def test_abi_against_float64(device, name, hw):
    _check_case(name, hw)


def test_abi_against_float64_full_hd(device):
    _check_case("textured", LR.FULL_HD)


def test_padding_words_are_untouched_and_not_read(device):
    """The fourth word of a stride-4 gradient and the floats past it keep the sentinel's bits; NaN in the fourth word of the
    stride-4 inputs (and past both images) reaches no result."""
    h, w = 67, 93
    x, y = LR.scene("textured", h, w)
    rc, out, grad, raw = abi_loss(x, y, 0.2, (4, 4, 4))
    assert rc == 0 and np.isfinite(out).all() and np.isfinite(grad).all()
    pad = raw[:h * w * 4].reshape(-1, 4)[:, 3]
    print(f"sentinels found: {int((pad == SENT).sum())} of {h * w} fourth words, {int((raw[h * w * 4:] == SENT).sum())} of {TAIL} past the image")
    assert (pad == SENT).all() and (raw[h * w * 4:] == SENT).all()
    rc3, out3, grad3, _ = abi_loss(x, y, 0.2, (3, 3, 3))
    assert np.array_equal(out.view(np.uint32), out3.view(np.uint32)) and np.array_equal(grad.view(np.uint32), grad3.view(np.uint32)), \
        "the strides changed a result"


@pytest.mark.parametrize("hw", LR.SIZES + (LR.FULL_HD,), ids=lambda s: f"{s[0]}x{s[1]}")
def test_two_calls_give_the_same_bits(device, hw):
    x, y = LR.scene("textured", *hw)
    a = abi_loss(x, y, 0.2, (4, 3, 3))
    b = abi_loss(x, y, 0.2, (4, 3, 3))
    same_out = np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    differing = int((a[3] != b[3]).sum())
    print(f"{hw[0]}x{hw[1]}: out4 bit-equal {same_out}, gradient words that differ {differing}")
    assert a[0] == 0 and b[0] == 0 and same_out and differing == 0


def test_lambda_zero_without_a_workspace_is_a_plain_l1(device):
    x, y = LR.scene("noise", 67, 93)
    rc, out, grad, _ = abi_loss(x, y, 0.0, (3, 3, 3), workspace=False)
    ref = LR.analytic_form(x, y, 0.0)
    print(f"L1 alone: loss {out[0]:.8g} l1 {out[1]:.8g} (float64 {ref[1]:.8g}), ssim {out[2]}")
    assert rc == 0 and np.isnan(out[2]) and out[0] == out[1] and abs(float(out[1]) - ref[1]) <= SCALAR_BOUND
    assert LR.rel_l2(grad, ref[3]) <= GRAD_BOUND
    xt, yt = torch.from_numpy(x).cuda().requires_grad_(), torch.from_numpy(y).cuda()
    loss = AG.photometric_loss(xt, yt, 0.0)
    loss.backward()
    assert float(loss.detach()) == float(out[0]) and np.array_equal(xt.grad.cpu().numpy(), grad)
    _, l1, ssim = AG.photometric_loss(xt, yt, 0.0, return_terms=True)  # (asking for the terms computes them)
    assert abs(float(ssim) - LR.analytic_form(x, y, 0.0)[2]) <= SCALAR_BOUND and not l1.requires_grad


def _frame_scene():
    n, w, h, seed, degree = 3000, 160, 120, 7, 1  # test_render_gaussians_gradients' scene
    pos, scl, rot, col, sh = TG._torch_scene(n, w, h, seed, degree=degree)
    return TG.camera_u(w, h), pos, scl, rot, col[:, 3].copy(), sh, w, h


def test_photometric_loss_is_the_abi_bit_for_bit_on_the_view_rasterize_returns(device):
    u, pos, scl, rot, op, sh, w, h = _frame_scene()
    _, target = LR.scene("textured", h, w)
    tt = torch.from_numpy(target).cuda()
    rgb, _ = AG.render_gaussians(u, TG._leaf(pos), TG._leaf(scl), TG._leaf(rot), TG._leaf(op), sh=TG._leaf(sh), width=w, height=h)
    assert rgb.stride() == (4 * w, 4, 1) and rgb._base is not None, "rasterize no longer returns a view of its (H, W, 4) buffer"
    passed, stride = AG._image(rgb, "rgb", (3,))
    print(f"rgb strides {rgb.stride()}: passed with pixel stride {stride}, data_ptr equal {passed.data_ptr() == rgb.data_ptr()}")
    assert passed is rgb and stride == 4 and passed.data_ptr() == rgb._base.data_ptr()
    rgb.retain_grad()
    for lam in (0.2, 1.0):
        rgb.grad = None
        loss, l1, ssim = AG.photometric_loss(rgb, tt, lam, return_terms=True)
        loss.backward(retain_graph=True)
        rc, out, grad, _ = abi_loss(rgb.detach(), tt, lam, (4, 3, 3))
        got = np.array([float(loss.detach()), float(l1), float(ssim)], np.float32)
        same = np.array_equal(got.view(np.uint32), out[:3].view(np.uint32))
        differing = int((rgb.grad.cpu().numpy().view(np.uint32) != grad.view(np.uint32)).sum())
        print(f"lambda={lam}: loss {got[0]:.8g} l1 {got[1]:.8g} ssim {got[2]:.8g}; scalars bit-equal {same}, gradient words that differ {differing}")
        assert rc == 0 and same and differing == 0
        assert not l1.requires_grad and not ssim.requires_grad and loss.dim() == 0
    # other layouts: contiguous (H, W, 3) is stride 3 in place; a transposed one is copied; an (H, W, 4) target is read in place
    c3 = rgb.detach().contiguous()
    assert AG._image(c3, "rgb", (3,))[0] is c3 and AG._image(c3, "rgb", (3,))[1] == 3
    t4 = torch.cat([tt, torch.full((h, w, 1), float("nan"), device="cuda")], dim=2)
    assert AG._image(t4, "target", (3, 4))[0] is t4 and AG._image(t4, "target", (3, 4))[1] == 4
    a = float(AG.photometric_loss(c3, t4))
    b = float(AG.photometric_loss(c3.permute(1, 0, 2).contiguous().permute(1, 0, 2), tt))
    assert a == b == float(AG.photometric_loss(rgb.detach(), tt))


def test_gradients_through_the_frame(device):
    """render_gaussians -> photometric_loss -> backward against the same frame followed by the float64 restatement's loss:
    per-parameter relative L2 <= 1e-4 (torch.autograd.gradcheck is of no use in float32)."""
    u, pos, scl, rot, op, sh, w, h = _frame_scene()
    _, target = LR.scene("textured", h, w)
    tt = torch.from_numpy(target).cuda()
    grads = []
    for fused in (True, False):
        leaves = dict(means=TG._leaf(pos), scales=TG._leaf(scl), rotations=TG._leaf(rot), opacities=TG._leaf(op), sh=TG._leaf(sh))
        rgb, _ = AG.render_gaussians(u, leaves["means"], leaves["scales"], leaves["rotations"], leaves["opacities"], sh=leaves["sh"],
                                     width=w, height=h)
        loss = AG.photometric_loss(rgb, tt) if fused else LR.conv2d_loss(rgb.double(), tt.double(), shifts=True)[0]
        loss.backward()
        grads.append({k: v.grad.detach().cpu().numpy().astype(np.float64) for k, v in leaves.items()})
    for name in ("means", "scales", "rotations", "opacities", "sh"):
        e = LR.rel_l2(grads[0][name], grads[1][name])
        print(f"{name}: relative L2 {e:.3g}")
        assert np.isfinite(grads[0][name]).all() and np.abs(grads[0][name]).max() > 0
        assert e <= 1e-4, f"{name}: relative L2 {e:.3g}"


def test_refusals(device):
    x, y = LR.scene("noise", 8, 9)
    X, Y = _pack(x, 3), _pack(y, 3)
    cx = AG._context(X)
    lib = cx.lib
    nbytes = int(lib.splat_image_loss_workspace_bytes(9, 8))
    assert nbytes == 8 * 9 * 36
    ws = torch.empty(nbytes // 4, device="cuda")
    out = torch.zeros(4, device="cuda")
    up = torch.ones(1, device="cuda")
    G = torch.zeros(8 * 9 * 3, device="cuda")

    def fwd(image=X.data_ptr(), istride=3, target=Y.data_ptr(), tstride=3, w=9, h=8, lam=0.2, wsp=ws.data_ptr(), wsb=nbytes, o=out.data_ptr()):
        return lib.splat_image_loss(cx.ctx, image, istride, target, tstride, w, h, lam, wsp, wsb, o)

    def bwd(image=X.data_ptr(), istride=3, target=Y.data_ptr(), tstride=3, w=9, h=8, lam=0.2, wsp=ws.data_ptr(), wsb=nbytes, upp=up.data_ptr(),
            g=G.data_ptr(), gstride=3):
        return lib.splat_image_loss_backward(cx.ctx, image, istride, target, tstride, w, h, lam, wsp, wsb, upp, g, gstride)
    assert fwd() == 0 and bwd() == 0
    bad = dict(image=None, target=None, w=0, h=0, istride=2, tstride=0, lam=-0.1, wsb=nbytes - 16, wsp=None, o=None)
    for key, value in bad.items():
        rc = fwd(**{key: value})
        print(f"splat_image_loss({key}={value}): {rc}")
        assert rc == -1, key
    for key, value in dict(bad, lam=1.5, upp=None, g=None, gstride=2).items():
        if key == "o":
            continue
        rc = bwd(**{key: value})
        print(f"splat_image_loss_backward({key}={value}): {rc}")
        assert rc == -1, key
    assert fwd(lam=float("nan")) == -1 and fwd(lam=1.0) == 0 and fwd(lam=0.0, wsp=None, wsb=0) == 0
    torch.cuda.synchronize()
    xt, yt = torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda()
    for args in ((xt.cpu(), yt), (xt, yt.cpu()), (xt.double(), yt), (xt, yt.half()), (xt, yt[:7]), (xt[..., :2], yt), (xt.reshape(-1, 3), yt),
                 (x, yt), (xt, yt, 1.5), (xt, yt, -1.0)):
        with pytest.raises(sr.SplatError):
            AG.photometric_loss(*args)


def fit(loss_fn, steps=300):
    """test_fitting_converges' loop (tests/test_gpu_ellipsoid_grad.py: the cloud, the perturbations, the learning rates, 300 Adam
    steps) with loss_fn(rgb, target) in place of its mean squared error: (losses, params, target, frame, seconds)."""
    n, w, h = 2000, 256, 256
    u = TG.camera_u(w, h)
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
    for _ in range(steps):
        opt.zero_grad()
        loss = loss_fn(frame(*params), target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses, params, target, frame, time.time() - t0


def torch_loss(rgb, target):
    """The float32 torch conv2d route (the 2-D window), with the copy conv2d needs of rasterize's stride-4 view."""
    return LR.conv2d_loss(rgb.contiguous(), target)[0]


def test_fit_with_the_fused_loss(device):
    """test_fitting_converges with photometric_loss in place of its L2 loss.  The same loop with the float32 torch conv2d loss
    (torch_loss above) was run first on an MI355X: loss 0.112842 -> 0.00149183, final / initial r_torch = 0.0132 (R_TORCH; the fused
    loop in the same run: 0.112842 -> 0.00150249, 0.0133).  The fused loop's
    ratio must be <= 10 r_torch: the two trajectories differ by rounding only, and the factor covers Adam's sensitivity to it,
    not a weaker optimum."""
    losses, params, target, frame, elapsed = fit(AG.photometric_loss)
    ratio = losses[-1] / losses[0]
    print(f"fit: loss {losses[0]:.4g} -> {losses[-1]:.4g} (ratio {ratio:.4g}; torch conv2d loop {R_TORCH}) in {elapsed:.1f} s")
    assert all(np.isfinite(losses)) and all(torch.isfinite(p).all() for p in params)
    with torch.no_grad():
        rgb = frame(*params)
        fused = float(AG.photometric_loss(rgb, target))
        ref = float(LR.conv2d_loss(rgb.double(), target.double(), shifts=True)[0])
    print(f"final frame: fused loss {fused:.8g}, float64 {ref:.8g}, |difference| {abs(fused - ref):.3g}")
    assert abs(fused - ref) <= SCALAR_BOUND
    assert ratio <= 10 * R_TORCH
    assert elapsed < 30
