"""GPU tests of AbsGS's absolute screen-space gradient through torch autograd and the fit (splat_renderer_amd.autograd:
rasterize / render_gaussians(absgrad=True); splat_renderer_amd.fit: GaussianFit(absgrad=True)).

rasterize(absgrad=True) leaves in aux.absgrad what the C entry point gives for the same frame: bit for bit with
deterministic=True, within the per-splat bound of tests/test_gpu_absgrad.py otherwise; rec.grad, col.grad and the image are the
absgrad=False run's bits under deterministic=True.  A fit's step() turns the plane into grad_accum by
splat_density_accumulate_abs, with the signed gradients still going to Adam.  And the case the statistic exists for: one splat
under a point-symmetric error, which the signed statistic cannot see and the absolute one can (tests/absgrad_ref.py says why
that perturbation touches four pixels only).
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from splat_renderer_amd import _lib
from splat_renderer_amd import autograd as AG
from splat_renderer_amd.fit import GaussianFit
from tests import absgrad_ref as AR
from tests import composite_grad_terms_ref as CT
from tests import test_gpu_grad_per_splat as TPS

pytestmark = pytest.mark.gpu

SH_C0 = 0.28209479177387814


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu().numpy()


def _leaf(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda", requires_grad=True)


def frame(s, absgrad, deterministic, depth=False):
    """One forward and backward of a tests/composite_grad_terms_ref scene through autograd with the scene's upstreams: dict(rgb,
    rec, col (the leaves, with .grad), aux, depths)."""
    g = torch.tensor(s["g"], device="cuda")
    pos, scl, rot, col = (_leaf(a) for a in (s["pos"][:, :3], s["scl"][:, :3], s["rot"], s["col"]))
    if depth:
        rec, depths, aux = AG.project_ellipsoids(s["u"], pos, scl, rot, return_depth=True)
    else:
        rec, aux = AG.project_ellipsoids(s["u"], pos, scl, rot)
        depths = None
    rec.retain_grad()
    out = AG.rasterize(rec, col, aux, s["w"], s["h"], depths=depths, deterministic=deterministic, absgrad=absgrad)
    loss = (out[0] * g[..., :3]).sum() + (out[1] * g[..., 3]).sum()
    if depth:
        gd = torch.tensor(s["gd"], device="cuda")
        loss = loss + (torch.where(torch.isfinite(out[2]), out[2], torch.zeros_like(out[2])) * gd).sum()
    assert aux.absgrad is None
    loss.backward()
    return dict(rgb=out[0].detach().clone(), alpha=out[1].detach().clone(), rec=rec, col=col, aux=aux, depths=depths, leaves=(pos, scl, rot))


def entry_point(s, fr, deterministic, depth=False):
    """(grec, gcol, gabs): the C entry point called directly on the frame's records, colours and lists."""
    aux = fr["aux"]
    cx, n, w, h = aux.ctx, aux.n, s["w"], s["h"]
    cx.bin(aux, w, h)
    idx, cnt, off = cx.lists()
    cfg = _lib.CompositeCfg(_lib.MODE_FRONT_TO_BACK, 1, 16, 0, _lib.U32_MAX, _lib.RECORDS_PROJECTED, 1, _lib.FOOTPRINT_ELLIPSOID)
    g = torch.tensor(s["g"], device="cuda")
    rec, col = fr["rec"].detach().contiguous(), fr["col"].detach().contiguous()
    grec, gcol = torch.zeros((n, 8), device="cuda"), torch.zeros((n, 4), device="cuda")
    gabs, gz = torch.zeros((n, 2), device="cuda"), torch.zeros(n, device="cuda")
    gd = torch.tensor(s["gd"], device="cuda") if depth else None
    tail = (fr["depths"].detach().contiguous().data_ptr(), 1, gd.data_ptr(), gz.data_ptr()) if depth else (None, 0, None, None)
    if deterministic:
        tiles = -(-w // 16) * -(-h // 16)
        nbytes = int(cx.lib.splat_composite_backward_det_abs_workspace_bytes(cx.total, tiles, n, int(depth)))
        ws = torch.empty(nbytes // 4 + 4, device="cuda", dtype=torch.int32)
        rc = cx.lib.splat_composite_backward_det_abs(cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), aux.projected.data_ptr(), idx, cnt, off,
                                                     cx.total, w, h, g.data_ptr(), n, grec.data_ptr(), gcol.data_ptr(), *tail, ws.data_ptr(), nbytes,
                                                     gabs.data_ptr())
    else:
        rc = cx.lib.splat_composite_backward_abs(cx.ctx, C.byref(cfg), col.data_ptr(), 1, rec.data_ptr(), idx, cnt, off, w, h, g.data_ptr(), n,
                                                 grec.data_ptr(), gcol.data_ptr(), *tail, gabs.data_ptr())
    assert rc == 0
    torch.cuda.synchronize()
    return grec, gcol, gabs


@pytest.mark.parametrize("depth", [False, True], ids=["colour", "depth"])
def test_rasterize_absgrad_is_the_entry_points(device, depth):
    s = CT.scene("hazy")
    n = s["n"]
    # deterministic: the entry point's bits, and beside them the bits of the run without the flag
    on = frame(s, True, True, depth)
    off = frame(s, False, True, depth)
    assert np.array_equal(on["rec"].detach().cpu().numpy().view(np.uint32), s["rec"].view(np.uint32)), "the scene's records are not the projector's"
    assert off["aux"].absgrad is None
    a = on["aux"].absgrad
    assert a is not None and tuple(a.shape) == (n, 2) and a.dtype == torch.float32 and not a.requires_grad
    grec, gcol, gabs = entry_point(s, on, True, depth)
    assert np.array_equal(bits(a), bits(gabs)) and (a > 0).any()
    assert np.array_equal(bits(on["rec"].grad), bits(grec)) and np.array_equal(bits(on["col"].grad), bits(gcol))
    for what in ("rgb", "alpha"):
        assert np.array_equal(bits(on[what]), bits(off[what])), what
    assert np.array_equal(bits(on["rec"].grad), bits(off["rec"].grad)) and np.array_equal(bits(on["col"].grad), bits(off["col"].grad))
    for x, y in zip(on["leaves"], off["leaves"]):
        assert np.array_equal(bits(x.grad), bits(y.grad))
    # zeros for the splats no pixel consumed, and a fresh tensor per backward
    assert (a[torch.tensor(~s["reached"], device="cuda")] == 0).all()
    again = frame(s, True, True, depth)
    assert again["aux"].absgrad.data_ptr() != a.data_ptr() and np.array_equal(bits(again["aux"].absgrad), bits(a))
    # the atomic path: within the per-splat bound of the float64 sums
    atom = frame(s, True, False, depth)
    m = AR.want_abs("hazy", depth)
    ref = AR.restated_abs("hazy", "quadrant", depth)
    q = CT.ratios(atom["aux"].absgrad.cpu().numpy(), m, m)
    print(f"hazy {'depth' if depth else 'colour'} through autograd: worst err / m = {q.max() / ref['c']:.2f} c_abs")
    assert (q <= TPS.MARGIN * ref["c"]).all()
    assert (atom["aux"].absgrad[torch.tensor(~s["reached"], device="cuda")] == 0).all()


def test_render_gaussians_hands_out_the_projection(device):
    s = CT.scene("needle")
    w, h = s["w"], s["h"]
    args = [torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda", requires_grad=True)
            for a in (s["pos"][:, :3], s["scl"][:, :3], s["rot"], s["col"][:, 3], s["col"][:, :3])]
    kw = dict(colors=args[4], width=w, height=h, deterministic=True)
    plain = AG.render_gaussians(s["u"], *args[:4], **kw)
    assert len(plain) == 2
    assert len(AG.render_gaussians(s["u"], *args[:4], absgrad=True, **kw)) == 2
    rgb, alpha, aux = AG.render_gaussians(s["u"], *args[:4], absgrad=True, return_aux=True, **kw)
    assert isinstance(aux, AG.ProjectedSplats) and aux.absgrad is None
    assert np.array_equal(bits(rgb), bits(plain[0])) and np.array_equal(bits(alpha), bits(plain[1]))
    g = torch.tensor(s["g"], device="cuda")
    ((rgb * g[..., :3]).sum() + (alpha * g[..., 3]).sum()).backward()
    a = aux.absgrad.cpu().numpy()
    m = AR.want_abs("needle", False)
    assert (CT.ratios(a, m, m) <= TPS.MARGIN * AR.restated_abs("needle", "quadrant", False)["c"]).all()
    *_, aux_off = AG.render_gaussians(s["u"], *args[:4], return_aux=True, **kw)
    assert aux_off.absgrad is None


def _fit_of(s, **kw):
    sh = ((s["col"][:, :3].astype(np.float64) - 0.5) / SH_C0).astype(np.float32)[:, None, :]
    return GaussianFit(s["pos"][:, :3].copy(), s["scl"][:, :3].copy(), s["rot"].copy(), np.clip(s["col"][:, 3], 1e-3, 1 - 1e-3), sh, **kw)


def test_fit_accumulates_the_absolute_statistic(device):
    s = CT.scene("needle")
    w, h, n = s["w"], s["h"], s["n"]
    target = torch.rand((h, w, 3), device="cuda", generator=torch.Generator(device="cuda").manual_seed(4))
    fits = {flag: _fit_of(s, absgrad=flag, deterministic=True) for flag in (True, False)}
    seen = {}
    for flag, fit in fits.items():
        rgb, _ = fit.render(s["u"], w, h)
        ((rgb - target) ** 2).sum().backward()
        rec = fit._frame[0]
        seen[flag] = dict(rec=rec.detach().clone(), grec=rec.grad.detach().clone(), gabs=fit._aux.absgrad.clone() if flag else None,
                          grads={k: getattr(fit, k).grad.detach().clone() for k in ("means", "log_scales", "rotations", "opacity_logits", "sh")})
        fit.step()
    on, off = seen[True], seen[False]
    # Adam got the signed gradients, and so the same step; the visibility mask is the same
    for k in on["grads"]:
        assert np.array_equal(bits(on["grads"][k]), bits(off["grads"][k])), k
        assert np.array_equal(bits(getattr(fits[True], k)), bits(getattr(fits[False], k))), k
    assert np.array_equal(fits[True].visible.cpu().numpy(), fits[False].visible.cpu().numpy())
    assert np.array_equal(bits(fits[True].denom), bits(fits[False].denom)) and np.array_equal(bits(fits[True].max_radius), bits(fits[False].max_radius))
    vis = fits[True].visible.cpu().numpy().astype(bool)
    assert vis.sum() > n // 2
    # grad_accum = hypot(abs.x W / 2, abs.y H / 2) on visible splats: splat_density_accumulate_abs's bits, the rule's value
    cx = AG._context(on["rec"])
    stats = [torch.zeros(n, device="cuda") for _ in range(3)]
    mask = torch.zeros(n, device="cuda", dtype=torch.uint8)
    assert cx.lib.splat_density_accumulate_abs(cx.ctx, on["rec"].data_ptr(), on["gabs"].data_ptr(), n, w, h, stats[0].data_ptr(), stats[1].data_ptr(),
                                               stats[2].data_ptr(), mask.data_ptr()) == 0
    assert np.array_equal(bits(fits[True].grad_accum), bits(stats[0]))
    ga = on["gabs"].cpu().numpy().astype(np.float64)
    want = np.where(vis, np.hypot(ga[:, 0] * w / 2, ga[:, 1] * h / 2), 0.0)
    got = fits[True].grad_accum.cpu().numpy()
    assert (np.abs(got - want) <= 1e-6 * want).all() and (got[vis] > 0).any()
    signed = fits[False].grad_accum.cpu().numpy()
    gs = on["grec"].cpu().numpy().astype(np.float64)
    assert (np.abs(signed - np.where(vis, np.hypot(gs[:, 0] * w / 2, gs[:, 1] * h / 2), 0.0)) <= 1e-6 * signed).all()
    assert (got >= signed * (1 - 1e-5)).all() and np.median(got[signed > 0] / signed[signed > 0]) > 2


def test_default_threshold_follows_the_statistic(device, monkeypatch):
    s = CT.scene("needle")
    seen = []
    real = _lib.DensifyCfg

    def spy(*a):
        seen.append(a[0])
        return real(*a)
    monkeypatch.setattr(_lib, "DensifyCfg", spy)
    for flag, explicit, want in ((False, None, 2e-4), (True, None, 8e-4), (True, 3e-4, 3e-4), (False, 5e-4, 5e-4)):
        fit = _fit_of(s, absgrad=flag)
        fit.densify_and_prune(**({} if explicit is None else dict(grad_threshold=explicit)))
        assert seen[-1] == want, (flag, explicit, seen[-1])


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomic", "fixed-order"])
def test_a_splat_pulled_both_ways_is_split_only_by_the_absolute_statistic(device, deterministic):
    w, h = AR.SYM_W, AR.SYM_H
    u = AR.symmetric_uniforms()
    colour = np.array([0.6, 0.55, 0.7])
    lr0 = dict(means=0.0, log_scales=0.0, rotations=0.0, opacity_logits=0.0, sh=0.0, sh_rest=0.0)

    def make(flag):
        sh = ((colour - 0.5) / SH_C0).astype(np.float32).reshape(1, 1, 3)
        return GaussianFit(np.array([[0.0, 0.0, 4.0]], np.float32), np.array([[1.0, 0.6, 0.8]], np.float32),
                           np.array([[0.9, 0.1, 0.2, 0.3]], np.float32), np.array([0.7], np.float32), sh, lr=lr0, absgrad=flag,
                           deterministic=deterministic)
    # the two statistics on the CPU, in float64, from the frame's own record, for the fixed perturbation
    probe = make(False)
    with torch.no_grad():
        probe.render(u, w, h)
    rec = probe._frame[0].detach().cpu().numpy()[0]
    assert rec[0] == 16.0 and rec[1] == 16.0, "the splat's record centre is not exactly (16, 16)"
    col = np.concatenate([np.float32(0.5) + np.float32(SH_C0) * ((colour - 0.5) / SH_C0).astype(np.float32), [np.float32(0.7)]])
    P = AR.symmetric_perturbation()
    g = np.zeros((h, w, 4))
    g[..., :3] = -2.0 * P.astype(np.float64)  # d/drgb of sum (rgb - (rgb0 + P))^2 at rgb = rgb0
    s64, a64 = AR.one_splat_sums(rec, col, g)
    signed, absolute = AR.density_statistic(s64), AR.density_statistic(a64)
    assert signed > 0 and absolute >= 100 * signed, "the perturbation does not separate the statistics: pick another one"
    thr = math.sqrt(signed * absolute)
    print(f"float64: signed {signed:.3g}, absolute {absolute:.3g}, threshold {thr:.3g}")
    out = {}
    for flag in (True, False):
        fit = make(flag)
        rgb, _ = fit.render(u, w, h)
        target = rgb.detach() + torch.tensor(P, device="cuda")
        ((rgb - target) ** 2).sum().backward()
        fit.step()
        stat = float(fit.grad_accum[0])
        assert float(fit.denom[0]) == 1.0
        counts = fit.densify_and_prune(grad_threshold=thr)
        out[flag] = (stat, counts)
        print(f"absgrad={flag}: grad_accum {stat:.6g} -> {counts}")
    assert out[False][0] < thr <= out[True][0]
    assert abs(out[True][0] - absolute) <= 1e-4 * absolute
    assert out[True][1]["n"] > 1 and out[True][1]["cloned"] + out[True][1]["split"] == 1
    assert out[False][1]["n"] == 1 and out[False][1]["kept"] == 1
