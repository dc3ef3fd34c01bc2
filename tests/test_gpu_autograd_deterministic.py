"""GPU tests of deterministic=True in splat_renderer_amd.autograd and GaussianFit: the same .grad bits from two fresh graphs
(the camera's included), through the path that rebuilds a frame's lists, no workspace on the default path, and whole fits -
3DGS density control and 3DGS-MCMC - that end in the same parameters, moments and PLY bytes when run twice."""
import numpy as np
import pytest
import torch

import splat_renderer_amd as sr
from splat_renderer_amd import autograd as AG
from tests import ellipsoid_ref as ER
from tests import test_gpu_ellipsoid_grad as TG

pytestmark = pytest.mark.gpu

NAMES = ("means", "scales", "rotations", "opacities", "sh", "uniforms")


def _frame_inputs(n, w, h, seed, degree=1):
    pos, scl, rot, col, sh = TG._torch_scene(n, w, h, seed, degree=degree)
    rng = np.random.default_rng(seed + 100)
    ups = (rng.uniform(-1, 1, (h, w, 3)).astype(np.float32), rng.uniform(-1, 1, (h, w)).astype(np.float32),
           rng.uniform(-1, 1, (h, w)).astype(np.float32))
    return (pos, scl, rot, col[:, 3].copy(), sh, TG.camera_u(w, h)), tuple(torch.as_tensor(a, device="cuda") for a in ups)


def _graph(arrays, ups, w, h, deterministic=True):
    """A fresh graph of one frame with a depth map: (leaves by name, loss)."""
    leaves = {name: TG._leaf(a) for name, a in zip(NAMES[:5], arrays[:5])}
    leaves["uniforms"] = torch.tensor(np.asarray(arrays[5], np.float32), requires_grad=True)
    rgb, alpha, depth = AG.render_gaussians(leaves["uniforms"], leaves["means"], leaves["scales"], leaves["rotations"], leaves["opacities"],
                                            sh=leaves["sh"], width=w, height=h, return_depth=True, deterministic=deterministic)
    g_rgb, g_alpha, g_depth = ups
    loss = (rgb * g_rgb).sum() + (alpha * g_alpha).sum() + (torch.where(alpha > 0, depth, torch.zeros_like(depth)) * g_depth).sum()
    return leaves, loss


def _grads(leaves):
    torch.cuda.synchronize()
    return {name: t.grad.detach().cpu().numpy().copy() for name, t in leaves.items()}


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def test_render_gaussians_deterministic(device):
    n, w, h = 3000, 160, 120
    arrays, ups = _frame_inputs(n, w, h, 7)
    runs = []
    for _ in range(2):
        leaves, loss = _graph(arrays, ups, w, h)
        loss.backward()
        runs.append(_grads(leaves))
    for name in NAMES:
        assert np.isfinite(runs[0][name]).all() and np.abs(runs[0][name]).max() > 0, name
        assert _same_bits(runs[0][name], runs[1][name]), f"{name}.grad differs between two backward passes"
    # frame A, then frame B (which re-bins the shared binner), then A's backward: A's lists are rebuilt, the same bits
    arrays_b, ups_b = _frame_inputs(3500, w, h, 9)
    leaves_a, loss_a = _graph(arrays, ups, w, h)
    _graph(arrays_b, ups_b, w, h)
    loss_a.backward()
    late = _grads(leaves_a)
    for name in NAMES:
        assert _same_bits(late[name], runs[0][name]), f"{name}.grad differs after the lists were rebuilt"
    # within the atomic path's rounding of the default path's gradients
    leaves_d, loss_d = _graph(arrays, ups, w, h, deterministic=False)
    loss_d.backward()
    default = _grads(leaves_d)
    for name in NAMES[:5]:
        e = TG.rel_l2(runs[0][name].reshape(-1), default[name].reshape(-1))
        print(f"{name}: deterministic vs default relative L2 {e:.3g}")
        assert e <= 2e-4, f"{name}: relative L2 {e:.3g} to the default path"


def test_default_path_allocates_no_workspace(device):
    n, w, h = 3000, 160, 120
    arrays, ups = _frame_inputs(n, w, h, 7)
    peaks, calls = {}, []
    lib = AG._context(ups[0]).lib
    real = {name: getattr(lib, name) for name in ("splat_composite_backward", "splat_composite_backward_depth", "splat_composite_backward_det",
                                                  "splat_composite_backward_det_workspace_bytes")}

    def counted(name):
        def call(*args):
            calls.append(name)
            return real[name](*args)
        return call
    try:
        for name in real:
            setattr(lib, name, counted(name))
        for flag in (False, True, False):  # (the first pass also warms the allocator's pools; the later two are compared)
            leaves, loss = _graph(arrays, ups, w, h, deterministic=flag)
            cx = AG._context(leaves["means"])
            pairs = cx.total
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            del calls[:]
            loss.backward()
            torch.cuda.synchronize()
            peaks[flag] = torch.cuda.max_memory_allocated() - before
            want = ["splat_composite_backward_det_workspace_bytes", "splat_composite_backward_det"] if flag else ["splat_composite_backward_depth"]
            assert calls == want, f"deterministic={flag}: backward called {calls}"
            del leaves, loss
    finally:
        for name, fn in real.items():
            setattr(lib, name, fn)
    tiles = ((w + 15) // 16) * ((h + 15) // 16)
    ws = int(cx.lib.splat_composite_backward_det_workspace_bytes(pairs, tiles, n, 1))
    print(f"backward's peak above its start: default {peaks[False]} B, deterministic {peaks[True]} B; workspace {ws} B for {pairs} pairs")
    assert pairs > 5000 and ws >= 40 * pairs
    # the two backward passes allocate the same tensors but for the workspace: the default path holds none
    assert peaks[True] >= peaks[False] + ws - 4096, "the default backward's peak is not a workspace below the deterministic one's"


# ---- whole fits, twice ------------------------------------------------------------------------------------------------------
FIT_N, FIT_W, FIT_H, FIT_STEPS = 400, 64, 64, 40


def _fit_start():
    pos, scl, rot, col = ER.make_cloud(FIT_N, 41, 0.6, 0.06, degenerate=False)
    rng = np.random.default_rng(41)
    sh = rng.normal(0, 0.4, (FIT_N, 4, 3)).astype(np.float32)
    target = torch.as_tensor(rng.uniform(0, 1, (FIT_H, FIT_W, 3)).astype(np.float32), device="cuda")
    return (pos[:, :3].copy(), scl[:, :3].copy(), rot, np.clip(col[:, 3], 0.05, 0.95), sh), target, TG.camera_u(FIT_W, FIT_H)


def _run_fit(mcmc, path):
    start, target, u = _fit_start()
    fit = sr.GaussianFit(*start, sparse=not mcmc, deterministic=True)
    events = []
    for step in range(1, FIT_STEPS + 1):
        rgb, _ = fit.render(u, FIT_W, FIT_H)
        loss = AG.photometric_loss(rgb, target)
        if mcmc:
            loss = loss + fit.regularizer()
        loss.backward()
        fit.step()
        if mcmc:
            fit.inject_noise()
            if step in (20, 35):
                events.append((fit.relocate(min_opacity=0.3), fit.add_new(max_splats=FIT_N + 60)))
        else:
            if step in (20, 35):
                events.append(fit.densify_and_prune(grad_threshold=1e-6, max_splats=2 * FIT_N))
            if step == 30:
                fit.reset_opacity(0.01)
    torch.cuda.synchronize()
    fit.save_ply(path)
    return fit, events


@pytest.mark.parametrize("mcmc", [False, True], ids=["density-control", "mcmc"])
def test_a_whole_fit_twice(device, tmp_path, mcmc):
    paths = [str(tmp_path / f"run{k}.ply") for k in range(2)]
    (fit_a, events_a), (fit_b, events_b) = (_run_fit(mcmc, p) for p in paths)
    print(f"{'mcmc' if mcmc else 'density control'}: n {FIT_N} -> {fit_a.n}; events {events_a}")
    assert events_a == events_b and fit_a.n == fit_b.n
    assert fit_a.n != FIT_N, "the fit's splat count never changed: the run does not cover density control"
    for name in ("means", "log_scales", "rotations", "opacity_logits", "sh"):
        a, b = getattr(fit_a, name), getattr(fit_b, name)
        assert torch.isfinite(a).all(), name
        assert torch.equal(a, b), f"{name} differs between the two runs"
        assert torch.equal(fit_a.m[name], fit_b.m[name]) and torch.equal(fit_a.v[name], fit_b.v[name]), f"{name}: moments differ"
    with open(paths[0], "rb") as fa, open(paths[1], "rb") as fb:
        assert fa.read() == fb.read(), "the two saved PLY files differ"
