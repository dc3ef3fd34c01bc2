"""The float64 restatements of the image loss (tests/image_loss_ref.py) against each other and against hand-worked values, and
the new entry points' declarations.  No GPU."""
import os
import re

import numpy as np
import pytest

from tests import image_loss_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("splat_image_loss", "splat_image_loss_backward", "splat_image_loss_workspace_bytes")


def test_window_sums_to_one():
    g = LR.window()
    assert g.shape == (11,) and abs(g.sum() - 1.0) <= 1e-15
    assert np.array_equal(g, g[::-1]) and g.argmax() == 5
    assert abs(g[4] / g[5] - np.exp(-1.0 / 4.5)) <= 1e-15


@pytest.mark.parametrize("name", LR.SCENES)
@pytest.mark.parametrize("hw", LR.SMALL_SIZES + ((67, 93),))
def test_the_two_float64_forms_agree(name, hw):
    x, y = LR.scene(name, *hw)
    for lam in (0.0, 0.2, 1.0):
        a = LR.conv2d_form(x, y, lam)
        b = LR.analytic_form(x, y, lam)
        for c in (LR.conv2d_form(x, y, lam, two_d=False), LR.conv2d_form(x, y, lam, shifts=True)):
            for u, v, w in zip(a[:3], b[:3], c[:3]):
                assert abs(u - v) <= 1e-12 and abs(u - w) <= 1e-12
            e, e2 = LR.rel_l2(b[3], a[3]), LR.rel_l2(c[3], a[3])
            assert e <= 1e-12 and e2 <= 1e-12, f"{name} {hw} lambda={lam}: relative L2 {e:.3g} (closed form), {e2:.3g} (separable)"


@pytest.mark.parametrize("form", ["conv2d", "analytic"])
def test_identical_images(form):
    x, _ = LR.scene("noise", 40, 50)
    fn = LR.conv2d_form if form == "conv2d" else LR.analytic_form
    loss, l1, ssim, grad = fn(x, x.copy())
    assert l1 == 0.0 and ssim == 1.0 and loss == 0.0
    assert np.abs(grad).max() <= 1e-12


def test_hand_worked_one_pixel_image():
    """1 x 1: the only tap inside the image is the centre one, weight w0 = g[5]^2."""
    w0 = float(LR.window()[5]) ** 2
    for lam in (0.0, 0.2, 1.0):
        m_sum, l_sum = 0.0, 0.0
        x, y = (0.3, 0.9, 1.7), (0.6, 0.2, 0.5)
        for a, b in zip(x, y):
            a, b = float(np.float32(a)), float(np.float32(b))
            mx, my = w0 * a, w0 * b
            sx, sy, sxy = w0 * a * a - mx * mx, w0 * b * b - my * my, w0 * a * b - mx * my
            m_sum += (2 * mx * my + LR.C1) * (2 * sxy + LR.C2) / ((mx * mx + my * my + LR.C1) * (sx + sy + LR.C2))
            l_sum += abs(a - b)
        want = (1 - lam) * l_sum / 3 + lam * (1 - m_sum / 3)
        xa, ya = np.asarray(x, np.float32).reshape(1, 1, 3), np.asarray(y, np.float32).reshape(1, 1, 3)
        for fn in (LR.conv2d_form, LR.analytic_form):
            loss, l1, ssim, _ = fn(xa, ya, lam)
            assert abs(loss - want) <= 1e-14 and abs(l1 - l_sum / 3) <= 1e-15 and abs(ssim - m_sum / 3) <= 1e-14


def test_gradient_is_the_derivative():
    """The closed form against central differences of the loss, at a few pixels of a small image."""
    x, y = LR.scene("textured", 13, 17)
    _, _, _, grad = LR.analytic_form(x, y)
    x64 = x.astype(np.float64)
    for (r, c, ch) in ((0, 0, 0), (6, 8, 1), (12, 16, 2), (3, 11, 0)):
        d = np.zeros_like(x64)
        d[r, c, ch] = 1e-6
        num = (LR.analytic_form(x64 + d, y)[0] - LR.analytic_form(x64 - d, y)[0]) / 2e-6
        assert abs(num - grad[r, c, ch]) <= 1e-8 and abs(grad[r, c, ch]) > 1e-5, (r, c, ch, num, grad[r, c, ch])


def test_entry_points_are_declared_everywhere():
    from splat_renderer_amd import _lib
    header = open(os.path.join(ROOT, "include", "splat.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    addon = open(os.path.join(ROOT, "splat_renderer_amd", "napi", "splat_napi.c")).read()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), f"{name} is not declared in include/splat.h"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.SIGNATURES"
        assert "EXPORT(%s)" % name[len("splat_"):] in addon, f"{name} has no method in the N-API addon"
    assert _lib.load().splat_abi_version() == 3
    assert _lib.load().splat_image_loss_workspace_bytes(1920, 1080) == 1920 * 1080 * 36
    from splat_renderer_amd import autograd
    assert callable(autograd.photometric_loss)
