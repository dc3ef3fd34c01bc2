"""The photometric loss of include/splat.h ("Image loss") restated in float64, twice, and the scenes its tests use.

    loss = (1 - lambda) mean|x - y| + lambda (1 - mean m),  m the SSIM map over an 11 x 11 Gaussian window of sigma 1.5, zero padding

conv2d_form: torch.nn.functional.conv2d (the 2-D window g (x) g, or the two 1-D passes) with the gradient from torch.autograd: what
a user of the project wrote before the fused kernel, in any dtype and on any device.
analytic_form: NumPy, the separable window as eleven shifted adds per pass, and the gradient from the closed form of the header:
no line shared with the first.
"""
import numpy as np

LAMBDA = 0.2
C1, C2 = 0.01 ** 2, 0.03 ** 2
RADIUS = 5
BG = (0.05, 0.05, 0.1)  # the composite's background

SCENES = ("noise", "textured", "near_equal", "background", "bright")
SMALL_SIZES = ((1, 1), (3, 7), (11, 11))  # (H, W): smaller than, and equal to, the window
SIZES = SMALL_SIZES + ((67, 93), (270, 480))
FULL_HD = (1080, 1920)  # once, on `textured`


def window():
    k = np.arange(2 * RADIUS + 1, dtype=np.float64)
    g = np.exp(-((k - RADIUS) ** 2) / (2.0 * 1.5 ** 2))
    return g / g.sum()


def _textured(h, w, rng):
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    out = np.empty((h, w, 3))
    for c in range(3):
        fx, fy = rng.uniform(0.02, 0.3, 2)
        ph = rng.uniform(0, 2 * np.pi, 2)
        out[..., c] = 0.5 + 0.4 * np.sin(fx * xx + ph[0]) * np.cos(fy * yy + ph[1])
    return out


def scene(name, h, w, seed=0):
    """(x, y): float32 (h, w, 3) arrays, already rounded, so that a float64 reference sees what the kernel sees."""
    rng = np.random.default_rng(1000 * SCENES.index(name) + seed)
    if name == "noise":
        x, y = rng.random((h, w, 3)), rng.random((h, w, 3))
    elif name == "textured":
        y = _textured(h, w, rng)
        x = np.clip(y + 0.05 * rng.standard_normal((h, w, 3)), 0.0, 1.0)
    elif name == "near_equal":
        y = _textured(h, w, rng)
        x = y + 1e-3 * rng.standard_normal((h, w, 3))
    elif name == "background":
        y = _textured(h, w, rng)
        x = np.broadcast_to(np.asarray(BG), (h, w, 3))
    elif name == "bright":
        x, y = 3.0 * rng.random((h, w, 3)), rng.random((h, w, 3))
    else:
        raise ValueError(name)
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(y, np.float32)


def rel_l2(got, ref):
    got, ref = np.asarray(got, np.float64).reshape(-1), np.asarray(ref, np.float64).reshape(-1)
    return float(np.linalg.norm(got - ref) / max(np.linalg.norm(ref), 1e-300))


# ---- form 1: conv2d and autograd ---------------------------------------------------------------------------------------------
def conv2d_loss(x, y, lam=LAMBDA, two_d=True, shifts=False):
    """(loss, l1, ssim) as 0-d tensors of x's dtype and device; x, y (H, W, 3) torch tensors; differentiable in x.
    shifts=True: the same separable window as eleven shifted slices of a padded tensor per pass instead of conv2d (plain
    elementwise kernels: float64 on any device, where a convolution library may not offer it)."""
    import torch
    import torch.nn.functional as F
    g = torch.as_tensor(window(), dtype=x.dtype, device=x.device)
    a, b = x.permute(2, 0, 1)[None], y.permute(2, 0, 1)[None]

    if shifts:
        def conv(t):
            h, w = t.shape[2:]
            p = F.pad(t, (RADIUS, RADIUS, 0, 0))
            rows = sum(g[k] * p[..., k:k + w] for k in range(2 * RADIUS + 1))
            p = F.pad(rows, (0, 0, RADIUS, RADIUS))
            return sum(g[k] * p[:, :, k:k + h] for k in range(2 * RADIUS + 1))
    elif two_d:
        k2 = torch.outer(g, g)[None, None].expand(3, 1, -1, -1).contiguous()

        def conv(t):
            return F.conv2d(t, k2, padding=RADIUS, groups=3)
    else:
        kh = g[None, None, None, :].expand(3, 1, 1, -1).contiguous()
        kv = g[None, None, :, None].expand(3, 1, -1, 1).contiguous()

        def conv(t):
            return F.conv2d(F.conv2d(t, kh, padding=(0, RADIUS), groups=3), kv, padding=(RADIUS, 0), groups=3)
    mx, my = conv(a), conv(b)
    sx, sy, sxy = conv(a * a) - mx * mx, conv(b * b) - my * my, conv(a * b) - mx * my
    m = ((2 * mx * my + C1) * (2 * sxy + C2)) / ((mx * mx + my * my + C1) * (sx + sy + C2))
    ssim = m.mean()
    l1 = (a - b).abs().mean()
    return (1 - lam) * l1 + lam * (1 - ssim), l1, ssim


def conv2d_form(x, y, lam=LAMBDA, two_d=True, dtype=None, device="cpu", shifts=False):
    """(loss, l1, ssim, grad (H, W, 3)) as Python floats and a float64 NumPy array; dtype: torch.float64 by default."""
    import torch
    dtype = torch.float64 if dtype is None else dtype
    xt = torch.tensor(np.asarray(x), dtype=dtype, device=device, requires_grad=True)
    yt = torch.tensor(np.asarray(y), dtype=dtype, device=device)
    loss, l1, ssim = conv2d_loss(xt, yt, lam, two_d, shifts)
    loss.backward()
    return float(loss.detach()), float(l1.detach()), float(ssim.detach()), xt.grad.detach().cpu().numpy().astype(np.float64)


# ---- form 2: NumPy and the closed form ---------------------------------------------------------------------------------------
def _conv(img):
    """The separable window over an (H, W, 3) float64 array, zero padding."""
    g = window()
    h, w = img.shape[:2]
    pad = np.zeros((h, w + 2 * RADIUS, 3))
    pad[:, RADIUS:RADIUS + w] = img
    rows = sum(g[k] * pad[:, k:k + w] for k in range(2 * RADIUS + 1))
    pad = np.zeros((h + 2 * RADIUS, w, 3))
    pad[RADIUS:RADIUS + h] = rows
    return sum(g[k] * pad[k:k + h] for k in range(2 * RADIUS + 1))


def analytic_form(x, y, lam=LAMBDA):
    """(loss, l1, ssim, grad (H, W, 3)) in float64."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    n = x.size
    mx, my = _conv(x), _conv(y)
    sx, sy, sxy = _conv(x * x) - mx * mx, _conv(y * y) - my * my, _conv(x * y) - mx * my
    A, B = 2 * mx * my + C1, 2 * sxy + C2
    Cc, D = mx * mx + my * my + C1, sx + sy + C2
    m = A * B / (Cc * D)
    ssim = m.mean()
    l1 = np.abs(x - y).mean()
    dmu = 2 * my * B / (Cc * D) - 2 * mx * m / Cc - 2 * my * A / (Cc * D) + 2 * mx * m / D
    dsx = -m / D
    dsxy = 2 * A / (Cc * D)
    grad = (1 - lam) * np.sign(x - y) / n - (lam / n) * (_conv(dmu) + 2 * x * _conv(dsx) + y * _conv(dsxy))
    return float((1 - lam) * l1 + lam * (1 - ssim)), float(l1), float(ssim), grad
