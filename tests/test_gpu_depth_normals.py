"""GPU tests of the depth-map normals and the fused normal-consistency loss (splat_depth_normals, splat_depth_normals_backward,
splat_normal_consistency, splat_normal_consistency_backward) against the float64 restatement of tests/depth_normals_ref.py,
within the per-pixel bounds its docstring derives.

K_N and K_G are twice the largest ratio |error| / (2^-24 bound) measured on one MI355X over every case below (MEASURED_N,
MEASURED_G; profiles/normal_loss_bench.txt records the measurement); each test prints its own largest ratios."""
import ctypes as C

import numpy as np
import pytest
import torch

from splat_renderer_amd import autograd as AG
from tests import depth_normals_ref as DR

pytestmark = pytest.mark.gpu

MEASURED_N, MEASURED_G = 0.78, 0.29  # largest ratios measured on the MI355X: forward map / dL/dF, and dL/ddepth
K_N, K_G = 2.0 * MEASURED_N, 2.0 * MEASURED_G

# (W, H): below 3 a side; one interior pixel; a tile edge, edge + 1, edge + 2 and two tiles + 1 under the halo-2 gather; many tiles
SHAPES = ((1, 1), (2, 7), (3, 3), (3, 4), (5, 5), (33, 17), (34, 18), (35, 19), (65, 33), (200, 120))
CAMERAS = ((60.0, False), (1200.0, False), (90.0, True))  # (focal in pixels, mirrored)
UPSTREAM = 1.7


def cuda(a):
    return torch.tensor(np.ascontiguousarray(a, np.float32), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def fptr(u):
    return u.ctypes.data_as(C.POINTER(C.c_float)) if u is not None else None


def strided(img, stride, fill):
    """(H, W, stride) device buffer, filled with `fill`, whose first three floats per pixel are img's."""
    h, w = img.shape[:2]
    buf = np.full((h, w, stride), fill, np.float32)
    buf[..., :3] = img
    return cuda(buf)


def run(u, kind, z, F, weight, gN, stride, upstream=UPSTREAM):
    """All four kernels on one input, every image with pixel stride `stride`: dict of host arrays."""
    h, w = z.shape
    zd = cuda(z)
    cx = AG._context(zd)
    lib, k = cx.lib, DR.KINDS[kind]
    sentinel = np.float32(-7.25)
    Nd, gNd, Fd = strided(np.zeros((h, w, 3)), stride, sentinel), strided(gN, stride, np.nan), strided(F, stride, np.nan)
    gFd = strided(np.zeros((h, w, 3)), stride, sentinel)
    wd = cuda(weight) if weight is not None else None
    gz_map, gz_loss = (torch.full((h, w), float("nan"), device="cuda") for _ in range(2))
    out4 = torch.full((4,), float("nan"), device="cuda")
    up = cuda([upstream])
    wp = wd.data_ptr() if wd is not None else None
    AG.check(lib.splat_depth_normals(cx.ctx, fptr(u), k, zd.data_ptr(), w, h, Nd.data_ptr(), stride), cx.ctx)
    AG.check(lib.splat_depth_normals_backward(cx.ctx, fptr(u), k, zd.data_ptr(), w, h, gNd.data_ptr(), stride, gz_map.data_ptr()), cx.ctx)
    AG.check(lib.splat_normal_consistency(cx.ctx, fptr(u), k, zd.data_ptr(), Fd.data_ptr(), stride, wp, w, h, out4.data_ptr()), cx.ctx)
    AG.check(lib.splat_normal_consistency_backward(cx.ctx, fptr(u), k, zd.data_ptr(), Fd.data_ptr(), stride, wp, w, h, up.data_ptr(),
                                                   gFd.data_ptr(), stride, gz_loss.data_ptr()), cx.ctx)
    torch.cuda.synchronize()
    return dict(N=host(Nd), gz_map=host(gz_map), out4=host(out4), gF=host(gFd), gz_loss=host(gz_loss), sentinel=sentinel)


def ratio(err, bound):
    """max of err / (2^-24 bound) where the bound is positive; the error must be exactly 0 where it is 0."""
    assert (err[bound == 0] == 0).all()
    m = bound > 0
    return float((err[m] / (DR.EPS * bound[m])).max()) if m.any() else 0.0


def check_case(u, kind, z, F, weight, gN, stride, got, worst):
    h, w = z.shape
    z64, F64, g64 = z.astype(np.float64), F.astype(np.float64), gN.astype(np.float64)
    w64 = None if weight is None else weight.astype(np.float64)
    L, frac, term_bound, r = DR.loss(F64, z64, u, w64, kind)
    finite = np.isfinite(z64)
    # validity, exact; untouched words
    N = got["N"][..., :3]
    assert ((N != 0).any(axis=2) == r.valid).all() and (N[~r.valid] == 0).all()
    for name in ("N", "gF"):
        assert (got[name][..., 3:] == got["sentinel"]).all(), f"{name}: words past the third were written"
    for name in ("N", "gz_map", "out4", "gz_loss"):
        assert np.isfinite(got[name]).all(), name
    assert np.isfinite(got["gF"][..., :3]).all()
    assert (got["gz_map"][~finite] == 0).all() and (got["gz_loss"][~finite] == 0).all()
    assert abs(float(got["out4"][1]) * w * h - r.valid.sum()) <= 1e-6 * w * h and (got["out4"][2:] == 0).all()  # the count, through one float
    # the forward map and dL/dF
    worst["N"] = max(worst["N"], ratio(np.linalg.norm(N - r.N, axis=2), r.E))
    gF, gF_bound, gz, gz_bound = DR.loss_backward(r, F64, w64, UPSTREAM)
    assert (got["gF"][..., :3][~r.valid] == 0).all()
    worst["N"] = max(worst["N"], ratio(np.linalg.norm(got["gF"][..., :3] - gF, axis=2), gF_bound))
    # dL/ddepth, of the map and of the loss
    gm, gm_bound = DR.backward(r, g64)
    worst["G"] = max(worst["G"], ratio(np.abs(got["gz_map"] - gm), gm_bound), ratio(np.abs(got["gz_loss"] - gz), gz_bound))
    # the scalar
    assert abs(got["out4"][0] - L) <= K_N * DR.EPS * term_bound.mean() + 4 * DR.EPS * abs(L), (got["out4"][0], L)


def inputs(w, h, seed):
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((h, w, 3)).astype(np.float32)
    gN = rng.standard_normal((h, w, 3)).astype(np.float32)
    weight = rng.random((h, w)).astype(np.float32)
    return F, gN, weight


def plant(a, invalid, value):
    a = a.copy()
    a[invalid] = value
    return a


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_kernels_against_float64(device, shape):
    w, h = shape
    worst = {"N": 0.0, "G": 0.0}
    case = 0
    for focal, mirrored in CAMERAS:
        u = DR.pinhole_camera(w, h, focal, mirrored)
        for kind in (DR.DISTANCE, DR.Z):
            for name, z in DR.depth_maps(u, w, h, kind, seed=case).items():
                F, gN, weight = inputs(w, h, 100 + case)
                stride = (3, 4, 8)[case % 3]
                wt = weight if case % 2 else None
                # NaN and inf planted where no result may depend on them: the upstream, F and w of invalid pixels
                invalid = ~DR.normals(z.astype(np.float64), u, kind)[1]
                bad = (np.nan, np.inf, -np.inf)[case % 3]
                got = run(u, kind, z, plant(F, invalid, bad), None if wt is None else plant(wt, invalid, bad), plant(gN, invalid, bad), stride)
                check_case(u, kind, z, F, wt, gN, stride, got, worst)
                if name == "holes" and case % 8 == 2:  # ... and they change nothing: the same bytes without them
                    clean = run(u, kind, z, F, wt, gN, stride)
                    for key in ("N", "gz_map", "out4", "gz_loss"):
                        assert np.array_equal(got[key].view(np.uint32), clean[key].view(np.uint32)), key
                    assert np.array_equal(got["gF"][..., :3].view(np.uint32), clean["gF"][..., :3].view(np.uint32))
                case += 1
    print(f"{w}x{h}: largest |error| / (2^-24 bound): forward map and dL/dF {worst['N']:.3f}, dL/ddepth {worst['G']:.3f}")
    assert worst["N"] <= K_N and worst["G"] <= K_G, worst


def test_two_runs_give_the_same_bytes(device):
    for w, h in ((65, 33), (200, 120)):
        u = DR.pinhole_camera(w, h, 1200.0)
        z = DR.depth_maps(u, w, h, DR.DISTANCE, seed=4)["holes"]
        F, gN, weight = inputs(w, h, 9)
        a, b = (run(u, DR.DISTANCE, z, F, weight, gN, 4) for _ in range(2))
        for key in ("N", "gz_map", "out4", "gF", "gz_loss"):
            assert np.array_equal(a[key].view(np.uint32), b[key].view(np.uint32)), key
        assert np.abs(a["gz_loss"]).max() > 0 and np.abs(a["gz_map"]).max() > 0


def test_invalid_arguments_are_refused(device):
    w, h = 9, 8
    u = DR.pinhole_camera(w, h, 60.0)
    z = cuda(np.ones((h, w)))
    img, gimg, gz, out4, up = cuda(np.zeros((h, w, 4))), cuda(np.zeros((h, w, 4))), cuda(np.zeros((h, w))), cuda(np.zeros(4)), cuda([1.0])
    cx = AG._context(z)
    lib = cx.lib
    ortho = u.copy()
    ortho[[3, 7, 11]] = 0.0
    ortho[15] = 1.0
    base = dict(u=u, kind=0, z=z.data_ptr(), w=w, h=h, img=img.data_ptr(), stride=4, gimg=gimg.data_ptr(), gstride=4, gz=gz.data_ptr(),
                out4=out4.data_ptr(), up=up.data_ptr(), weight=None)

    def calls(a):
        return {
            "depth_normals": lambda: lib.splat_depth_normals(cx.ctx, fptr(a["u"]), a["kind"], a["z"], a["w"], a["h"], a["gimg"], a["gstride"]),
            "depth_normals_backward": lambda: lib.splat_depth_normals_backward(cx.ctx, fptr(a["u"]), a["kind"], a["z"], a["w"], a["h"], a["img"],
                                                                               a["stride"], a["gz"]),
            "normal_consistency": lambda: lib.splat_normal_consistency(cx.ctx, fptr(a["u"]), a["kind"], a["z"], a["img"], a["stride"], a["weight"],
                                                                       a["w"], a["h"], a["out4"]),
            "normal_consistency_backward": lambda: lib.splat_normal_consistency_backward(
                cx.ctx, fptr(a["u"]), a["kind"], a["z"], a["img"], a["stride"], a["weight"], a["w"], a["h"], a["up"], a["gimg"], a["gstride"],
                a["gz"]),
        }

    for name, call in calls(base).items():
        assert call() == 0, name
    everywhere = (("u", None), ("kind", 2), ("z", None), ("w", 0), ("h", 0), ("w", 65536), ("h", 65536), ("u", ortho))
    only = {"depth_normals": (("gimg", None), ("gstride", 2)), "depth_normals_backward": (("img", None), ("stride", 2), ("gz", None)),
            "normal_consistency": (("img", None), ("stride", 2), ("out4", None)),
            "normal_consistency_backward": (("img", None), ("stride", 2), ("up", None), ("gimg", None), ("gstride", 2), ("gz", None))}
    for name in calls(base):
        for key, value in everywhere + only[name]:
            rc = calls(dict(base, **{key: value}))[name]()
            assert rc == -1, f"splat_{name}({key}={'a camera' if key == 'u' else value}): {rc}"
            assert lib.splat_last_error(cx.ctx)
    torch.cuda.synchronize()
