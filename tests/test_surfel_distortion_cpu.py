"""CPU tests of the surfel frame's depth-distortion map (include/splat.h, "Depth distortion"): the binary32 operation order of
csrc/surfel.h restated in tests/surfel_distortion_ref.py holds to float64 on the GPU tests' clouds and the unshifted order does not,
the backward's formulas equal autograd on the pairwise sum, and the library and its binding declare the entry points.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from oracle import np_oracle as NO
from tests import ellipsoid_ref as ER
from tests import surfel_distortion_ref as DR
from tests import surfel_ref as SR

CLOUDS = [(3000, 160, 120, 1, 1.0, 0.03), (500, 64, 64, 3, 0.5, 0.2)]  # test_gpu_surfel.py's: n, w, h, seed, spread, scale
NEAR, FAR = 0.2, 100.0
NEW_SYMBOLS = ("splat_composite_surfel_distortion", "splat_composite_backward_distortion")


def camera_u(w, h):
    vp, eye = NO.camera(aspect=w / h)
    u = np.zeros(22, np.float32)
    u[:16], u[16:19], u[20], u[21] = vp, eye, w, h
    return u


def rel_l2(got, ref):
    return np.linalg.norm(got - ref) / np.linalg.norm(ref)


@pytest.mark.parametrize("case", CLOUDS)
def test_the_shifted_order_holds_to_float64_and_the_unshifted_does_not(case):
    """The bounds are the GPU test's: off rim / near pixels |Dist - ref64| <= 1e-3 Dist + 1e-8 and relative L2 <= 2e-5.  The plain
    m_i in the same prefix sums is at least 5e-5 off: the bound tells the two orders apart."""
    n, w, h, seed, spread, scale = case
    pos, scl, rot, col = ER.make_cloud(n, seed, spread, scale)
    u = camera_u(w, h)
    rec, cw, counts, offsets, idx = SR.lists(u, pos, scl, rot, w, h)
    ref = SR.composite(rec, col, cw, idx, counts, offsets, w, h)
    ok = ~(ref["rim"] | ref["near"])
    _, want = DR.maps(rec, col, cw, ref["steps"], w, h, NEAR, FAR)
    assert (want[ok] > 0).mean() > 0.25
    got = DR.distortion32(rec, col, cw, ref["steps"], w, h, NEAR, FAR).astype(np.float64)
    plain = DR.distortion32(rec, col, cw, ref["steps"], w, h, NEAR, FAR, shifted=False).astype(np.float64)
    e, e_plain = rel_l2(got[ok], want[ok]), rel_l2(plain[ok], want[ok])
    print(f"distortion restated {case[:3]}: relative L2 {e:.3g} shifted, {e_plain:.3g} unshifted; worst pixel "
          f"{(np.abs(got - want)[ok] / (want[ok] + 1e-30)).max():.3g}")
    assert (np.abs(got - want)[ok] <= 1e-3 * want[ok] + 1e-8).all()
    assert e <= 2e-5
    assert e_plain >= 5e-5
    assert (got[np.isinf(ref["depth"])] == 0).all()


@pytest.mark.parametrize("far", [FAR, np.inf])
def test_backward_formulas_equal_autograd_on_a_nine_entry_pixel(far):
    rng = np.random.default_rng(17)
    alpha0, t0 = rng.uniform(0.05, 0.6, 9), np.sort(rng.uniform(1.0, 6.0, 9)) + rng.normal(0, 0.2, 9)
    alpha, t = torch.tensor(alpha0, requires_grad=True), torch.tensor(t0, requires_grad=True)
    T = torch.cat([torch.ones(1, dtype=torch.float64), torch.cumprod(1 - alpha, 0)[:-1]])
    wgt = T * alpha
    m = (1 - NEAR / t) if np.isinf(far) else far * (t - NEAR) / ((far - NEAR) * t)
    dist = sum(wgt[i] * wgt[j] * (m[i] - m[j]) ** 2 for i in range(9) for j in range(i))
    dist.backward()
    got, galpha, gt = DR.pixel_grads(alpha0, t0, NEAR, far)
    assert abs(got - float(dist.detach())) <= 1e-12 * float(dist.detach())
    assert np.abs(galpha - alpha.grad.numpy()).max() <= 1e-12 and np.abs(gt - t.grad.numpy()).max() <= 1e-12
    assert np.abs(alpha.grad.numpy()).max() > 1e-4 and np.abs(t.grad.numpy()).max() > 1e-5


def test_constant():
    assert DR.constant(0.2, np.inf) == np.float32(0.2)
    assert DR.constant(0.2, 100.0) == np.float32(float(np.float32(0.2)) * 100.0 / (100.0 - float(np.float32(0.2))))


def test_library_exports_and_binding_declares_the_distortion_entry_points():
    import __graft_entry__ as g
    from splat_renderer_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    dll = C.CDLL(_lib.LIB_PATH)
    assert [s for s in NEW_SYMBOLS if not hasattr(dll, s)] == []
    assert [s for s in NEW_SYMBOLS if s not in _lib.SIGNATURES] == []
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "splat.h")).read()
    kinds = {"uint32_t": C.c_uint32, "float": C.c_float}
    for name in NEW_SYMBOLS:
        proto = re.search(r"\bint " + name + r"\(([^;]*)\);", header)
        assert proto, name
        want = []
        for arg in proto.group(1).split(","):
            arg = " ".join(arg.split())
            if "splat_composite_cfg *" in arg:
                want.append(C.POINTER(_lib.CompositeCfg))
            elif "*" in arg:
                want.append(C.c_void_p)
            else:
                want.append(kinds[arg.rsplit(" ", 1)[0]])
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int and list(args) == want, name
