"""CPU tests of AbsGS's absolute screen-space gradient (include/splat.h, splat_composite_backward_abs): the new entry points are
declared everywhere the ABI is, the ABI version did not move, and the NumPy reference (tests/absgrad_ref.py) is what it says:
its binary32 restatement is terms32's arithmetic, its constant is finite, and the absolute sums dominate the signed ones by the
margins that make the statistic worth having."""
import os
import re

import numpy as np
import pytest

from oracle import np_oracle as NO
from tests import absgrad_ref as AR
from tests import composite_grad_terms_ref as CT
from tests import ellipsoid_grad_ref as GR
from tests import ellipsoid_ref as ER
from tests.test_abi_cpu import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ("splat_composite_backward_abs", "splat_composite_backward_det_abs", "splat_composite_backward_det_abs_workspace_bytes",
                    "splat_density_accumulate_abs")


def test_entry_points_are_declared_everywhere():
    from splat_renderer_amd import _lib
    declared = declared_functions()
    napi = open(os.path.join(ROOT, "splat_renderer_amd", "napi", "splat_napi.c")).read()
    exported = set(re.findall(r"EXPORT\(([a-z0-9_]+)\)", napi.split("napi_property_descriptor d[]")[1]))
    for name in NEW_ENTRY_POINTS:
        assert name in declared, f"{name} is not declared in include/splat.h"
        assert name in _lib.SIGNATURES, f"{name} is not in _lib.SIGNATURES"
        assert name[len("splat_"):] in exported, f"{name} has no method in the N-API addon"
    sig, det = _lib.SIGNATURES["splat_composite_backward_abs"], _lib.SIGNATURES["splat_composite_backward_det_abs"]
    assert len(sig[1]) == len(_lib.SIGNATURES["splat_composite_backward_depth"][1]) + 1
    assert len(det[1]) == len(_lib.SIGNATURES["splat_composite_backward_det"][1]) + 1
    assert _lib.SIGNATURES["splat_density_accumulate_abs"] == _lib.SIGNATURES["splat_density_accumulate"]
    lib = _lib.load()
    assert lib.splat_abi_version() == 3
    # the det workspace: 16 per tile, 4 per splat rounded up to 16, 4 NV per pair with NV = 11 / 12; 0 where it cannot fit
    for pairs, tiles, n in ((0, 1, 0), (1000, 12, 77), (12_500_000, 8160, 5_000_000)):
        for dep, nv in ((0, 11), (1, 12)):
            assert lib.splat_composite_backward_det_abs_workspace_bytes(pairs, tiles, n, dep) == 16 * tiles + 16 * ((n + 3) // 4) + 4 * nv * pairs
    assert lib.splat_composite_backward_det_abs_workspace_bytes(1 << 62, 1, 1, 0) == 0
    assert lib.splat_composite_backward_det_abs_workspace_bytes((1 << 64) // 48, 1, 1, 1) == 0
    # the existing one did not move
    assert lib.splat_composite_backward_det_workspace_bytes(1000, 12, 77, 1) == 16 * 12 + 16 * 20 + 40 * 1000


def test_python_surface():
    import inspect
    from splat_renderer_amd import autograd as AG
    from splat_renderer_amd.fit import GaussianFit
    assert inspect.signature(AG.rasterize).parameters["absgrad"].default is False
    rg = inspect.signature(AG.render_gaussians).parameters
    assert rg["absgrad"].default is False and rg["return_aux"].default is False
    assert inspect.signature(GaussianFit.__init__).parameters["absgrad"].default is False
    assert inspect.signature(GaussianFit.densify_and_prune).parameters["grad_threshold"].default is None
    assert AG.ProjectedSplats(None, np.zeros(22, np.float32), 0, None, None, None).absgrad is None


@pytest.mark.parametrize("name", CT.SCENES)
def test_restatement_and_dominance(name):
    s = CT.scene(name)
    reached = s["reached"]
    for depth in (False, True):
        m, total = (s["m_depth"], s["sum64_depth"]) if depth else (s["m"], s["sum64"])
        # an absolute sum is at least the absolute value of the signed one (both float64 sums of the same terms)
        assert (m[:, :2] >= np.abs(total[:, :2])).all()
        assert (m[~reached] == 0).all()
        for order in CT.ORDERS:
            gd = s["gd"] if depth else None
            t = AR.pair_terms32(s["rec"], s["col"], s["z"], s["lay"], s["w"], s["g"], gd, order)
            signed = np.zeros((s["n"], t.shape[1]), np.float32)
            np.add.at(signed, s["lay"]["spl"], t)
            want = CT.terms32(s["rec"], s["col"], s["z"], s["lay"], s["w"], s["g"], gd, order)
            assert np.array_equal(signed.view(np.uint32), want.view(np.uint32)), "pair_terms32 is no longer terms32's arithmetic"
            ref = AR.restated_abs(name, order, depth)
            assert np.isfinite(ref["c"]) and 0 < ref["c"] < 2.0 ** -14, ref["c"]
            assert (ref["abs32"][~reached] == 0).all() and (ref["abs32"] >= 0).all()
            print(f"{name} {order} {'depth' if depth else 'colour'}: c_abs = {ref['c'] * 2 ** 24:.1f} x 2^-24")
    # what the statistic is for: the absolute sum of c.x is at least twice the signed one for most reached splats
    share = float((s["m"][reached, 0] >= 2 * np.abs(s["sum64"][reached, 0])).mean())
    with np.errstate(all="ignore"):
        ratio = float(np.nanmedian(s["m"][reached, 0] / np.abs(s["sum64"][reached, 0])))
    print(f"{name}: median absolute / signed (c.x) {ratio:.1f}; {100 * share:.1f} % of reached splats with ratio >= 2")
    assert share > 0.5


def _symmetric_splat():
    u = AR.symmetric_uniforms()
    pos = np.array([[0, 0, 4, 1]], np.float32)
    scl = np.array([[1.0, 0.6, 0.8, 0]], np.float32)
    rot = np.array([[0.9, 0.1, 0.2, 0.3]], np.float32)
    rec, proj, keys = ER.project(u, pos, scl, rot)
    return u, pos, scl, rot, rec, proj, keys


def test_symmetric_case_cancels_in_float64():
    """The one-splat frame of the fit's GPU test: the closed form of absgrad_ref.one_splat_sums is terms64 on the same frame, the
    centre is exactly (16, 16), and for the fixed perturbation the absolute statistic is >= 100 x the signed one, which is
    not zero (the threshold between them is their geometric mean)."""
    w, h = AR.SYM_W, AR.SYM_H
    u, pos, scl, rot, rec, proj, keys = _symmetric_splat()
    assert rec[0, 0] == 16.0 and rec[0, 1] == 16.0
    col = np.array([[0.6, 0.55, 0.7, 0.7]], np.float32)
    _, order = NO.sort_pairs(keys, np.arange(keys.shape[0], dtype=np.uint32))
    counts, offsets, idx = NO.bin_sorted(proj, order, w, h, 16)
    assert (counts == 1).all() and counts.shape[0] == 4
    dec = GR.decisions(rec, col, idx, counts, offsets, w, h)
    lay = CT.pair_layout(dec["steps"], counts, w)
    g = np.zeros((h, w, 4), np.float32)
    g[..., :3] = -2 * AR.symmetric_perturbation()
    t64 = CT.terms64(rec, col, proj[:, 4], lay, w, g)
    signed, absolute = AR.one_splat_sums(rec[0], col[0], g)
    assert np.allclose(absolute, t64["m"][0, :2], rtol=1e-12, atol=0) and (absolute > 0).all()
    assert np.abs(signed).max() <= 1e-14 * absolute.min() and np.abs(t64["sum"][0, :2]).max() <= 1e-14 * absolute.min()
    s, b = AR.density_statistic(signed), AR.density_statistic(absolute)
    assert s > 0 and b >= 100 * s, "the perturbation leaves no usable float64 residue: pick another one"
