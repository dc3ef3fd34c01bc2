"""The pair-by-pair restatement of the composite backward (tests/composite_grad_terms_ref.py) against torch autograd, and the
conditions that keep tests/test_gpu_grad_per_splat.py honest, asserted on the references alone: no GPU.

terms64's per-splat sums are the gradients: they must equal ellipsoid_grad_ref.composite_grads (and, with the depth channel,
ellipsoid_depth_grad_ref.composite_depth_grads), which differentiate the same recorded pairs without any hand-derived formula.
terms32's distance from autograd, in units of m = sum |term|, is each scene's constant c_scene; it is printed here and is what
the GPU test scales its per-splat bound by."""
import numpy as np
import pytest

from tests import composite_grad_terms_ref as CT

NEW = ("hazy", "veil", "needle")


@pytest.mark.parametrize("name", CT.SCENES)
def test_terms64_sums_are_autograds_gradients(name):
    s = CT.scene(name)
    for label, got, want in (("colour", s["sum64"], s["want"]), ("depth", s["sum64_depth"], s["want_depth"])):
        assert got.shape == want.shape
        for k in range(want.shape[1]):
            top = np.abs(want[:, k]).max()
            e = np.abs(got[:, k] - want[:, k]).max()
            assert top > 0 and e <= 1e-12 * top, f"{name} {label} {CT.NAMES[k]}: {e:.3g} of {top:.3g}"
    # the depth channel is there: it moves the record and opacity gradients, and the nine colour-only numbers' m bounds them
    assert np.abs(s["sum64_depth"][:, :9] - s["sum64"]).max() > 0 and np.abs(s["sum64_depth"][:, 9]).max() > 0
    assert (np.abs(s["sum64"]) <= s["m"] * (1 + 1e-12)).all()
    assert (s["m"][~s["reached"]] == 0).all() and (s["m_depth"][~s["reached"]] == 0).all()


@pytest.mark.parametrize("name", CT.SCENES)
def test_scenes_are_what_the_gpu_tests_need(name):
    s = CT.scene(name)
    lay, dec = s["lay"], s["dec"]
    masked = float((dec["rim"] | dec["near"]).mean())
    needles = int((s["cond"][np.isfinite(s["cond"])] > 1e4).sum())
    deep = int(((lay["L"] > 2 * CT.GCH) & (lay["L"] % CT.GCH != 0)).sum())
    print(f"{name}: longest list {int(s['counts'].max())}, in-cut pairs per pixel max {int(lay['K'].max())} p99 "
          f"{np.percentile(lay['K'], 99):.0f}, masked {masked:.3f}, reached {s['reached'].mean():.3f}, {deep} pixels stop past entry "
          f"{2 * CT.GCH} off a chunk boundary, {needles} splats with cond > 1e4, {int((s['gd'] != 0).sum())} pixels with a depth upstream")
    assert s["reached"].mean() >= 0.85
    assert (s["gd"] != 0).mean() >= 0.5
    if name in NEW:
        assert masked <= 0.15
    if name in ("hazy", "veil"):  # every lane stays in more than four chunks of real pairs in both walks
        assert lay["K"].max() > 4 * CT.GCH
    if name == "veil":
        assert deep >= 100
    if name == "needle":
        assert needles >= 10


@pytest.mark.parametrize("order", CT.ORDERS)
@pytest.mark.parametrize("name", CT.SCENES)
def test_c_scene(name, order):
    """Prints c_scene = max over reached splats and numbers of |sum32 - autograd| / m.  Plain binary32 in the kernel's order must
    stay within a few hundred half-ulps of m on these lists (at most 480 pairs deep, sums of up to a few thousand terms): a
    restatement that was wrong, not merely rounded, would be off by orders of magnitude more."""
    s = CT.scene(name)
    for depth in (False, True):
        r = CT.restated(name, order, depth)
        print(f"{name} {order} {'depth' if depth else 'colour'}: c_scene = {r['c'] * 2 ** 24:.1f} x 2^-24 (on {CT.NAMES[r['worst']]}), "
              f"relative L2 per number at most {r['l2'].max():.3g}")
        assert np.isfinite(r["sum32"]).all()
        assert 0 < r["c"] <= 512 * 2.0 ** -24
        assert (r["sum32"][~s["reached"]] == 0).all()
