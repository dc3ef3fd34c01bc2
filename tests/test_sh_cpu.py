"""CPU tests of what the SH colour kernels' GPU tests stand on (tests/sh_ref.py): the float64 basis against an independent
library, and the scene and the error measures against a float32 restatement of the kernels."""
import numpy as np
import pytest

from tests import ellipsoid_ref as ER
from tests import sh_ref as SR

RESTATEMENT_UNITS = 8.0  # about 1.6 times the worst the float32 restatement reaches on scene() at n = 20 000 (4.5, 5.1, 2.1)


def test_sh_basis_is_scipys_real_harmonics():
    """Band l of ER.sh_basis, columns m = -l .. l, is sqrt(2) Im Y_l^|m| (m < 0), Re Y_l^0, sqrt(2) Re Y_l^m (m > 0) of scipy's
    complex harmonics: the order and the signs inside each band, which orthonormality cannot see.  Bound 1e-12 (float64 on
    both sides; 4.2e-15 measured)."""
    sp = pytest.importorskip("scipy.special")
    rng = np.random.default_rng(5)
    d = rng.standard_normal((2000, 3))
    d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
    theta, phi = np.arccos(np.clip(d[:, 2], -1, 1)), np.arctan2(d[:, 1], d[:, 0])  # polar, azimuth
    if hasattr(sp, "sph_harm_y"):
        harm = lambda l, m: sp.sph_harm_y(l, m, theta, phi)  # noqa: E731
    else:
        harm = lambda l, m: sp.sph_harm(m, l, phi, theta)  # noqa: E731
    Y = ER.sh_basis(d, 3)
    worst = 0.0
    for l in range(4):
        for m in range(-l, l + 1):
            c = harm(l, abs(m))
            want = np.sqrt(2) * c.imag if m < 0 else c.real if m == 0 else np.sqrt(2) * c.real
            e = float(np.abs(Y[:, l * l + l + m] - want).max())
            worst = max(worst, e)
            assert e <= 1e-12, f"l={l} m={m}: {e:.3g}"
    print(f"ER.sh_basis against scipy: {worst:.3g}")


def test_basis_gradient_is_the_polynomials():
    """basis64's |grad Y| (complex step) against central differences of ER.sh_basis in R^3."""
    rng = np.random.default_rng(6)
    d = rng.standard_normal((500, 3))
    d /= np.sqrt((d * d).sum(axis=1, keepdims=True))
    _, Gn = SR.basis64(d, 3)
    h = 1e-6
    G = np.stack([(ER.sh_basis(d + h * e, 3) - ER.sh_basis(d - h * e, 3)) / (2 * h) for e in np.eye(3)], axis=2)
    assert np.abs(Gn - np.sqrt((G * G).sum(axis=2))).max() <= 1e-8
    assert (Gn[:, 0] == 0).all() and np.allclose(Gn[:, 1:4], ER.SH_C1)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_scene_is_what_it_says(degree):
    sc = SR.scene(degree, 20000, 7)
    d, ln = SR.direction64(sc.eye, sc.pos)
    assert np.abs(sc.eye).min() > 0
    assert np.array_equal(d[:SR.N_AXIS_ROWS], SR.AXES[np.arange(SR.N_AXIS_ROWS) % 6]), "the axis rows are not exactly on the axes"
    assert ln.min() < 2e-3 and ln.max() > 500 and ln.min() >= 0.99e-3 and ln.max() <= 1.01e3
    assert np.abs(sc.sh).max() > 5 and np.median(np.abs(sc.sh)) < 0.5
    clamped = float((SR.forward32(sc)[:, :3] == 0).mean())
    print(f"degree {degree}: {100 * clamped:.1f} % of the channels clamped")
    assert 0.03 <= clamped <= 0.25
    # every forward agrees on the clamp: the float32 restatement's decisions are float64's
    assert np.array_equal(SR.forward32(sc)[:, :3] > 0, SR.colors64(sc)[:, :3] > 0)
    again = SR.scene(degree, 20000, 7)
    assert all(np.array_equal(getattr(sc, k), getattr(again, k)) for k in ("pos", "sh", "op", "g"))
    small = SR.scene(degree, 5, 7)
    assert small.n == 5 and small.sh.shape == (5, (degree + 1) ** 2, 3)


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_restatement_is_within_8_units(degree):
    """A condition on the scene and the measures, not on a kernel: NumPy float32 in the kernels' operation order stays within 8
    units of 2^-24 of float64 in all three measures.  The GPU bounds are 3 times the restatement's own figures; this keeps them
    from growing unseen when the scene changes."""
    sc = SR.scene(degree, 20000, 7)
    c32 = SR.forward32(sc)
    passed = c32[:, :3] > 0
    gsh32, gp32 = SR.backward32(sc)
    gsh64, gp64, _ = SR.backward64(sc, passed)
    e_c = float(SR.color_units(sc, c32, SR.colors64(sc)).max())
    e_s = float(SR.grad_sh_units(sc, gsh32, gsh64, passed).max())
    e_p = float(SR.grad_pos_units(sc, gp32, gp64, passed).max())
    print(f"degree {degree}: float32 restatement colour {e_c:.2f}, grad_sh {e_s:.2f}, grad_positions {e_p:.2f} units of 2^-24")
    assert np.isfinite(c32).all() and np.isfinite(gsh32).all() and np.isfinite(gp32).all()
    assert e_c <= RESTATEMENT_UNITS and e_s <= RESTATEMENT_UNITS and e_p <= RESTATEMENT_UNITS
    if degree == 0:
        assert not gp32.any() and not gp64.any()
    else:
        assert e_p > 0


@pytest.mark.parametrize("degree", [0, 1, 2, 3])
def test_edge_scene_reaches_the_edge(degree):
    """edge_scene() puts at least 200 channels on each side of the clamp's edge within 4 colour units of it, and at degree 0 at
    least 200 whose binary32 sum is exactly 0: where `>` and `>=` differ."""
    sc = SR.edge_scene(degree, 11)
    above, below = SR.edge_counts(sc)
    exact = int((SR.sums32(sc) == 0).sum())
    print(f"degree {degree}: {sc.n} rows, {above} channels above the edge and {below} below it within 4 units; {exact} binary32 sums exactly 0")
    assert above >= 200 and below >= 200
    if degree == 0:
        assert exact >= 200


def test_measures_see_a_dropped_term_and_a_swapped_channel():
    """The measures are tight enough to matter: dropping the lowest-weight term of a colour, or reading one channel's coefficient
    for another's, is far outside 8 units on most of the scene."""
    sc = SR.scene(3, 2000, 7)
    ref = SR.colors64(sc)
    Y, _ = SR.basis64(SR.direction64(sc.eye, sc.pos)[0], 3)
    terms = Y[:, :, None] * sc.sh.astype(np.float64)
    k = np.abs(terms).argmin(axis=1)  # (n, 3) the smallest term of each channel
    dropped = 0.5 + terms.sum(axis=1) - np.take_along_axis(terms, k[:, None, :], axis=1)[:, 0, :]
    live = (ref[:, :3] > 0) & (dropped > 0)
    e = SR.color_units(sc, np.maximum(dropped, 0), ref)
    assert np.median(e[live]) > 100 * RESTATEMENT_UNITS
    swapped = sc.rows(sc.n)
    swapped.sh = sc.sh.copy()
    swapped.sh[:, 5, 1] = sc.sh[:, 5, 2]
    e = SR.color_units(sc, SR.forward32(swapped), ref)[:, 1]
    assert np.median(e[ref[:, 1] > 0]) > 100 * RESTATEMENT_UNITS
