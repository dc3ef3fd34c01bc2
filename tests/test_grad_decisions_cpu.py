"""CPU checks of tests/grad_decisions_ref.py: its exact binary32 rounding, and that the stacks it builds really straddle T_STOP
under the two forward kernels' update orders (exact rational arithmetic, no floating-point library trusted)."""
from fractions import Fraction

import numpy as np
import pytest

from tests import grad_decisions_ref as DR


def test_rn32_is_binary32_rounding():
    rng = np.random.default_rng(0)
    a = rng.uniform(1e-3, 1, 2000).astype(np.float32)
    b = rng.uniform(1e-3, 1, 2000).astype(np.float32)
    for x, y in zip(a, b):
        assert DR.rn32(Fraction(float(x)) * Fraction(float(y))) == Fraction(float(x * y))
        assert DR.rn32(Fraction(float(x)) - Fraction(float(y))) == Fraction(float(x - y))
    # ties go to even
    one = Fraction(1)
    assert DR.rn32(one + Fraction(1, 2 ** 24)) == one
    assert DR.rn32(one + Fraction(3, 2 ** 24)) == one + Fraction(4, 2 ** 24)
    assert DR.f32(DR.T_STOP) == Fraction(DR.T_STOP) and float(np.float32(1) - np.float32(DR.T_STOP)) >= 0.99


def test_the_two_orders_are_the_kernels_own():
    rng = np.random.default_rng(1)
    for _ in range(500):
        T, g, o = (np.float32(v) for v in rng.uniform(0.005, 1, 3))
        want_q = np.float32(T - np.float32(T * np.float32(g * o)))  # separate binary32 operations
        assert DR.step_quadrant(Fraction(float(T)), Fraction(float(g)), Fraction(float(o))) == Fraction(float(want_q))
        w = np.float32(T * g)
        d64 = np.float64(T) - np.float64(o) * np.float64(w)  # o w is exact in binary64; the difference usually is too
        want_p = np.float32(d64)
        got_p = DR.step_px(Fraction(float(T)), Fraction(float(g)), Fraction(float(o)))
        if Fraction(float(d64)) == Fraction(float(T)) - Fraction(float(o)) * Fraction(float(w)):
            assert got_p == Fraction(float(want_p))  # one rounding, numpy's: the fused update exactly
        else:  # (binary64 rounded first: at most one binary32 ulp apart)
            assert abs(got_p - Fraction(float(want_p))) <= abs(Fraction(float(want_p))) * Fraction(1, 2 ** 23)


@pytest.mark.parametrize("geom", DR.GEOMS)
def test_crafted_stacks_straddle_t_stop(geom):
    """For every value the hardware exp2 may return for the geometry, the stacks the GPU test builds: each final entry leaves T
    within 4 ulps of T_STOP under both orders, the "split" ones stop under exactly one of them (the witness entry after it is
    consumed under the other), and there are split stacks stopping under each order."""
    b, dl = geom
    u = np.float32(np.float32(b) * np.float32(-dl))
    d2 = np.float32(u * u)
    for g in DR.g_candidates(d2):
        assert 0.5 <= g < 1
        stacks = DR.search(float(g), np.random.default_rng(7), want=12)
        kinds = [k for k, _ in stacks]
        assert kinds.count("split") >= 6 and "both" in kinds and "neither" in kinds
        stopped_by = set()
        for kind, ops in stacks:
            n = len(ops)
            Lq, Tq = DR.walk(g, ops, "quadrant")
            Lp, Tp = DR.walk(g, ops, "px")
            for L, Ts in ((Lq, Tq), (Lp, Tp)):
                assert L >= n - 1  # nothing before the final entry stops the pixel
                assert abs(DR.ulps_from_stop(Ts[n - 2])) <= 4
            if kind == "split":
                assert {Lq, Lp} == {n - 1, n}
                stopped_by.add("quadrant" if Lq == n - 1 else "px")
            else:
                assert Lq == Lp == (n - 1 if kind == "both" else n)
        assert stopped_by == {"quadrant", "px"}
