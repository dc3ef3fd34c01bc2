"""Exact models of the two forward composites' transmittance updates for ellipsoid records, and hand-built list stacks whose
last entry leaves T within a few ulps of T_STOP (include/splat.h: a pixel stops after the entry with 1 - T >= 0.99, i.e.
T <= T_STOP).

For an entry with footprint value g (the hardware exp2's binary32 result) and opacity o the two kernels compute
  k_composite     a = rn(g o);  w = rn(T a);  T' = rn(T - w)          (csrc/composite_quadrant.h: g *= opacity; T -= T * g)
  k_composite_px  w = rn(T g);  T' = rn(T - o w)  (one fused rounding) (csrc/composite_px.hip: T = fma(-opacity, T * g, T))
where rn is binary32 round-to-nearest-even.  Both are restated here in exact rational arithmetic (fractions), so a stack found
by search() is known to straddle T_STOP under one order and not the other without trusting any floating-point library.

A stack is list positions 0 .. k-1 at one pixel, all with the same footprint value g: body entries that take T down to just
above the stop, one final entry whose opacity was searched, and a witness entry (opacity 0.5) that a pixel consumes only if the
final entry did not stop it."""
from fractions import Fraction

import numpy as np

T_STOP = float.fromhex("0x1.47ae4p-7")  # composite.h: the last transmittance that stops a pixel
WITNESS_OPACITY = 0.5
O_BODY_MAX = float(np.float32(0.95))
# stack footprints: (B00 = B11, centre offset along x); the offsets keep g = exp(-4.5 d2) from being a binary32 value and >= 0.5
GEOMS = [(0.7, 0.25), (0.6, 0.375), (0.55, 0.3125)]


def rn32(x):
    """The binary32 value nearest to the rational x (ties to even), as a Fraction.  Normal range only (what T, g and o reach)."""
    x = Fraction(x)
    if x == 0:
        return Fraction(0)
    s = -1 if x < 0 else 1
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert -126 <= e <= 127, "outside binary32's normal range"
    scale = Fraction(2) ** (23 - e)  # 24 significant bits
    m = a * scale
    q, r = divmod(m.numerator, m.denominator)
    if 2 * r > m.denominator or (2 * r == m.denominator and q & 1):
        q += 1
    return s * Fraction(q) / scale


def f32(x):
    """A float (or Fraction) that is a binary32 value, as a Fraction (asserting it is one)."""
    v = Fraction(float(np.float32(x)))
    assert v == (x if isinstance(x, Fraction) else Fraction(float(x))), f"{x!r} is not a binary32 value"
    return v


def step_quadrant(T, g, o):
    """k_composite's update: rn(T - rn(T rn(g o)))."""
    a = rn32(g * o)
    return rn32(T - rn32(T * a))


def step_px(T, g, o):
    """k_composite_px's update: rn(T - o rn(T g)), the subtraction fused."""
    return rn32(T - o * rn32(T * g))


STEP = {"quadrant": step_quadrant, "px": step_px}


def walk(g, opacities, order):
    """(consumed count, T after each consumed entry) of a stack under one update order; stops after T <= T_STOP."""
    T, Ts = Fraction(1), []
    gs, stop = f32(g), Fraction(T_STOP)
    for k, o in enumerate(opacities):
        T = STEP[order](T, gs, f32(o))
        Ts.append(T)
        if T <= stop:
            return k + 1, Ts
    return len(opacities), Ts


def ulps_from_stop(T):
    """Signed distance of T from T_STOP in binary32 ulps at T_STOP (2^-30)."""
    return float((Fraction(T) - Fraction(T_STOP)) * 2 ** 30)


def search(g, rng, want=8, tries=400, max_ulps=4):
    """Stacks (lists of binary32 opacities, final entry second to last, witness last) for footprint value g whose final entry
    leaves T within max_ulps of T_STOP under both orders, returned with a kind: "split" (one order stops at the final entry,
    the other does not), "both" (both stop) or "neither".  Up to `want` split stacks and want // 2 of each other kind."""
    gs, stop = f32(g), Fraction(T_STOP)
    out, kinds = [], {"split": 0, "both": 0, "neither": 0}
    quota = {"split": want, "both": max(want // 2, 1), "neither": max(want // 2, 1)}
    for _ in range(tries):
        if all(kinds[k] >= quota[k] for k in kinds):
            break
        body, T = [], {o: Fraction(1) for o in STEP}
        while True:  # body entries until the next one at opacity 0.95 would stop the pixel under either order
            o = float(np.float32(rng.uniform(0.3, O_BODY_MAX)))
            if any(STEP[k](T[k], gs, f32(O_BODY_MAX)) <= stop for k in STEP):
                break
            nT = {k: STEP[k](T[k], gs, f32(o)) for k in STEP}
            if any(v <= stop for v in nT.values()):
                break
            body.append(o)
            T = nT
        # the final opacity that would put T exactly on T_STOP (quadrant order), then its binary32 neighbours
        o0 = np.float32(float((1 - stop / T["quadrant"]) / gs))
        if not (0 < o0 <= 1):
            continue
        cands = [o0]
        for _k in range(12):
            cands.append(np.nextafter(cands[-1], np.float32(2)))
        lo = o0
        for _k in range(12):
            lo = np.nextafter(lo, np.float32(0))
            cands.append(lo)
        for o in cands:
            o = float(o)
            if not (0 < o <= 1):
                continue
            Tq, Tp = step_quadrant(T["quadrant"], gs, f32(o)), step_px(T["px"], gs, f32(o))
            if abs(ulps_from_stop(Tq)) > max_ulps or abs(ulps_from_stop(Tp)) > max_ulps:
                continue
            sq, sp = Tq <= stop, Tp <= stop
            kind = "split" if sq != sp else ("both" if sq else "neither")
            if kinds[kind] < quota[kind]:
                kinds[kind] += 1
                out.append((kind, body + [o, WITNESS_OPACITY]))
                break
    return out


def g_candidates(d2):
    """The binary32 values the hardware exp2 may return for exp(-4.5 d2) (d2 binary32): the float64 value rounded, and its two
    binary32 neighbours (v_exp_f32 is accurate to 1 ulp)."""
    arg = np.float32(d2) * np.float32(-6.492127684000335)  # binary32, as the kernels form it
    e = np.float32(np.exp2(np.float64(arg)))
    return [np.nextafter(e, np.float32(0)), e, np.nextafter(e, np.float32(2))]
