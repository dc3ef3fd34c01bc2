"""A NumPy reference for splat_composite_contribution (include/splat.h, "Contribution of every splat to a frame"): per splat the
hit count, the largest and the summed blend weight over the (pixel, consumed entry inside the cut) pairs of a frame.

The pairs are the ones tests/ellipsoid_grad_ref.decisions recorded (the binary32 composite's own choices: the cut and the
early-out stop); their weights w = T alpha are replayed with a float64 T per pixel from the recorded binary32 alphas.  Where the
kernel's rounding may choose differently (the rim and near pixels of `decisions`), callers mask the pixel on both sides.
"""
import numpy as np

Q = 2.0 ** -24  # the unit of weight_sum_u64


def clamp_mask(mask, width, height):
    """The kernel's pixel mask as float64 (H W,): clamped to [0, 1], NaN -> 0; all ones for None."""
    if mask is None:
        return np.ones(width * height)
    m = np.asarray(mask, np.float32).reshape(-1).astype(np.float64)
    assert m.shape[0] == width * height
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(m), 0.0, np.clip(m, 0.0, 1.0))


def contribution(dec, n, width, height, mask=None, min_weight=0.0):
    """dec: decisions(...)'s result.  Returns dict(hits_lo, hits_hi (n,) int64: the count lies in [lo, hi] - a pair whose wm is
    within 1e-5 min_weight + 1e-7 of the threshold may fall either side; the bracket is a point for min_weight = 0), wmax, wsum
    (n,) float64 and pairs (n,) int64, the number of pairs with a mask > 0."""
    m = clamp_mask(mask, width, height)
    T = np.ones(width * height)
    lo, hi, pairs = (np.zeros(n, np.int64) for _ in range(3))
    wmax, wsum = np.zeros(n), np.zeros(n)
    tol = 1e-5 * min_weight + 1e-7 if min_weight > 0 else 0.0
    for (pix, s, _stop), a in zip(dec["steps"], dec["alpha"]):
        if pix.size == 0:
            continue
        a = a.astype(np.float64)
        w = T[pix] * a          # (a pixel appears at most once per list position)
        T[pix] = T[pix] * (1.0 - a)
        on = m[pix] > 0
        wm, s = (m[pix] * w)[on], s[on]
        np.add.at(pairs, s, 1)
        np.maximum.at(wmax, s, wm)
        np.add.at(wsum, s, wm)
        np.add.at(lo, s[wm >= min_weight + tol], 1)
        np.add.at(hi, s[wm >= min_weight - tol], 1)
    return dict(hits_lo=lo, hits_hi=hi, wmax=wmax, wsum=wsum, pairs=pairs)


def brute_force(rec, color_opacity, indices, counts, offsets, width, height, mask=None, min_weight=0.0, tile=16):
    """The same statistic by a plain loop over pixels and list entries (binary32 decisions as ellipsoid_ref.composite makes them,
    float64 T), independent of `decisions`: dict(hits, wmax, wsum, pairs) with hits at the threshold itself (no bracket)."""
    from oracle import np_oracle as NO
    F = np.float32
    rec = np.asarray(rec, F)
    col = np.asarray(color_opacity, F)
    bnd, okb = NO.disc_bounds(rec)
    n = rec.shape[0]
    m = clamp_mask(mask, width, height)
    ntx = -(-width // tile)
    hits, pairs = np.zeros(n, np.int64), np.zeros(n, np.int64)
    wmax, wsum = np.zeros(n), np.zeros(n)
    for y in range(height):
        for x in range(width):
            t = (y // tile) * ntx + x // tile
            pxf, pyf = F(x) + F(0.5), F(y) + F(0.5)
            T32, T64 = F(1), 1.0
            for k in range(int(counts[t])):
                s = int(indices[int(offsets[t]) + k])
                r, b = rec[s], bnd[s]
                dx, dy = pxf - r[0], pyf - r[1]
                with np.errstate(all="ignore"):
                    uu, vv = r[2] * dx + r[3] * dy, r[4] * dx + r[5] * dy
                    d2 = uu * uu + vv * vv
                    g = F(col[s, 3] * np.exp(F(-4.5) * d2))
                inside = not (pxf < b[0] or pxf > b[2] or pyf < b[1] or pyf > b[3])
                take = bool(okb[s]) and inside and bool(d2 <= F(1))
                g = g if take else F(0)
                if take and m[y * width + x] > 0:
                    wm = m[y * width + x] * T64 * float(g)
                    pairs[s] += 1
                    wmax[s] = max(wmax[s], wm)
                    wsum[s] += wm
                    hits[s] += wm >= min_weight
                T64 *= 1.0 - float(g)
                T32 = F(T32 * (F(1) - g))
                if (F(1) - T32) >= F(0.99):
                    break
    return dict(hits=hits, wmax=wmax, wsum=wsum, pairs=pairs)


def select(score, threshold=None, keep=None):
    """prune_by_importance's rule on a NumPy score array: ascending kept indices.  threshold: score >= threshold; keep: an int
    count or a float fraction of n rounded down (at least 1) of the highest scores, ties to the lower index (a stable sort)."""
    score = np.asarray(score)
    n = score.shape[0]
    if threshold is not None:
        return np.nonzero(score.astype(np.float64) >= threshold)[0]
    k = min(n, max(1, int(np.floor(keep * n)))) if isinstance(keep, float) else min(n, int(keep))
    order = np.argsort(-score.astype(np.float64), kind="stable")[:k]
    return np.sort(order)
