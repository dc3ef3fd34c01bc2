"""The specification of include/splat.h's "Density control and optimiser" block as NumPy, written from the rules and not from
the kernels: Philox4x32-10, the Box-Muller normals of a split, the per-frame statistics, the densification plan, its
application, and Adam.  float64 throughout, except where the contract itself is stated in binary32 (visible(): one rounding
per operation) or in integers (Philox, the plan's layout).
"""
import numpy as np

F = np.float32
LOG_SHRINK = np.log(1.6)
KEPT, COPY, CHILD0, CHILD1 = 0, 1, 2, 3  # a row's kind (bits 30-31)
PARENT_MASK = 0x3FFFFFFF


def philox4x32_10(counter, key):
    """counter (..., 4), key (..., 2) uint32 -> (..., 4) uint32 (Salmon et al., SC'11)."""
    c = [np.asarray(counter, np.uint32)[..., j].astype(np.uint64) for j in range(4)]
    k = [np.asarray(key, np.uint32)[..., j].astype(np.uint64) for j in range(2)]
    c = list(np.broadcast_arrays(*c))
    mask = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & mask]
        k = [(k[0] + np.uint64(0x9E3779B9)) & mask, (k[1] + np.uint64(0xBB67AE85)) & mask]
    return np.stack(c, axis=-1).astype(np.uint32)


def split_normals(parent, k, seed):
    """(len(parent), 3) float64: xi_k of the split of `parent` under `seed` (counter (parent, k, 0, 0), key (seed low, seed high))."""
    parent = np.asarray(parent, np.uint32)
    ctr = np.zeros(parent.shape + (4,), np.uint32)
    ctr[..., 0], ctr[..., 1] = parent, np.asarray(k, np.uint32)
    x = philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32))
    u = (x.astype(np.float64) + 0.5) * 2.0 ** -32
    ra, rb = np.sqrt(-2.0 * np.log(u[..., 0])), np.sqrt(-2.0 * np.log(u[..., 2]))
    return np.stack([ra * np.cos(2 * np.pi * u[..., 1]), ra * np.sin(2 * np.pi * u[..., 1]), rb * np.cos(2 * np.pi * u[..., 3])], axis=-1)


def rotation_matrices(q):
    """(n, 3, 3) float64 of quaternions (w, x, y, z) of any non-zero length."""
    q = np.asarray(q, np.float64)
    q = q / np.sqrt((q * q).sum(axis=1, keepdims=True))
    w, x, y, z = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)], axis=1),
                     np.stack([2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)], axis=1),
                     np.stack([2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], axis=1)], axis=1)


def visible(rec, width, height):
    """(mask (n,) bool, radius (n,) float64).  The mask is the contract's binary32 decision, one rounding per operation:
    not the all-zero record, and c -/+ (hx, hy) overlaps [0, W) x [0, H); the radius max(hx, hy) is float64."""
    r = np.asarray(rec, F)
    with np.errstate(all="ignore"):
        b00, b01, b11 = r[:, 2], r[:, 3], r[:, 5]
        hx = np.sqrt(b01 * b01 + b11 * b11) / (b00 * b11)
        hy = F(1) / b11
        on = (r != 0).any(axis=1) & (r[:, 0] + hx > 0) & (r[:, 0] - hx < F(width)) & (r[:, 1] + hy > 0) & (r[:, 1] - hy < F(height))
        d = r.astype(np.float64)
        radius = np.maximum(np.sqrt(d[:, 3] ** 2 + d[:, 5] ** 2) / (d[:, 2] * d[:, 5]), 1.0 / d[:, 5])
    return on, radius


def accumulate(rec, grec, width, height, grad_accum, denom, max_radius):
    """One frame: returns (mask uint8, grad_accum, denom, max_radius), the three as new float64 arrays."""
    on, radius = visible(rec, width, height)
    g = np.asarray(grec, np.float64)
    ga, dn, mr = (np.array(a, np.float64) for a in (grad_accum, denom, max_radius))
    ga[on] += np.hypot(g[on, 0] * width / 2, g[on, 1] * height / 2)
    dn[on] += 1
    mr[on] = np.maximum(mr[on], radius[on])
    return on.astype(np.uint8), ga, dn, mr


def plan_quantities(log_scales, logits, grad_accum, denom):
    """g, s, o per splat in float64 (NaN kept: np.max propagates it)."""
    with np.errstate(all="ignore"):
        dn = np.asarray(denom, np.float64)
        g = np.where(dn > 0, np.asarray(grad_accum, np.float64) / np.where(dn > 0, dn, 1), 0.0)
        s = np.exp(np.max(np.asarray(log_scales, np.float64), axis=1))
        o = 1.0 / (1.0 + np.exp(-np.asarray(logits, np.float64)))
    return g, s, o


def plan(log_scales, logits, grad_accum, denom, max_radius, grad_threshold, scale_threshold, min_opacity, max_screen_radius=0.0,
         max_world_scale=0.0, max_splats=0):
    """(rows uint32, counts {pruned, kept, cloned, split}, refused indices) by the rules, splat by splat."""
    g, s, o = plan_quantities(log_scales, logits, grad_accum, denom)
    r = np.asarray(max_radius, np.float64)
    n = g.shape[0]
    with np.errstate(all="ignore"):
        dead = ~(o >= min_opacity)
        if max_screen_radius > 0:
            dead |= r > max_screen_radius
        if max_world_scale > 0:
            dead |= ~(s <= max_world_scale)
        wants = ~dead & (g >= grad_threshold)
        big = s > scale_threshold
    survivors = int((~dead).sum())
    rows, refused = [], []
    counts = dict(pruned=n - survivors, kept=0, cloned=0, split=0)
    granted = 0
    for i in range(n):
        if dead[i]:
            continue
        if wants[i] and (max_splats == 0 or survivors + granted < max_splats):
            granted += 1
            if big[i]:
                rows += [i | (CHILD0 << 30), i | (CHILD1 << 30)]
                counts["split"] += 1
            else:
                rows += [i, i | (COPY << 30)]
                counts["cloned"] += 1
        else:
            if wants[i]:
                refused.append(i)
            rows.append(i)
            counts["kept"] += 1
    return np.array(rows, np.uint32), counts, np.array(refused, np.int64)


def apply_rows(rows, plane, zero_new=False):
    """splat_densify_rows: every row its parent's; zero_new: zeros for kinds 1-3."""
    rows = np.asarray(rows, np.uint32)
    out = np.asarray(plane)[(rows & PARENT_MASK).astype(np.int64)].copy()
    if zero_new:
        out[(rows >> 30) != 0] = 0
    return out


def apply_geometry(rows, means, log_scales, rotations, seed):
    """splat_densify_geometry in float64: (means_out, log_scales_out)."""
    rows = np.asarray(rows, np.uint32)
    parent, kind = (rows & PARENT_MASK).astype(np.int64), rows >> 30
    mu, ls = np.asarray(means, np.float64)[parent].copy(), np.asarray(log_scales, np.float64)[parent].copy()
    child = kind >= 2
    if child.any():
        p = parent[child]
        xi = split_normals(p, kind[child] - 2, seed)
        R = rotation_matrices(np.asarray(rotations)[p])
        mu[child] += np.einsum("nij,nj->ni", R, np.exp(ls[child]) * xi)
        ls[child] -= LOG_SHRINK
    return mu, ls


def adam(p, m, v, g, t, lr, beta1=0.9, beta2=0.999, eps=1e-15, mask=None):
    """Step t (1-based) of torch's Adam (no amsgrad, no weight decay) in float64; lr a scalar or an array broadcast over p.
    mask (rows,): rows with 0 keep p, m, v.  Returns new (p, m, v)."""
    p, m, v, g = (np.array(a, np.float64) for a in (p, m, v, g))
    m2 = beta1 * m + (1 - beta1) * g
    v2 = beta2 * v + (1 - beta2) * g * g
    p2 = p - (lr / (1 - beta1 ** t)) * m2 / (np.sqrt(v2) / np.sqrt(1 - beta2 ** t) + eps)
    if mask is not None:
        on = np.asarray(mask).astype(bool).reshape((-1,) + (1,) * (p.ndim - 1))
        p2, m2, v2 = np.where(on, p2, p), np.where(on, m2, m), np.where(on, v2, v)
    return p2, m2, v2
