"""The specification of include/splat.h's "MCMC relocation" block as NumPy and Python integers, written from the rules and not
from the kernels: the 24-bit integer weights, the draws (exact big-integer arithmetic), the opacity and scale correction of a
relocation (float64), its application to the planes and their moments, and the per-step noise (float64).  Philox4x32-10, the
Box-Muller transform and the rotation matrix are tests/density_ref.py's.
"""
import math

import numpy as np

from tests import density_ref as DR

RELOCATE, ADD = 1, 2  # the modes; also the third word of a draw's Philox counter
NOISE_STREAM = 3
NMAX = 51
PLANES = ("means", "log_scales", "rotations", "opacity_logits", "sh")
BINOM = [[math.comb(a, k) for k in range(NMAX)] for a in range(NMAX)]
OPACITY_MAX = 1.0 - 2.0 ** -23


def q_min(min_opacity):
    return int(math.ceil(float(min_opacity) * 2.0 ** 24))


def scaled_opacity(logits):
    """2^24 sigmoid(logit) in float64 (NaN for a NaN logit): what the weights are the floor of."""
    with np.errstate(all="ignore"):
        return 1.0 / (1.0 + np.exp(-np.asarray(logits, np.float32).astype(np.float64))) * 2.0 ** 24


def weights(logits, min_opacity):
    """(q, dead, weight): q = floor(2^24 o) as int64 (0 for a NaN logit), dead = q < q_min, weight = q where alive, else 0."""
    x = scaled_opacity(logits)
    q = np.where(np.isnan(x), 0.0, np.floor(x)).astype(np.int64)
    dead = q < q_min(min_opacity)
    return q, dead, np.where(dead, 0, q)


def sample(logits, mode, n_draws, seed, min_opacity):
    """(targets, sources, counts, (dead, alive, draws made)): the draws of splat_mcmc_sample, with Python integers."""
    n = len(logits)
    _, dead, w = weights(logits, min_opacity)
    cum, total = [], 0
    for x in w.tolist():
        total += x
        cum.append(total)
    n_dead = int(dead.sum())
    counts = np.zeros(n, np.uint32)
    if mode == RELOCATE:
        targets = np.flatnonzero(dead).astype(np.uint32)
    else:
        targets = (n + np.arange(n_draws)).astype(np.uint32)
    draws = len(targets)
    if total == 0 or draws == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.uint32), counts, (n_dead, n - n_dead, 0)
    ctr = np.zeros((draws, 4), np.uint32)
    ctr[:, 0], ctr[:, 2] = np.arange(draws), mode
    x = DR.philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32))
    r = [int(a) | (int(b) << 32) for a, b in zip(x[:, 0].tolist(), x[:, 1].tolist())]
    t = np.array([(ri * total) >> 64 for ri in r], np.uint64)  # < T < 2^54
    sources = np.searchsorted(np.array(cum, np.uint64), t, side="right").astype(np.uint32)  # the smallest i with C_i > t
    np.add.at(counts, sources, 1)
    return targets, sources, counts, (n_dead, n - n_dead, draws)


def relocation(o, N):
    """(o', D) in float64: the opacity of each of N copies that composite to o, and the scale ratio's denominator (the new
    scale is the old one times o / D)."""
    o = float(o)
    on = 1.0 - (1.0 - o) ** (1.0 / N)
    D = 0.0
    for a in range(1, N + 1):
        s = 0.0
        for k in range(a):
            s += BINOM[a - 1][k] * (-1.0) ** k * on ** (k + 1) / math.sqrt(k + 1)
        D += s
    return on, D


def new_values(logit, c, min_opacity):
    """(new logit, log(o / D)) in float64 for a source with float32 logit `logit` drawn c > 0 times."""
    o = 1.0 / (1.0 + math.exp(-float(np.float32(logit))))
    on, D = relocation(o, min(c + 1, NMAX))
    oc = min(max(on, float(min_opacity)), OPACITY_MAX)
    return math.log(oc) - math.log(1.0 - oc), math.log(o / D)


def apply(planes, m, v, targets, sources, counts, min_opacity):
    """splat_mcmc_apply on dicts of arrays keyed by PLANES (`planes` with the target rows present).  Returns (planes, m, v,
    touched): copies with means, rotations, sh and the moments in their own dtype (bit moves and exact zeros) and
    opacity_logits, log_scales as float64 (the unrounded new values; untouched rows the float32 inputs); touched: the rows
    written."""
    out = {k: np.array(planes[k], np.float64 if k in ("opacity_logits", "log_scales") else None) for k in PLANES}
    m, v = {k: np.array(m[k]) for k in PLANES}, {k: np.array(v[k]) for k in PLANES}
    rows = out["means"].shape[0]
    touched = np.zeros(rows, bool)
    drawn = np.flatnonzero(np.asarray(counts) > 0)
    new = {int(i): new_values(planes["opacity_logits"][i], int(counts[i]), min_opacity) for i in drawn}
    old_ls = np.asarray(planes["log_scales"], np.float64)
    for t, s in zip(np.asarray(targets).tolist(), np.asarray(sources).tolist()):  # (A)
        for k in ("means", "rotations", "sh"):
            out[k][t] = planes[k][s]
        out["opacity_logits"][t] = new[s][0]
        out["log_scales"][t] = old_ls[s] + new[s][1]
        touched[t] = True
    for i in drawn.tolist():  # (B)
        out["opacity_logits"][i] = new[i][0]
        out["log_scales"][i] = old_ls[i] + new[i][1]
        touched[i] = True
    for k in PLANES:
        m[k][touched] = 0
        v[k][touched] = 0
    return out, m, v, touched


def noise(log_scales, rotations, logits, scale, step, seed):
    """(delta (n, 3), bound terms): what splat_mcmc_noise adds to the means, in float64, and per splat sigma_max^2 |xi|_2 g scale
    (the magnitude its error bound is stated in), g and the opacity."""
    n = len(logits)
    ls = np.asarray(log_scales, np.float32).astype(np.float64)
    with np.errstate(all="ignore"):
        o = 1.0 / (1.0 + np.exp(-np.asarray(logits, np.float32).astype(np.float64)))
        g = 1.0 / (1.0 + np.exp(-100.0 * (0.005 - o)))
    ctr = np.zeros((n, 4), np.uint32)
    ctr[:, 0], ctr[:, 1], ctr[:, 2] = np.arange(n), step, NOISE_STREAM
    x = DR.philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], np.uint32))
    u = (x.astype(np.float64) + 0.5) * 2.0 ** -32
    ra, rb = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    xi = np.stack([ra * np.cos(2 * np.pi * u[:, 1]), ra * np.sin(2 * np.pi * u[:, 1]), rb * np.cos(2 * np.pi * u[:, 3])], axis=1)
    R = DR.rotation_matrices(np.asarray(rotations, np.float32))
    cov = np.einsum("nij,nj,nkj->nik", R, np.exp(2.0 * ls), R)
    s = float(np.float32(scale))
    delta = np.einsum("nij,nj->ni", cov, xi) * (g * s)[:, None]
    magnitude = np.exp(2.0 * ls).max(axis=1) * np.sqrt((xi * xi).sum(axis=1)) * g * s
    return delta, magnitude, g, o
