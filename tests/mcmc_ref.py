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


# ---- clouds past 256 block sums: the second and third trip of the 64-bit scan of the block sums --------------------------------

SCAN_TILE, SCAN_TRIP = 2048, 256 * 2048  # weights per block sum; weights per trip of k_scan64_sums (256 block sums): 524 288
FAR_SIZES = (SCAN_TRIP, SCAN_TRIP + 1, 1229577)  # 256 block sums (one trip, full), 257, 601 (three trips, the last partial)
FAR_CASES = tuple(f"n={n}" for n in FAR_SIZES) + ("saturated", "alive past two trips", "alive in the first block")


def normal_logits(n, seed):
    return np.random.default_rng(seed).normal(-1.0, 2.5, n).astype(np.float32)


def off_integers(logits, margin=1e-6):
    """(logits, moved): the logits with every finite one whose 2^24 o lies within `margin` of an integer replaced by the next
    float32 above it, until none is left.  Among a million random logits about two lie that close (2 margin each), and floor()
    of such a value is the one thing two correct implementations may disagree on (tests/test_gpu_mcmc.py, "sample"): the
    clouds are kept clear of it instead of excusing it.  One float32 step moves 2^24 o by thousands of margins."""
    logits = np.array(logits, np.float32)
    moved = 0
    while True:
        x = scaled_opacity(logits)
        near = np.flatnonzero(np.isfinite(logits) & (np.abs(x - np.round(x)) < margin))
        if near.size == 0:
            return logits, moved
        logits[near] = np.nextafter(logits[near], np.float32(np.inf))
        moved += near.size


def far_case(name):
    """(logits, (lo, hi) of the rows that may be alive) of the clouds of FAR_CASES.  The sized ones are normal_logits(n, 100 + n);
    `saturated`: every logit 17, every weight 2^24 - 1; the last two: N(1, 1) logits on [2^20, n) or on [0, 2048) and -20 (dead,
    weight 0) everywhere else, so that the first two trips' totals, or every block sum after the first, are 0."""
    n = FAR_SIZES[2]
    if name.startswith("n="):
        n = int(name[2:])
        return off_integers(normal_logits(n, 100 + n))[0], (0, n)
    if name == "saturated":
        return np.full(n, 17.0, np.float32), (0, n)
    lo, hi = {"alive past two trips": (2 * SCAN_TRIP, n), "alive in the first block": (0, SCAN_TILE)}[name]
    logits = np.full(n, -20.0, np.float32)
    logits[lo:hi] = np.random.default_rng(300 + lo).normal(1.0, 1.0, hi - lo).astype(np.float32)
    return off_integers(logits)[0], (lo, hi)


def far_case_regime(name, logits, alive, sources, min_opacity):
    """Asserts, from the restatement alone, that a cloud of FAR_CASES with the `sources` of its 5000 added draws reaches what it
    is there for; returns (cumulative weight at the end of the first trip, total weight, draws with a source past the first
    trip).  The draws past the first trip are asked for from n = 1 229 577 on: at 524 289 ONE splat lies past it."""
    n = len(logits)
    q, dead, w = weights(logits, min_opacity)
    first, total = int(w[:SCAN_TRIP].sum()), int(w.sum())
    past = int((sources >= SCAN_TRIP).sum())
    blocks = -(-n // SCAN_TILE)
    lo, hi = alive
    assert not w[:lo].any() and not w[hi:].any() and ((sources >= lo) & (sources < hi)).all(), f"{name}: a source outside [{lo}, {hi})"
    if name.startswith("n="):
        assert blocks == {FAR_SIZES[0]: 256, FAR_SIZES[1]: 257, FAR_SIZES[2]: 601}[n]
        assert first > 2 ** 32, f"{name}: the carry out of the first trip fits 32 bits"
        if n == FAR_SIZES[2]:
            assert past >= 1000, f"{name}: {past} of {len(sources)} draws have a source past the first trip"
    elif name == "saturated":
        assert (q == 2 ** 24 - 1).all() and total == n * (2 ** 24 - 1) and total > 2e13 and past >= 1000
    elif name == "alive past two trips":
        assert int(w[:2 * SCAN_TRIP].sum()) == 0 and total > 2 ** 32 and past == len(sources)
    else:
        assert int(w[SCAN_TILE:].sum()) == 0 and first == total > 2 ** 32 and past == 0 and blocks == 601
    return first, total, past
